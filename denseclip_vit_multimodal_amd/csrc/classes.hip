// The fused head paths for any class count 1 <= K <= 256 (ADE20K's 150, ...): the score map, the
// fused upsample + cross-entropy (+ gradient) and the fused upsample + evaluation.  Their 19-class
// counterparts (misc.hip, headloss.hip, headeval.hip) hold a pixel's K values in registers and the
// K-channel low-res patch in LDS; here neither scales with K: the classes are walked in chunks of
// CK = 16, the low-res patch is staged per chunk, and what a pixel needs between chunks is a running
// (max, argmax, sum-exp, target logit).
//
// CK = 16 from the register budget: the CE kernel holds 5 arrays of CK floats per thread (the two
// x-interpolated rows, the two folded gradient rows, the pixel's values) plus 2 x CK folded column
// gradients and 8 pixels of running state: 234 VGPRs at CK = 16 (2 waves per SIMD, no scratch), and
// its arrays alone pass 256 at CK = 32; the evaluation kernel holds 4 pixels x CK values (158 / 175
// VGPRs).  LDS per workgroup: 16 x the tile's low-res patch (<= 48 KB, as at K = 19) for the
// evaluation, 8.4 KB for the CE.
//
//   score map:  score_map_kernel's product (misc.hip) with the class embeddings cut into 32-row
//               tiles on grid.z; every tile repeats the pixel norms from the same fragments in the
//               same order, so an all-zero pixel row scores 0 in every tile.
//   CE:         headloss.hip's bands (one low-res row x 32 low-res columns per workgroup, 32 x 8
//               threads).  A thread's pixels are taken 8 rows of one column at a time; per block an
//               online max / sum-exp / target-logit pass over the chunks, then a second pass that
//               recomputes each chunk's values, forms softmax - onehot and folds it through the
//               transposed interpolation: the 8 column slices by a xor butterfly, the right-hand
//               weights to the neighbouring column through LDS, then a read-modify-write of the
//               workgroup's gradient tile in the workspace by the one thread that owns the element
//               (no atomics; blocks and chunks in loop order).  The merge and the partial sums are
//               headloss.hip's, in the same fixed orders.
//   evaluation: headeval.hip's tile walk with eval_tile.h's chunked scoring (seg_score_chunk /
//               seg_score_finish).  K x K confusion cells do not fit LDS at K = 150, so the counts
//               go to one of HIST_REPLICAS u32 histograms in the workspace with integer atomics
//               (exact in any order; for K <= 32 a workgroup counts in LDS first and adds its cells
//               once); the CE sum keeps f32 terms, f64 partials and a fixed order.
#include "ce_band.h"

namespace {

constexpr int K_MAX = DCLIP_CLASSES_MAX;

// ============================================================================ score map
template <typename TV>
__global__ __launch_bounds__(256) void score_map_classes_kernel(const TV* __restrict__ v, int64_t bstride,
                                                                int64_t row_off, int64_t ld,
                                                                const float* __restrict__ t,
                                                                float* __restrict__ score, int HW, int C, int K,
                                                                float eps) {
    typedef typename Mfma<TV>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [32][C + 8] TV
    TV* tn = (TV*)smem;
    const int pitch = C + 8;
    const int b = blockIdx.y;
    const int k0 = blockIdx.z * 32;                   // this workgroup's class tile
    const int kn = K - k0 < 32 ? K - k0 : 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, hh = lane >> 5;
    // the tile's embedding norms: a wave per row, each lane's 16-byte chunks in order, then the
    // wave's fixed butterfly
    __shared__ float nrm[32];
    const f32x4* tb = (const f32x4*)(t + ((int64_t)b * K + k0) * C);
    const int c4 = C / 4;
    for (int k = wave; k < kn; k += 4) {
        float ss = 0.f;
        for (int j = lane; j < c4; j += 64) {
            const f32x4 x = tb[k * c4 + j];
            ss += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
        }
        ss = wave_sum(ss);
        if (lane == 0) nrm[k] = ss;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * c4; i += 256) {
        const int k = i / c4, c = 4 * (i - k * c4);
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (k < kn) x = tb[i] * (1.f / fmaxf(sqrtf(nrm[k]), eps));
        typedef TV t4 __attribute__((ext_vector_type(4)));
        *(t4*)(tn + k * pitch + c) = t4{(TV)x[0], (TV)x[1], (TV)x[2], (TV)x[3]};
    }
    __syncthreads();
    // one 32-pixel group per workgroup, its channels split over the 4 waves, the partial products
    // and norms summed through LDS in wave order
    float* red = (float*)(smem + (size_t)32 * pitch * sizeof(TV));  // [3][17][64]
    const int nsteps = C / 16, s0 = wave * nsteps / 4, s1 = (wave + 1) * nsteps / 4;
    const int p = blockIdx.x * 32 + l32;
    const int pc = p < HW ? p : HW - 1;
    const TV* row = v + (int64_t)b * bstride + (row_off + pc) * ld + 8 * hh;
    const TV* arow = tn + l32 * pitch + 8 * hh;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float ss = 0.f;
    for (int s = s0; s < s1; ++s) {
        const frag bf = *(const frag*)(row + 16 * s);
        const frag af = *(const frag*)(arow + 16 * s);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += (float)bf[j] * (float)bf[j];
        acc = Mfma<TV>::mma(af, bf, acc);
    }
    if (wave > 0) {
        float* r = red + (wave - 1) * 17 * 64;
#pragma unroll
        for (int e = 0; e < 16; ++e) r[e * 64 + lane] = acc[e];
        r[16 * 64 + lane] = ss;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int wv = 0; wv < 3; ++wv) {
            const float* r = red + wv * 17 * 64;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += r[e * 64 + lane];
            ss += r[16 * 64 + lane];
        }
        ss += __shfl_xor(ss, 32, 64);  // the other half-wave holds the pixel's other 8-column chunks
        const float inv = 1.f / fmaxf(sqrtf(ss), eps);
        if (p < HW) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (k < kn) score[((int64_t)b * K + k0 + k) * HW + p] = acc[r] * inv;
            }
        }
    }
}

// ============================================================================ fused CE
constexpr int NPART = 2;  // doubles of loss partials per workgroup: sum of -log p, #valid

// part: [nwg][NPART] f64; tiles: [B][h][2][band_cols][K] f32
template <typename TL>
__global__ __launch_bounds__(NTH) void ce_classes_kernel(const TL* __restrict__ low, int K, int h, int w, int H, int W,
                                                         int chunks, const void* __restrict__ lab,
                                                         int lab_dt, int ignore, double* __restrict__ part,
                                                         float* __restrict__ tiles) {
    __shared__ float low_s[2][CK][JW + 1];
    __shared__ float gr_s[2][CK][JW];  // the right-hand weights of each low-res column: upper, lower row
    __shared__ double red_s[NTH / 64][2];
    const int tid = threadIdx.x;
    const int wg = blockIdx.x;
    const int ch = wg % chunks;
    const int i = (wg / chunks) % h;
    const int b = wg / (chunks * h);
    const int jc = ch * JW;
    const int i1 = i + (i < h - 1 ? 1 : 0);
    const bool last_band = i1 == i;  // the lower row is the upper row: both fold into row 0
    const int ncol = (jc + JW + 1 <= w ? JW + 1 : w - jc);
    const int jj = tid >> 3, xs = tid & 7;
    const int j0 = jc + jj;
    int ylo, yhi;
    band_range(i, h, H, &ylo, &yhi);
    int xlo = 0, xhi = -1;
    if (j0 < w) band_range(j0, w, W, &xlo, &xhi);
    const int64_t bc = band_cols(w, chunks);
    float* trow0 = tiles + ((((int64_t)b * h + i) * 2) * bc + (int64_t)ch * (JW + 1)) * K;  // [jx][K]
    float* trow1 = trow0 + bc * K;
    const bool owner = xs == 0 && j0 < w;  // of tile column jj (and of column JW, for jj = JW - 1)
    bool touched = false;                  // uniform: the tile has been written
    double lsum = 0.0;
    unsigned lcnt = 0;
    // every thread walks its own column's [xlo, xhi] 8 outputs apart; the trip count is the workgroup's
    // widest (low-res column 0 also owns the outputs whose source is clamped at 0: about 1.5 W / w of
    // them), taken with a barrier vote so that the barriers inside stay uniform
    for (int it = 0; __syncthreads_or(xlo + xs + 8 * it <= xhi); ++it) {
        const int x = xlo + xs + 8 * it;
        bool colok = x <= xhi;
        const Lerp X = lerp_index(colok ? x : 0, w, W);
        colok = colok && X.i0 == j0;
        const int j1 = colok ? X.i1 - jc : jj;
        const bool edge = j1 == jj;  // clamped right edge: both weights on one column
        for (int y0 = ylo; y0 <= yhi; y0 += YB) {
            // the column's labels 8 rows at a time, all loads in flight together
            int tl[YB];
#pragma unroll
            for (int u = 0; u < YB; ++u) {
                const int y = y0 + u;
                tl[u] = (colok && y <= yhi) ? load_label(lab, lab_dt, ((int64_t)b * H + y) * W + x) : -1;
            }
            unsigned vmask = 0;
            float yl1[YB];
#pragma unroll
            for (int u = 0; u < YB; ++u) {
                const int y = y0 + u;
                const Lerp Y = lerp_index(y <= yhi ? y : yhi, h, H);
                yl1[u] = Y.l1;
                const int t = tl[u];
                if (colok && y <= yhi && Y.i0 == i && t != ignore && t >= 0 && t < K) vmask |= 1u << u;
            }
            if (!__syncthreads_or(vmask != 0)) continue;  // nothing to score in this block, for any thread
            // pass 1: running max / sum-exp / target logit over the chunks
            float m[YB], s[YB], vt[YB];
#pragma unroll
            for (int u = 0; u < YB; ++u) {
                m[u] = -INFINITY;
                s[u] = 0.f;
                vt[u] = 0.f;
            }
            for (int k0 = 0; k0 < K; k0 += CK) {
                const int kc = K - k0 < CK ? K - k0 : CK;
                __syncthreads();  // the previous chunk's readers are done
                stage_band(low_s, low, b, K, k0, h, w, i, i1, jc, ncol);
                __syncthreads();
                if (vmask == 0) continue;
                float ut[CK], ub[CK];
#pragma unroll
                for (int k = 0; k < CK; ++k) {
                    ut[k] = X.l0 * low_s[0][k][jj] + X.l1 * low_s[0][k][j1];
                    ub[k] = X.l0 * low_s[1][k][jj] + X.l1 * low_s[1][k][j1];
                }
#pragma unroll
                for (int u = 0; u < YB; ++u) {
                    if (!((vmask >> u) & 1u)) continue;
                    const float l1 = yl1[u], l0 = 1.f - l1;
                    const int tk = tl[u] - k0;
                    float v[CK];
                    float mn = m[u], vtu = vt[u];
#pragma unroll
                    for (int k = 0; k < CK; ++k) {
                        v[k] = l0 * ut[k] + l1 * ub[k];
                        if (k < kc) mn = fmaxf(mn, v[k]);
                        vtu = k == tk ? v[k] : vtu;
                    }
                    float su = s[u] * __expf(m[u] - mn);
#pragma unroll
                    for (int k = 0; k < CK; ++k)
                        if (k < kc) su += __expf(v[k] - mn);
                    m[u] = mn;
                    s[u] = su;
                    vt[u] = vtu;
                }
            }
#pragma unroll
            for (int u = 0; u < YB; ++u) {
                if (!((vmask >> u) & 1u)) continue;
                lsum += (double)(__logf(s[u]) - (vt[u] - m[u]));  // -log softmax[t]
                ++lcnt;
                s[u] = 1.0f / s[u];
            }
            // pass 2: softmax - onehot of each chunk, folded through the transposed interpolation
            for (int k0 = 0; k0 < K; k0 += CK) {
                const int kc = K - k0 < CK ? K - k0 : CK;
                __syncthreads();
                stage_band(low_s, low, b, K, k0, h, w, i, i1, jc, ncol);
                __syncthreads();
                float at[CK], ab[CK];
#pragma unroll
                for (int k = 0; k < CK; ++k) {
                    at[k] = 0.f;
                    ab[k] = 0.f;
                }
                if (vmask != 0) {
                    float ut[CK], ub[CK];
#pragma unroll
                    for (int k = 0; k < CK; ++k) {
                        ut[k] = X.l0 * low_s[0][k][jj] + X.l1 * low_s[0][k][j1];
                        ub[k] = X.l0 * low_s[1][k][jj] + X.l1 * low_s[1][k][j1];
                    }
#pragma unroll
                    for (int u = 0; u < YB; ++u) {
                        if (!((vmask >> u) & 1u)) continue;
                        const float l1 = yl1[u], l0 = 1.f - l1;
                        const int tk = tl[u] - k0;
#pragma unroll
                        for (int k = 0; k < CK; ++k) {
                            const float v = l0 * ut[k] + l1 * ub[k];
                            float d = __expf(v - m[u]) * s[u] - (k == tk ? 1.f : 0.f);
                            d = k < kc ? d : 0.f;
                            at[k] += l0 * d;
                            ab[k] += l1 * d;
                        }
                    }
                }
                // along x: left weights stay on column jj, right weights go to column jj + 1; the
                // column's 8 slices (8 adjacent lanes) by a xor butterfly, the same order on every run
                float glu[CK], gll[CK];
#pragma unroll
                for (int k = 0; k < CK; ++k) {
                    float a0 = edge ? at[k] : X.l0 * at[k], a1 = edge ? 0.f : X.l1 * at[k];
                    float b0 = edge ? ab[k] : X.l0 * ab[k], b1 = edge ? 0.f : X.l1 * ab[k];
#pragma unroll
                    for (int o = 1; o < 8; o <<= 1) {
                        a0 += __shfl_xor(a0, o, 64);
                        a1 += __shfl_xor(a1, o, 64);
                        b0 += __shfl_xor(b0, o, 64);
                        b1 += __shfl_xor(b1, o, 64);
                    }
                    glu[k] = a0;
                    gll[k] = b0;
                    if (xs == 0) {
                        gr_s[0][k][jj] = a1;
                        gr_s[1][k][jj] = b1;
                    }
                }
                __syncthreads();
                // tile column jx: its own left weights, then column jx - 1's right weights; every tile
                // element has one owner thread, which adds the blocks in loop order
                if (owner) {
#pragma unroll
                    for (int k = 0; k < CK; ++k) {
                        if (k >= kc) continue;
                        float u0 = glu[k] + (jj > 0 ? gr_s[0][k][jj - 1] : 0.f);
                        float u1 = gll[k] + (jj > 0 ? gr_s[1][k][jj - 1] : 0.f);
                        if (last_band) {
                            u0 += u1;
                            u1 = 0.f;
                        }
                        float* p0 = trow0 + (int64_t)jj * K + k0 + k;
                        float* p1 = trow1 + (int64_t)jj * K + k0 + k;
                        *p0 = touched ? *p0 + u0 : u0;
                        *p1 = touched ? *p1 + u1 : u1;
                    }
                    if (jj == JW - 1 && ncol == JW + 1) {
#pragma unroll
                        for (int k = 0; k < CK; ++k) {
                            if (k >= kc) continue;
                            float u0 = gr_s[0][k][JW - 1], u1 = gr_s[1][k][JW - 1];
                            if (last_band) {
                                u0 += u1;
                                u1 = 0.f;
                            }
                            float* p0 = trow0 + (int64_t)JW * K + k0 + k;
                            float* p1 = trow1 + (int64_t)JW * K + k0 + k;
                            *p0 = touched ? *p0 + u0 : u0;
                            *p1 = touched ? *p1 + u1 : u1;
                        }
                    }
                }
            }
            touched = true;
        }
    }
    if (!touched) {  // no valid pixel in the band's chunk: its tile is zero
        const int64_t n = (int64_t)ncol * K;
        for (int64_t e = tid; e < 2 * n; e += NTH) (e < n ? trow0 : trow1 - n)[e] = 0.f;
    }
    // loss partials: wave sums (fixed butterfly), then the 4 waves in order
    double a = lsum, c = (double)lcnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    if ((tid & 63) == 0) {
        red_s[tid >> 6][0] = a;
        red_s[tid >> 6][1] = c;
    }
    __syncthreads();
    if (tid < 2) {
        double sum = 0.0;
        for (int wv = 0; wv < NTH / 64; ++wv) sum += red_s[wv][tid];
        part[(int64_t)wg * NPART + tid] = sum;
    }
}

// loss_sum / count += the workgroups' partials, in workgroup order within each thread's stripe,
// then a fixed LDS tree (the counts are integers below 2^53: exact)
__global__ __launch_bounds__(256) void ce_classes_sums_kernel(const double* __restrict__ part, int nwg,
                                                              double* __restrict__ loss_sum,
                                                              unsigned* __restrict__ count) {
    __shared__ double red[2][256];
    const int t = threadIdx.x;
    double s[2] = {0.0, 0.0};
    for (int e = t; e < nwg; e += 256)
#pragma unroll
        for (int c = 0; c < 2; ++c) s[c] += part[(int64_t)e * NPART + c];
#pragma unroll
    for (int c = 0; c < 2; ++c) red[c][t] = s[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o)
#pragma unroll
            for (int c = 0; c < 2; ++c) red[c][t] += red[c][t + o];
        __syncthreads();
    }
    if (t == 0) {
        loss_sum[0] += red[0][0];
        count[0] += (unsigned)(red[1][0] + 0.5);
    }
}

int64_t ce_ws_floats(int B, int K, int h, int w) {
    const int chunks = (w + JW - 1) / JW;
    const int64_t nwg = (int64_t)B * h * chunks;
    // the f64 partials first (8-byte aligned), then the tiles
    return nwg * 2 * NPART + (int64_t)B * h * 2 * band_cols(w, chunks) * K;
}

template <typename TL>
void launch_ce(const void* low, int B, int K, int h, int w, int H, int W, const void* lab, int lab_dt, int ignore,
               double* loss_sum, unsigned* count, float* grad, float* ws, hipStream_t st) {
    const int chunks = (w + JW - 1) / JW;
    const int nwg = B * h * chunks;
    double* part = (double*)ws;
    float* tiles = ws + (int64_t)nwg * 2 * NPART;
    ce_classes_kernel<TL><<<nwg, NTH, 0, st>>>((const TL*)low, K, h, w, H, W, chunks, lab, lab_dt, ignore, part,
                                               tiles);
    ce_classes_sums_kernel<<<1, 256, 0, st>>>(part, nwg, loss_sum, count);
    const int64_t total = (int64_t)B * K * h * w;
    int64_t blocks = (total + 255) / 256;
    blocks = blocks > 4096 ? 4096 : blocks;
    ce_classes_merge_kernel<<<(unsigned)blocks, 256, 0, st>>>(tiles, B, K, h, w, chunks, grad);
}

// ============================================================================ fused evaluation
constexpr int HIST_REPLICAS = 32;  // u32 K x K histograms in ws; workgroup g counts into g % 32
constexpr int PART_BYTES = NWG_MAX * 2 * 8;  // per workgroup: CE partial, #valid (f64)
constexpr int HIST_LDS_K = 32;     // up to 32 x 32 cells (4 KB) a workgroup counts in LDS and adds once at its end

Tiling make_tiling(int B, int h, int w, int H, int W) {
    Tiling t;
    t.nrow = low_span(TH, h, H);
    t.tw = 128;
    t.ncol = low_span(t.tw, w, W);
    if ((int64_t)CK * t.nrow * t.ncol * 4 > LDS_TILE_MAX) {  // 16 x 11 x 67 floats fit at any scale >= 1
        t.tw = 64;
        t.ncol = low_span(t.tw, w, W);
    }
    t.lds = (size_t)CK * t.nrow * t.ncol * 4;
    finish_tiling(t, B, H, W);
    return t;
}

__global__ __launch_bounds__(256) void eval_classes_zero_kernel(unsigned* __restrict__ hist, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) hist[e] = 0u;
}

// LAB: labels given (confusion counts, CE sum, #valid); pred may be null then.  !LAB: pred only.
template <typename TL, bool LAB>
__global__ __launch_bounds__(256) void eval_seg_classes_kernel(const TL* __restrict__ low, int K, int h, int w, int H,
                                                               int W, Tiling tl, const void* __restrict__ lab,
                                                               int lab_dt, int ignore, int vec_lab, int vec_pred,
                                                               uint8_t* __restrict__ pred, char* __restrict__ ws) {
    extern __shared__ float low_s[];
    __shared__ double red_s[4 * 2];
    const int tid = threadIdx.x;
    const int xs = tl.tw >> 2;  // threads along x
    const int tx = tid % xs, ty = tid / xs;
    // few classes mean few cells and many pixels per cell: global atomics would queue on them, so the
    // workgroup counts in LDS and adds its non-zero cells to its replica once
    __shared__ unsigned hist_l[HIST_LDS_K * HIST_LDS_K];
    unsigned* hist = nullptr;
    unsigned* hist_g = nullptr;
    if constexpr (LAB) {
        hist_g = (unsigned*)(ws + PART_BYTES) + (int64_t)(blockIdx.x % HIST_REPLICAS) * K * K;
        hist = hist_g;
        if (K <= HIST_LDS_K) {
            for (int e = tid; e < K * K; e += blockDim.x) hist_l[e] = 0u;
            hist = hist_l;
            __syncthreads();
        }
    }
    double lsum = 0.0;
    unsigned nvalid = 0;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const TileGeom g = tile_geom(tile, tl, h, w, H, W);
        const int y = g.y0 + ty, x = g.x0 + 4 * tx;
        const bool active = y < H && x < W;  // the others only stage
        const int yc = active ? y : g.y0, xc = active ? x : g.x0;
        const int n = W - xc < 4 ? W - xc : 4;
        const int64_t pix = ((int64_t)g.b * H + yc) * W + xc;
        int t[4] = {-1, -1, -1, -1};
        if constexpr (LAB)
            if (active) load_labels4(lab, lab_dt, pix, n, vec_lab != 0, t);
        const Lerp Y = lerp_index(yc, h, H);
        int r0 = Y.i0 - g.ilo, r1 = Y.i1 - g.ilo;
        r0 = r0 < g.nr ? r0 : g.nr - 1;
        r1 = r1 < g.nr ? r1 : g.nr - 1;
        Lerp X[4];
        int c0[4], c1[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            X[p] = lerp_index(xc + p < W ? xc + p : W - 1, w, W);
            c0[p] = X[p].i0 - g.jlo;
            c1[p] = X[p].i1 - g.jlo;
            c0[p] = c0[p] < g.nc ? c0[p] : g.nc - 1;
            c1[p] = c1[p] < g.nc ? c1[p] : g.nc - 1;
        }
        SegRun<4> run;
        run.reset();
        for (int k0 = 0; k0 < K; k0 += CK) {
            const int kc = K - k0 < CK ? K - k0 : CK;
            __syncthreads();  // the previous chunk's readers are done
            stage_patch_chunk(low_s, low, g.b, K, k0, kc, h, w, g.ilo, g.nr, g.jlo, g.nc, tl.nrow, tl.ncol);
            __syncthreads();
            if (!active) continue;
            float v[4][CK];
#pragma unroll
            for (int k = 0; k < CK; ++k) {
                const int ks = k < kc ? k : 0;  // never read LDS past the staged classes
                const float* top = low_s + (ks * tl.nrow + r0) * tl.ncol;
                const float* bot = low_s + (ks * tl.nrow + r1) * tl.ncol;
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    v[p][k] = bilerp(Y.l0, Y.l1, X[p].l0, X[p].l1, top[c0[p]], top[c1[p]], bot[c0[p]], bot[c1[p]]);
            }
            seg_score_chunk<CK, 4, LAB>(v, k0, kc, t, run);
        }
        if (!active) continue;
        int am[4];
        seg_score_finish<4, LAB>(run, K, t, n, ignore, hist, lsum, nvalid, am);
        store_pred4(pred, pix, n, vec_pred != 0, am);
    }
    if constexpr (LAB) {
        double a[2] = {lsum, (double)nvalid};
        wg_partials<2>(a, red_s, (double*)(ws + (int64_t)blockIdx.x * 16));  // __syncthreads inside: LDS adds landed
        if (K <= HIST_LDS_K)
            for (int e = tid; e < K * K; e += blockDim.x) {
                const unsigned c = hist_l[e];
                if (c != 0u) atomicAdd(&hist_g[e], c);
            }
    }
}

// cm += the replicas in order (one cell per thread); workgroup 0 also adds the workgroups' CE
// partials and counts, in workgroup order within each thread's stripe, then a fixed LDS tree
__global__ __launch_bounds__(256) void eval_seg_classes_fold_kernel(const char* __restrict__ ws, int nwg, int K,
                                                                    int64_t* __restrict__ cm,
                                                                    double* __restrict__ loss_sum,
                                                                    unsigned long long* __restrict__ count) {
    const int t = threadIdx.x;
    const int cells = K * K;
    const unsigned* hist = (const unsigned*)(ws + PART_BYTES);
    const int c = blockIdx.x * 256 + t;
    if (c < cells) {
        unsigned long long s = 0;
        for (int r = 0; r < HIST_REPLICAS; ++r) s += hist[(int64_t)r * cells + c];
        cm[c] += (int64_t)s;
    }
    if (blockIdx.x != 0) return;
    __shared__ double red[2][256];
    double s[2] = {0.0, 0.0};
    for (int e = t; e < nwg; e += 256) {
        s[0] += ((const double*)ws)[2 * e];
        s[1] += ((const double*)ws)[2 * e + 1];
    }
    red[0][t] = s[0];
    red[1][t] = s[1];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            red[0][t] += red[0][t + o];
            red[1][t] += red[1][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        loss_sum[0] += red[0][0];
        count[0] += (unsigned long long)(red[1][0] + 0.5);
    }
}

template <typename TL>
void launch_eval(const void* low, int B, int K, int h, int w, int H, int W, const void* lab, int lab_dt, int ignore,
                 uint8_t* pred, int64_t* cm, double* loss_sum, unsigned long long* count, void* ws, hipStream_t st) {
    const Tiling tl = make_tiling(B, h, w, H, W);
    const int nth = (tl.tw / 4) * TH;
    const int vec_lab = labels_aligned(lab, lab_dt, W), vec_pred = pred_aligned(pred, W);
    if (lab != nullptr) {
        const int64_t ncell = (int64_t)HIST_REPLICAS * K * K;
        int64_t zb = (ncell + 255) / 256;
        zb = zb > 1024 ? 1024 : zb;
        eval_classes_zero_kernel<<<(unsigned)zb, 256, 0, st>>>((unsigned*)((char*)ws + PART_BYTES), ncell);
        eval_seg_classes_kernel<TL, true><<<tl.nwg, nth, tl.lds, st>>>((const TL*)low, K, h, w, H, W, tl, lab, lab_dt,
                                                                       ignore, vec_lab, vec_pred, pred, (char*)ws);
        eval_seg_classes_fold_kernel<<<(K * K + 255) / 256, 256, 0, st>>>((const char*)ws, tl.nwg, K, cm, loss_sum,
                                                                          count);
    } else {
        eval_seg_classes_kernel<TL, false><<<tl.nwg, nth, tl.lds, st>>>((const TL*)low, K, h, w, H, W, tl, nullptr, 0,
                                                                        ignore, 0, vec_pred, pred, (char*)ws);
    }
}

}  // namespace

#define CLASSES_K_CHECK(NAME) \
    DCLIP_HOST_CHECK(K >= 1 && K <= K_MAX, NAME ": K=%d (1 <= K <= %d classes)", K, K_MAX)

extern "C" int dclip_score_map_classes(const void* v, int v_dt, int64_t bstride, int64_t row_off, int64_t ld,
                                       const float* t, float* score, int B, int HW, int C, int K, float eps,
                                       void* stream) {
    CLASSES_K_CHECK("dclip_score_map_classes");
    DCLIP_HOST_CHECK(v_dt == DCLIP_BF16 || v_dt == DCLIP_F16, "dclip_score_map_classes: v must be f16/bf16");
    DCLIP_HOST_CHECK(C > 0 && C % 16 == 0 && C <= 2048 && ld % 8 == 0 && bstride % 8 == 0 && ((uintptr_t)v % 16) == 0,
                     "dclip_score_map_classes: C %% 16 == 0, C <= 2048, 16-byte aligned rows");
    DCLIP_HOST_CHECK(B > 0 && HW > 0, "dclip_score_map_classes: empty input");
    DCLIP_HOST_CHECK(B <= 65535, "dclip_score_map_classes: B=%d (at most 65535)", B);
    DCLIP_HOST_CHECK(v && t && score, "dclip_score_map_classes: v, t and score required");
    const dim3 grid((HW + 31) / 32, B, (K + 31) / 32);
    const size_t lds = (size_t)32 * (C + 8) * 2 + 3 * 17 * 64 * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    if (v_dt == DCLIP_BF16)
        score_map_classes_kernel<bf16><<<grid, 256, lds, st>>>((const bf16*)v, bstride, row_off, ld, t, score, HW, C, K,
                                                               eps);
    else
        score_map_classes_kernel<f16><<<grid, 256, lds, st>>>((const f16*)v, bstride, row_off, ld, t, score, HW, C, K,
                                                              eps);
    DCLIP_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t dclip_upsample_ce_classes_ws_floats(int B, int K, int h, int w) {
    if (B <= 0 || K <= 0 || K > K_MAX || h <= 0 || w <= 0) return 0;
    return ce_ws_floats(B, K, h, w);
}

extern "C" int dclip_upsample_ce_classes(int low_dt, const void* logits, int B, int K, int h, int w,
                                         const void* labels, int lab_dt, int H, int W, int ignore_index,
                                         double* loss_sum, unsigned* count, float* grad, float* ws, void* stream) {
    CLASSES_K_CHECK("dclip_upsample_ce_classes");
    DCLIP_HOST_CHECK(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "dclip_upsample_ce_classes: bad sizes");
    DCLIP_HOST_CHECK(low_dt == DCLIP_F32 || low_dt == DCLIP_F16 || low_dt == DCLIP_BF16,
                     "dclip_upsample_ce_classes: low_dt=%d (f32, f16 or bf16)", low_dt);
    DCLIP_HOST_CHECK(lab_dt >= 0 && lab_dt <= 2,
                     "dclip_upsample_ce_classes: lab_dt=%d: labels int64 (0), int32 (1) or uint8 (2)", lab_dt);
    DCLIP_HOST_CHECK((int64_t)B * h * ((w + JW - 1) / JW) < ((int64_t)1 << 31),
                     "dclip_upsample_ce_classes: too many low-res bands");
    DCLIP_HOST_CHECK(logits && labels, "dclip_upsample_ce_classes: logits and labels required");
    DCLIP_HOST_CHECK(loss_sum && count && grad, "dclip_upsample_ce_classes: outputs required");
    DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                     "dclip_upsample_ce_classes: ws (dclip_upsample_ce_classes_ws_floats(B, K, h, w) f32, 8-byte "
                     "aligned) required");
    hipStream_t st = (hipStream_t)stream;
    EVAL_DISPATCH_LOW(low_dt, launch_ce<TL>(logits, B, K, h, w, H, W, labels, lab_dt, ignore_index, loss_sum, count,
                                            grad, ws, st));
    DCLIP_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t dclip_upsample_eval_seg_classes_ws_bytes(int B, int K, int h, int w) {
    if (B <= 0 || K <= 0 || K > K_MAX || h <= 0 || w <= 0) return 0;
    return (int64_t)PART_BYTES + (int64_t)HIST_REPLICAS * K * K * 4;
}

extern "C" int dclip_upsample_eval_seg_classes(int low_dt, const void* logits, int B, int K, int h, int w,
                                               const void* labels, int lab_dt, int H, int W, int ignore_index,
                                               uint8_t* pred, int64_t* cm, double* loss_sum,
                                               unsigned long long* count, void* ws, void* stream) {
    CLASSES_K_CHECK("dclip_upsample_eval_seg_classes");
    DCLIP_HOST_CHECK(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "dclip_upsample_eval_seg_classes: bad sizes");
    DCLIP_HOST_CHECK(low_dt == DCLIP_F32 || low_dt == DCLIP_F16 || low_dt == DCLIP_BF16,
                     "dclip_upsample_eval_seg_classes: low_dt=%d (f32, f16 or bf16)", low_dt);
    DCLIP_HOST_CHECK(H >= h && W >= w,
                     "dclip_upsample_eval_seg_classes: the output (%d x %d) must not be smaller than the input "
                     "(%d x %d)", H, W, h, w);
    DCLIP_HOST_CHECK((int64_t)B * H * W < ((int64_t)1 << 31),
                     "dclip_upsample_eval_seg_classes: B*H*W = %lld pixels (must be below 2^31)",
                     (long long)((int64_t)B * H * W));
    DCLIP_HOST_CHECK(logits != nullptr, "dclip_upsample_eval_seg_classes: logits required");
    if (int rc = check_seg_outputs("dclip_upsample_eval_seg_classes", labels, lab_dt, pred, cm, loss_sum, count))
        return rc;
    if (labels != nullptr)
        DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                         "dclip_upsample_eval_seg_classes: ws (dclip_upsample_eval_seg_classes_ws_bytes(B, K, h, w) "
                         "bytes, 8-byte aligned) required");
    hipStream_t st = (hipStream_t)stream;
    EVAL_DISPATCH_LOW(low_dt, launch_eval<TL>(logits, B, K, h, w, H, W, labels, lab_dt, ignore_index, pred, cm,
                                              loss_sum, count, ws, st));
    DCLIP_LAUNCH_CHECK();
    return 0;
}
