// The fused upsample + cross-entropy (+ gradient) of headloss.hip (K = 19) and classes.hip (any
// K <= 256) with F.cross_entropy's other arguments: class weights, label smoothing, a per-pixel
// weight (OHEM's keep mask, or the incoming gradient of reduction="none") and the per-pixel loss
// map.  The plain kernels stay where they are, untouched; these are their optioned forms, with the
// same bands, the same thread-to-pixel map and the same fixed summation orders, so that with
// neutral options the loss sum, the count and the gradient are bitwise the plain kernels'.
//
// For a valid pixel, P = softmax(u), w the class weights, Wsum = sum w, e the smoothing, q the pixel weight:
//     l     = (1 - e) w_t (-log P_t) + (e / K) sum_k w_k (-log P_k)
//     dl/du = (1 - e) w_t (P - onehot_t) + (e / K) (P Wsum - w)
//           = P cp - onehot_t ca - cs w        cp = (1 - e) w_t + (e / K) Wsum, ca = (1 - e) w_t, cs = e / K
// so a pixel carries three scalars (q folded in) where the plain kernels carry 1 / sum-exp, and the
// expression keeps the plain kernels' shape (exp * scalar - select): without smoothing and with
// w = q = 1 it is the same arithmetic.  The smoothing sum needs no second walk over the classes:
//     sum_k w_k (-log P_k) = Wsum lse - sum_k w_k u_k
// is one more running scalar per pixel (K = 19: sum_k w_k (u_k - max), the pixel's values being
// at hand).  The class weights are read through wave-uniform indices (scalar loads), never staged
// per thread; w_t, the one per-pixel read, comes from a copy in LDS.
//
// pixel_loss is cleared by a stream-ordered memset before the launch, then every valid pixel's one
// owner thread writes l (without q).  GRAD = false is the forward-only form: no second pass, no
// tiles, no merge.  Both kernels write their gradient tiles in classes.hip's layout and share its merge
// launch (ce_band.h, with the band geometry and the staging) and one sums launch, in headloss.hip's orders.
//
// Registers (gfx950, -O3; VGPRs, no AGPRs, no scratch anywhere; waves per SIMD in brackets), bf16
// logits, the other dtypes within 2 VGPRs:
//                        weights, grad   smoothed, grad   weights, forward   smoothed, forward
//     ce19_opt_kernel    251 (2)         256 (2)          107 (4)            123 (4)
//     ce_opt_kernel      254 (2)         183 (2)          143 (3)            150 (3)
// (the plain kernels: 234 at CK = 16.)  Every form holds 2 waves per SIMD; ce19_opt_kernel asks for
// them (amdgpu_waves_per_eu), without which its smoothed form took one AGPR past 256 and fell to 1.
// The gradient forms also keep 11 to 48 scalar registers in VGPR lanes (v_writelane; not scratch).  The
// smoothed ce19_opt_kernel sits exactly at 256, so the Makefile reads the compiler's resource remarks for
// this file and fails the build if any kernel here uses scratch or falls to 1 wave per SIMD.
// Smoothing is a template argument of its own: the forms differ by up to 70 registers either way, and
// the -w term is placed per column in ce19_opt_kernel (per pixel it needed 264 registers) and per
// pixel in ce_opt_kernel (per block it needed 259).
#include "ce_band.h"

namespace {

constexpr int K_MAX = DCLIP_CLASSES_MAX;
constexpr int NPART = 4;  // doubles of loss partials per workgroup: sum q l, sum q w_t, #valid, (pad)

struct CeOpt {
    const float* cw;  // K class weights or null
    const float* pw;  // (B, H, W) pixel weights or null
    float* pl;        // (B, H, W) pixel loss or null
    float eps;        // label smoothing
};

// l0 * a + l1 * b with both products rounded before the sum.  The plain 19-class kernel's build evaluates
// its per-pixel interpolation this way (the two products are paired into one packed multiply and the
// sum stays an add), while here the same expression would be contracted into a fused multiply-add: one
// rounding less, and neutral options would no longer repeat the plain kernel bit for bit.
__device__ __forceinline__ float lerp_rounded(float l0, float a, float l1, float b) {
#pragma clang fp contract(off)
    return l0 * a + l1 * b;
}

// the workgroup's three loss partials: wave sums (fixed butterfly), then the 4 waves in order
__device__ __forceinline__ void store_partials(double a, double a2, double c, double (&red_s)[NTH / 64][3],
                                               double* __restrict__ part) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        a2 += __shfl_xor(a2, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    if ((tid & 63) == 0) {
        red_s[tid >> 6][0] = a;
        red_s[tid >> 6][1] = a2;
        red_s[tid >> 6][2] = c;
    }
    __syncthreads();
    if (tid < 3) {
        double s = 0.0;
        for (int wv = 0; wv < NTH / 64; ++wv) s += red_s[wv][tid];
        part[(int64_t)blockIdx.x * NPART + tid] = s;
    }
}

// ============================================================================ K = 19, register-resident
// band_fold_kernel MODE 0 (headloss.hip) with the options.  part: [nwg][NPART] f64;
// tiles: [B][h][2][band_cols][K] f32
template <typename TL, bool SMOOTH, bool GRAD>
__global__ __launch_bounds__(NTH) __attribute__((amdgpu_waves_per_eu(2))) void ce19_opt_kernel(const TL* __restrict__ low, int h, int w, int H, int W,
                                                       int chunks, const void* __restrict__ lab, int lab_dt,
                                                       int ignore, CeOpt o, double* __restrict__ part,
                                                       float* __restrict__ tiles) {
    constexpr int K = 19;
    static_assert(NTH == JW * 8, "32 low-res columns x 8 column slices");
    __shared__ float low_s[2][JW + 1][K];  // the band's two low-res rows over the chunk (+1 column)
    __shared__ float g_s[4][JW][K];        // per low-res column: left-upper, right-upper, left-lower, right-lower
    __shared__ double red_s[NTH / 64][3];
    __shared__ float cw_s[K];  // the class weights, for the one per-pixel read: the target's
    const int tid = threadIdx.x;
    const int wg = blockIdx.x;
    const int ch = wg % chunks;
    const int i = (wg / chunks) % h;
    const int b = wg / (chunks * h);
    const int jc = ch * JW;
    const int i1 = i + (i < h - 1 ? 1 : 0);
    const int ncol = (jc + JW + 1 <= w ? JW + 1 : w - jc);
    if (tid < K) cw_s[tid] = o.cw ? o.cw[tid] : 1.f;
    for (int e = tid; e < 2 * (JW + 1) * K; e += NTH) {
        const int r = e / ((JW + 1) * K), jj = (e / K) % (JW + 1), k = e % K;
        const int row = r ? i1 : i;
        low_s[r][jj][k] = jj < ncol ? (float)low[(((int64_t)b * K + k) * h + row) * w + jc + jj] : 0.f;
    }
    __syncthreads();
    // the class weights of the smoothing terms: uniform indices, scalar loads
    const float* __restrict__ cwp = o.cw;
    auto cw = [&](int k) { return cwp ? cwp[k] : 1.f; };
    float Wsum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) Wsum += cw(k);
    const float om = 1.f - o.eps, cs = o.eps / (float)K;
    const int jj = tid >> 3, xs = tid & 7;
    const int j0 = jc + jj;
    int ylo, yhi;
    band_range(i, h, H, &ylo, &yhi);
    double lsum = 0.0, lwsum = 0.0;
    unsigned lcnt = 0;
    float g[4][K];  // folded gradient: 0: left-upper, 1: right-upper, 2: left-lower, 3: right-lower
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < K; ++k) g[q][k] = 0.f;
    if (j0 < w) {
        int xlo, xhi;
        band_range(j0, w, W, &xlo, &xhi);
        for (int x = xlo + xs; x <= xhi; x += 8) {
            const Lerp X = lerp_index(x, w, W);
            if (X.i0 != j0) continue;
            const int j1 = X.i1 - jc;
            float ut[K], ub[K], at[K], ab[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                ut[k] = X.l0 * low_s[0][jj][k] + X.l1 * low_s[0][j1][k];
                ub[k] = X.l0 * low_s[1][jj][k] + X.l1 * low_s[1][j1][k];
                at[k] = 0.f;
                ab[k] = 0.f;
            }
            float sq0 = 0.f, sq1 = 0.f;  // the column's sums of q e / K by row weight: the -w term, added once
            // the column's labels and pixel weights 8 rows at a time, all loads in flight together
            for (int y0 = ylo; y0 <= yhi; y0 += 8) {
                int tl[8];
                float tq[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int y = y0 + u;
                    const int64_t pix = ((int64_t)b * H + (y <= yhi ? y : yhi)) * W + x;
                    tl[u] = y <= yhi ? load_label(lab, lab_dt, pix) : ignore;
                    tq[u] = o.pw ? o.pw[pix] : 1.f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int y = y0 + u;
                    if (y > yhi) continue;
                    const Lerp Y = lerp_index(y, h, H);
                    if (Y.i0 != i) continue;
                    const int t = tl[u];
                    if (t == ignore || t < 0 || t >= K) continue;
                    float v[K];
#pragma unroll
                    for (int k = 0; k < K; ++k) v[k] = lerp_rounded(Y.l0, ut[k], Y.l1, ub[k]);
                    float m = v[0], vt = 0.f;
                    const float wt = cw_s[t];
#pragma unroll
                    for (int k = 1; k < K; ++k) m = fmaxf(m, v[k]);
#pragma unroll
                    for (int k = 0; k < K; ++k) vt = k == t ? v[k] : vt;
                    float s = 0.f, sw = 0.f;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        if constexpr (SMOOTH) sw += cw(k) * (v[k] - m);
                        v[k] = __expf(v[k] - m);
                        s += v[k];
                    }
                    const float ls = __logf(s);
                    const float nll = ls - (vt - m);  // -log softmax[t]
                    const float ca = SMOOTH ? om * wt : wt;
                    float l = ca * nll;
                    if constexpr (SMOOTH) l += cs * (Wsum * ls - sw);
                    const float q = tq[u];
                    if (o.pl) o.pl[((int64_t)b * H + y) * W + x] = l;
                    lsum += (double)q * (double)l;
                    lwsum += (double)(q * wt);
                    ++lcnt;
                    if constexpr (GRAD) {
                        const float qa = q * ca;
                        const float sp = (1.0f / s) * (SMOOTH ? q * (ca + cs * Wsum) : qa);
                        if constexpr (SMOOTH) {
                            sq0 += Y.l0 * (q * cs);
                            sq1 += Y.l1 * (q * cs);
                        }
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const float d = v[k] * sp - (k == t ? qa : 0.f);
                            at[k] += Y.l0 * d;
                            ab[k] += Y.l1 * d;
                        }
                    }
                }
            }
            if constexpr (GRAD) {
                if constexpr (SMOOTH) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        at[k] -= sq0 * cw(k);
                        ab[k] -= sq1 * cw(k);
                    }
                }
                if (j1 == jj) {  // clamped right edge: both weights on one column
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        g[0][k] += at[k];
                        g[2][k] += ab[k];
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        g[0][k] += X.l0 * at[k];
                        g[1][k] += X.l1 * at[k];
                        g[2][k] += X.l0 * ab[k];
                        g[3][k] += X.l1 * ab[k];
                    }
                }
            }
        }
    }
    if constexpr (GRAD) {
        // the column's 8 slices (8 adjacent lanes): a xor butterfly, the same order on every run
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                float v = g[q][k];
                v += __shfl_xor(v, 1, 64);
                v += __shfl_xor(v, 2, 64);
                v += __shfl_xor(v, 4, 64);
                g[q][k] = v;
            }
        if (xs == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int k = 0; k < K; ++k) g_s[q][jj][k] = g[q][k];
        }
    }
    store_partials(lsum, lwsum, (double)lcnt, red_s, part);  // its barrier also publishes g_s
    if constexpr (GRAD) {  // the chunk's gradient tile (rows i, i1 x the chunk's ncol columns)
        const int64_t bc = band_cols(w, chunks);
        float* trow = tiles + ((((int64_t)b * h + i) * 2) * bc + (int64_t)ch * (JW + 1)) * K;
        for (int e = tid; e < 2 * ncol * K; e += NTH) {
            const int r = e / (ncol * K), jx = (e / K) % ncol, k = e % K;
            float v = 0.f;
            if (!(r == 1 && i1 == i)) {
                // low-res column jx: its own left weights, then column jx - 1's right weights
                v = (jx < JW ? g_s[2 * r][jx][k] : 0.f) + (jx > 0 ? g_s[2 * r + 1][jx - 1][k] : 0.f);
                if (r == 0 && i1 == i)  // last band: the lower row is the upper row
                    v += (jx < JW ? g_s[2][jx][k] : 0.f) + (jx > 0 ? g_s[3][jx - 1][k] : 0.f);
            }
            trow[((int64_t)r * bc + jx) * K + k] = v;
        }
    }
}

// ============================================================================ any K, chunked
// ce_classes_kernel (classes.hip) with the options.  After pass 1 the per-pixel arrays change
// meaning: s holds P's coefficient (1 / sum-exp folded in), wt the one-hot's, sw the weights'.
template <typename TL, bool SMOOTH, bool GRAD>
__global__ __launch_bounds__(NTH) void ce_opt_kernel(const TL* __restrict__ low, int K, int h, int w, int H, int W,
                                                     int chunks, const void* __restrict__ lab, int lab_dt,
                                                     int ignore, CeOpt o, double* __restrict__ part,
                                                     float* __restrict__ tiles) {
    __shared__ float low_s[2][CK][JW + 1];
    __shared__ float gr_s[2][CK][JW];  // the right-hand weights of each low-res column: upper, lower row
    __shared__ double red_s[NTH / 64][3];
    __shared__ float cw_s[K_MAX];  // the class weights, for the one per-pixel read: the target's
    const int tid = threadIdx.x;
    const int wg = blockIdx.x;
    const int ch = wg % chunks;
    const int i = (wg / chunks) % h;
    const int b = wg / (chunks * h);
    const int jc = ch * JW;
    const int i1 = i + (i < h - 1 ? 1 : 0);
    for (int k = tid; k < K; k += NTH) cw_s[k] = o.cw ? o.cw[k] : 1.f;  // published by the walk's first barrier
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
    double lsum = 0.0, lwsum = 0.0;
    unsigned lcnt = 0;
    float Wsum = 0.f;  // uniform
    if constexpr (SMOOTH)
        for (int k = 0; k < K; ++k) Wsum += o.cw ? o.cw[k] : 1.f;
    const float om = 1.f - o.eps, cs = o.eps / (float)K;
    // every thread walks its own column's [xlo, xhi] 8 outputs apart; the trip count is the workgroup's
    // widest, taken with a barrier vote so that the barriers inside stay uniform
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
            // pass 1: running max / sum-exp / target logit (/ sum w u) over the chunks
            float m[YB], s[YB], vt[YB], wt[YB], sw[SMOOTH ? YB : 1];
#pragma unroll
            for (int u = 0; u < YB; ++u) {
                m[u] = -INFINITY;
                s[u] = 0.f;
                vt[u] = 0.f;
                if constexpr (SMOOTH) sw[u] = 0.f;
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
                        if constexpr (SMOOTH) {
                            const float wk = k < kc ? (o.cw ? o.cw[k0 + k] : 1.f) : 0.f;  // uniform
                            sw[u] += wk * v[k];
                        }
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
                const int64_t pix = ((int64_t)b * H + y0 + u) * W + x;
                const float q = o.pw ? o.pw[pix] : 1.f;
                const float ls = __logf(s[u]);
                const float nll = ls - (vt[u] - m[u]);  // -log softmax[t]
                const float wtu = cw_s[tl[u]];
                const float ca = SMOOTH ? om * wtu : wtu;
                float l = ca * nll;
                if constexpr (SMOOTH) l += cs * (Wsum * (m[u] + ls) - sw[u]);
                if (o.pl) o.pl[pix] = l;
                lsum += (double)q * (double)l;
                lwsum += (double)(q * wtu);
                ++lcnt;
                const float qa = q * ca;
                s[u] = (1.0f / s[u]) * (SMOOTH ? q * (ca + cs * Wsum) : qa);
                wt[u] = qa;
                if constexpr (SMOOTH) sw[u] = q * cs;
            }
            if constexpr (GRAD) {
                // pass 2: the gradient of each chunk, folded through the transposed interpolation
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
                                float d = __expf(v - m[u]) * s[u] - (k == tk ? wt[u] : 0.f);
                                if constexpr (SMOOTH) {
                                    const float wk = k < kc ? (o.cw ? o.cw[k0 + k] : 1.f) : 0.f;  // uniform
                                    d -= sw[u] * wk;
                                }
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
                        for (int sh = 1; sh < 8; sh <<= 1) {
                            a0 += __shfl_xor(a0, sh, 64);
                            a1 += __shfl_xor(a1, sh, 64);
                            b0 += __shfl_xor(b0, sh, 64);
                            b1 += __shfl_xor(b1, sh, 64);
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
    }
    if constexpr (GRAD) {
        if (!touched) {  // no valid pixel in the band's chunk: its tile is zero
            const int64_t n = (int64_t)ncol * K;
            for (int64_t e = tid; e < 2 * n; e += NTH) (e < n ? trow0 : trow1 - n)[e] = 0.f;
        }
    }
    store_partials(lsum, lwsum, (double)lcnt, red_s, part);
}

// sums[0..1] / count += the workgroups' partials, in workgroup order within each thread's stripe,
// then a fixed LDS tree (the counts are integers below 2^53: exact)
__global__ __launch_bounds__(256) void ce_opt_sums_kernel(const double* __restrict__ part, int nwg,
                                                          double* __restrict__ sums, unsigned* __restrict__ count) {
    __shared__ double red[3][256];
    const int t = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int e = t; e < nwg; e += 256)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += part[(int64_t)e * NPART + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c][t] = s[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o)
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c][t] += red[c][t + o];
        __syncthreads();
    }
    if (t == 0) {
        sums[0] += red[0][0];
        sums[1] += red[1][0];
        count[0] += (unsigned)(red[2][0] + 0.5);
    }
}

int64_t ws_floats(int B, int K, int h, int w) {
    const int chunks = (w + JW - 1) / JW;
    const int64_t nwg = (int64_t)B * h * chunks;
    // the f64 partials first (8-byte aligned), then the tiles
    return nwg * 2 * NPART + (int64_t)B * h * 2 * band_cols(w, chunks) * K;
}

template <typename TL, bool SMOOTH, bool GRAD>
void launch(const void* low, int B, int K, int h, int w, int H, int W, const void* lab, int lab_dt, int ignore,
            const CeOpt& o, double* sums, unsigned* count, float* grad, float* ws, hipStream_t st) {
    const int chunks = (w + JW - 1) / JW;
    const int nwg = B * h * chunks;
    double* part = (double*)ws;
    float* tiles = ws + (int64_t)nwg * 2 * NPART;
    if (K == 19)
        ce19_opt_kernel<TL, SMOOTH, GRAD><<<nwg, NTH, 0, st>>>((const TL*)low, h, w, H, W, chunks, lab, lab_dt,
                                                               ignore, o, part, tiles);
    else
        ce_opt_kernel<TL, SMOOTH, GRAD><<<nwg, NTH, 0, st>>>((const TL*)low, K, h, w, H, W, chunks, lab, lab_dt,
                                                             ignore, o, part, tiles);
    if (sums != nullptr) ce_opt_sums_kernel<<<1, 256, 0, st>>>(part, nwg, sums, count);
    if constexpr (GRAD) {
        const int64_t total = (int64_t)B * K * h * w;
        int64_t blocks = (total + 255) / 256;
        blocks = blocks > 4096 ? 4096 : blocks;
        ce_classes_merge_kernel<<<(unsigned)blocks, 256, 0, st>>>(tiles, B, K, h, w, chunks, grad);
    }
}

}  // namespace

extern "C" int64_t dclip_upsample_ce_opt_ws_floats(int B, int K, int h, int w) {
    if (B <= 0 || K <= 0 || K > K_MAX || h <= 0 || w <= 0) return 0;
    return ws_floats(B, K, h, w);
}

extern "C" int dclip_upsample_ce_opt(int low_dt, const void* logits, int B, int K, int h, int w, const void* labels,
                                     int lab_dt, int H, int W, int ignore_index, const float* class_weight,
                                     float label_smoothing, const float* pixel_weight, float* pixel_loss,
                                     double* sums, unsigned* count, float* grad, float* ws, void* stream) {
    DCLIP_HOST_CHECK(K >= 1 && K <= K_MAX, "dclip_upsample_ce_opt: K=%d (1 <= K <= %d classes)", K, K_MAX);
    DCLIP_HOST_CHECK(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "dclip_upsample_ce_opt: bad sizes");
    DCLIP_HOST_CHECK(low_dt == DCLIP_F32 || low_dt == DCLIP_F16 || low_dt == DCLIP_BF16,
                     "dclip_upsample_ce_opt: low_dt=%d (f32, f16 or bf16)", low_dt);
    DCLIP_HOST_CHECK(lab_dt >= 0 && lab_dt <= 2,
                     "dclip_upsample_ce_opt: lab_dt=%d: labels int64 (0), int32 (1) or uint8 (2)", lab_dt);
    DCLIP_HOST_CHECK((int64_t)B * H * W < ((int64_t)1 << 31),
                     "dclip_upsample_ce_opt: B*H*W = %lld pixels (must be below 2^31)",
                     (long long)((int64_t)B * H * W));
    DCLIP_HOST_CHECK((int64_t)B * h * ((w + JW - 1) / JW) < ((int64_t)1 << 31),
                     "dclip_upsample_ce_opt: too many low-res bands");
    DCLIP_HOST_CHECK(label_smoothing >= 0.f && label_smoothing < 1.f,
                     "dclip_upsample_ce_opt: label_smoothing=%g (0 <= label_smoothing < 1)", (double)label_smoothing);
    DCLIP_HOST_CHECK(logits && labels, "dclip_upsample_ce_opt: logits and labels required");
    DCLIP_HOST_CHECK((sums == nullptr) == (count == nullptr),
                     "dclip_upsample_ce_opt: sums and count go together (both or neither)");
    DCLIP_HOST_CHECK(grad || pixel_loss || sums,
                     "dclip_upsample_ce_opt: no output: grad, pixel_loss or sums with count required");
    DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                     "dclip_upsample_ce_opt: ws (dclip_upsample_ce_opt_ws_floats(B, K, h, w) f32, 8-byte aligned) "
                     "required");
    hipStream_t st = (hipStream_t)stream;
    if (pixel_loss != nullptr) {  // 0 wherever no thread scores a pixel; the owners of the valid ones write after it
        hipError_t e = hipMemsetAsync(pixel_loss, 0, (size_t)B * H * W * sizeof(float), st);
        if (e != hipSuccess) {
            dclip_set_error("dclip_upsample_ce_opt: clearing pixel_loss: %s", hipGetErrorString(e));
            return DCLIP_ERR_HIP;
        }
    }
    const CeOpt o{class_weight, pixel_weight, pixel_loss, label_smoothing};
    const bool smooth = label_smoothing > 0.f;
#define CE_OPT_LAUNCH(S, G)                                                                                     \
    EVAL_DISPATCH_LOW(low_dt, (launch<TL, S, G>(logits, B, K, h, w, H, W, labels, lab_dt, ignore_index, o, sums, \
                                                count, grad, ws, st)))
    if (grad != nullptr) {
        if (smooth) CE_OPT_LAUNCH(true, true);
        else CE_OPT_LAUNCH(false, true);
    } else {
        if (smooth) CE_OPT_LAUNCH(true, false);
        else CE_OPT_LAUNCH(false, false);
    }
#undef CE_OPT_LAUNCH
    DCLIP_LAUNCH_CHECK();
    return 0;
}
