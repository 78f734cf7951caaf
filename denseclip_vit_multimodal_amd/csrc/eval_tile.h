// What the fused head evaluation kernels share (headeval.hip: one low-res map per output pixel;
// headensemble.hip: V of them; headslide.hip: the windows that cover it; headslidetta.hip: the
// windows of V views).  Each kernel keeps what is its own: the patches it stages, its taps, its
// slot-to-pixel map and its accumulation over views / windows.  Here:
//   * before the values: the resize's source index, the tile's origin and low-res patch and its LDS
//     staging, the interpolation with its fused multiply-adds spelled out, the windows' rounded
//     division and host-side coverage check;
//   * after them, the scoring epilogue, once: the 4-pixel label load, argmax / CE / confusion counts
//     (seg_score), the depth terms (DepthSums), the class-map and depth-map stores, the per-workgroup
//     record in the caller's workspace and the one-workgroup folds;
//   * the host side the four files repeat: the tiling's tail, the alignment flags, the argument
//     checks of the labels-given / labels-absent and target-given / target-absent calls, the
//     dispatch on the low-res dtype.
// Everything here has internal linkage: each translation unit that includes it compiles its own copy.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int NWG_MAX = 1024;  // workgroups of the grid-stride walk (4 per CU)
constexpr int TH = 8;          // output rows per tile (one per thread row)
constexpr int NSUM = 12;       // f64 sums of the depth pass (dclip.h); the seg pass uses the first
constexpr int LDS_TILE_MAX = 48 * 1024;

struct Lerp {
    int i0, i1;
    float l0, l1;
};
// PyTorch upsample_bilinear2d, align_corners=False: headloss.hip's lerp_index, restated
__device__ __forceinline__ Lerp lerp_index(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Lerp r;
    r.i0 = (int)src;
    if (r.i0 > in - 1) r.i0 = in - 1;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = src - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

// low-res rows (columns) a run of `n` consecutive outputs can touch, with slack for the f32
// rounding of the source coordinate; in <= out
__host__ __device__ inline int low_span(int n, int in, int out) {
    const int s = (int)(((int64_t)(n - 1) * in) / out) + 4;
    return s < in ? s : in;
}

__host__ __device__ inline int64_t hist_cells(int K) { return ((int64_t)K * K + 1 + 1) / 2 * 2; }  // + #valid, even

// per-workgroup record in ws: NSUM f64 partials, then hist_cells(K) u32
__host__ __device__ inline int64_t record_bytes(int K) { return NSUM * 8 + hist_cells(K) * 4; }

struct Tiling {
    int tw, nrow, ncol, tiles_x, tiles_y, ntiles, nwg;
    size_t lds;
};
// the grid of 8 x t.tw tiles over B images of H x W, walked by at most NWG_MAX workgroups
inline void finish_tiling(Tiling& t, int B, int H, int W) {
    t.tiles_x = (W + t.tw - 1) / t.tw;
    t.tiles_y = (H + TH - 1) / TH;
    t.ntiles = B * t.tiles_y * t.tiles_x;  // < 2^31: B * H * W is
    t.nwg = t.ntiles < NWG_MAX ? t.ntiles : NWG_MAX;
}

struct TileOrigin {
    int b, y0, x0;
};
__device__ __forceinline__ TileOrigin tile_origin(int tile, const Tiling& tl) {
    TileOrigin o;
    o.b = tile / (tl.tiles_x * tl.tiles_y);
    o.y0 = ((tile / tl.tiles_x) % tl.tiles_y) * TH;
    o.x0 = (tile % tl.tiles_x) * tl.tw;
    return o;
}

// the tile's low-res patch -> LDS: rows [ilo, ilo + nr) x columns [jlo, jlo + nc) of every channel
template <typename TL>
__device__ __forceinline__ void stage_patch(float* __restrict__ low_s, const TL* __restrict__ low, int b, int K, int h,
                                            int w, int ilo, int nr, int jlo, int nc, int nrow, int ncol) {
    const int per = nr * nc;
    for (int e = threadIdx.x; e < K * per; e += blockDim.x) {
        const int k = e / per, r = (e % per) / nc, c = e % nc;
        low_s[(k * nrow + r) * ncol + c] = (float)low[(((int64_t)b * K + k) * h + ilo + r) * w + jlo + c];
    }
}

struct TileGeom {
    int b, y0, x0, ilo, nr, jlo, nc;
};
__device__ __forceinline__ TileGeom tile_geom(int tile, const Tiling& tl, int h, int w, int H, int W) {
    const TileOrigin o = tile_origin(tile, tl);
    TileGeom g;
    g.b = o.b;
    g.y0 = o.y0;
    g.x0 = o.x0;
    const int y1 = g.y0 + TH - 1 < H ? g.y0 + TH - 1 : H - 1;
    const int x1 = g.x0 + tl.tw - 1 < W ? g.x0 + tl.tw - 1 : W - 1;
    g.ilo = lerp_index(g.y0, h, H).i0;
    g.jlo = lerp_index(g.x0, w, W).i0;
    g.nr = lerp_index(y1, h, H).i1 - g.ilo + 1;
    g.nc = lerp_index(x1, w, W).i1 - g.jlo + 1;
    g.nr = g.nr < tl.nrow ? g.nr : tl.nrow;  // low_span() bounds both; never index LDS past the patch
    g.nc = g.nc < tl.ncol ? g.nc : tl.ncol;
    return g;
}

// One interpolated value, with every fused multiply-add spelled out: the definition of the resize's
// arithmetic, not left to the compiler's contraction, which does not fuse a thread's four pixels
// (slots) alike.  A flipped view must be the exact mirror of the plain one, and a pixel and its
// mirror sit in different slots, so the roundings are fixed.
//   bilerp:       one form for every slot (the segmentation kernels of the ensemble and the windows;
//                 eval_seg_kernel alone still leaves its interpolation to contraction).
//   bilerp_depth: the depth's form, for all four depth kernels: slot 0 fuses the outer sum on the
//                 bottom row, slot 1 the top row's sum on its right tap, everything else as bilerp.
//                 The slot is the source column % 4 (window-local under windows), flipped or not, so
//                 the mirror stays exact and one plain view is bitwise dclip_upsample_eval_depth
//                 (test_gpu_tta.py holds it).
__device__ __forceinline__ float bilerp(float yl0, float yl1, float xl0, float xl1, float a00, float a01, float a10,
                                        float a11) {
#pragma clang fp contract(off)
    const float top = fmaf(xl0, a00, xl1 * a01);
    const float bot = fmaf(xl0, a10, xl1 * a11);
    return fmaf(yl0, top, yl1 * bot);
}
__device__ __forceinline__ float bilerp_depth(int slot, float yl0, float yl1, float xl0, float xl1, float a00,
                                              float a01, float a10, float a11) {
#pragma clang fp contract(off)
    const float top = slot == 1 ? fmaf(xl1, a01, xl0 * a00) : fmaf(xl0, a00, xl1 * a01);
    const float bot = fmaf(xl0, a10, xl1 * a11);
    return slot == 0 ? fmaf(yl1, bot, yl0 * top) : fmaf(yl0, top, yl1 * bot);
}

// acc + u as one rounded add the compiler cannot fuse into the arithmetic that produced u: the
// views are summed as f32 values, in view order
__device__ __forceinline__ float add_rounded(float acc, float u) {
#pragma clang fp contract(off)
    return acc + u;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// sum / count as one correctly rounded division the compiler cannot turn into a multiplication by
// a reciprocal: a pixel covered once is exactly that window's resized value
__device__ __forceinline__ float div_rounded(float acc, float cnt) {
#pragma clang fp contract(off)
    return acc / cnt;
}

// The first pixel (raster order) of an H x W image (or view) that none of the wh x ww windows covers,
// by coordinate compression over the windows' edges: within a cell of the compressed grid every pixel
// has the same set of windows, so the cell's top-left pixel decides.  False when every pixel is covered.
inline bool first_uncovered(const dclip_window* wins, int nwin, int wh, int ww, int H, int W, int* py, int* px) {
    std::vector<int> ys{0}, xs{0};
    for (int i = 0; i < nwin; ++i) {
        ys.push_back(wins[i].y0);
        ys.push_back(wins[i].y0 + wh);
        xs.push_back(wins[i].x0);
        xs.push_back(wins[i].x0 + ww);
    }
    std::sort(ys.begin(), ys.end());
    ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
    std::sort(xs.begin(), xs.end());
    xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    for (int y : ys) {
        if (y >= H) break;
        for (int x : xs) {
            if (x >= W) break;
            bool hit = false;
            for (int i = 0; i < nwin && !hit; ++i)
                hit = y >= wins[i].y0 && y < wins[i].y0 + wh && x >= wins[i].x0 && x < wins[i].x0 + ww;
            if (!hit) {
                *py = y;
                *px = x;
                return true;
            }
        }
    }
    return false;
}

// 4 consecutive labels of one row; `vec`: the row segment is aligned for one vector load
__device__ __forceinline__ void load_labels4(const void* lab, int dt, int64_t pix, int n, bool vec, int* t) {
    if (vec) {
        if (dt == 0) {
            const longlong2 a = ((const longlong2*)((const int64_t*)lab + pix))[0];
            const longlong2 c = ((const longlong2*)((const int64_t*)lab + pix))[1];
            const long long v[4] = {a.x, a.y, c.x, c.y};
#pragma unroll
            for (int p = 0; p < 4; ++p) t[p] = (v[p] < 0 || v[p] > 0x7fffffff) ? -1 : (int)v[p];
        } else if (dt == 1) {
            const int4 a = *(const int4*)((const int32_t*)lab + pix);
            t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
        } else {
            const uint32_t a = *(const uint32_t*)((const uint8_t*)lab + pix);
#pragma unroll
            for (int p = 0; p < 4; ++p) t[p] = (int)((a >> (8 * p)) & 0xffu);
        }
        return;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        t[p] = -1;
        if (p < n) {
            if (dt == 0) {
                const int64_t v = ((const int64_t*)lab)[pix + p];
                t[p] = (v < 0 || v > 0x7fffffff) ? -1 : (int)v;
            } else if (dt == 1) {
                t[p] = ((const int32_t*)lab)[pix + p];
            } else {
                t[p] = ((const uint8_t*)lab)[pix + p];
            }
        }
    }
}

// the workgroup's f64 partials: wave butterflies (fixed), then the waves in order -> part[0..N)
template <int N>
__device__ __forceinline__ void wg_partials(double (&a)[N], double* __restrict__ red_s, double* __restrict__ part) {
    const int tid = threadIdx.x, nw = blockDim.x >> 6;
#pragma unroll
    for (int c = 0; c < N; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[c] += __shfl_xor(a[c], o, 64);
    if ((tid & 63) == 0)
#pragma unroll
        for (int c = 0; c < N; ++c) red_s[(tid >> 6) * N + c] = a[c];
    __syncthreads();
    if (tid < N) {
        double s = 0.0;
        for (int wv = 0; wv < nw; ++wv) s += red_s[wv * N + tid];
        part[tid] = s;
    }
}

// ----------------------------------------------------------------------------- segmentation epilogue
// the workgroup's LDS histogram (K x K confusion cells + #valid) starts at zero
template <int K>
__device__ __forceinline__ void hist_clear(unsigned* __restrict__ hist_s) {
    for (int e = threadIdx.x; e < K * K + 1; e += blockDim.x) hist_s[e] = 0u;
    __syncthreads();
}

// Scores PX consecutive pixels of one row from their K values v (already the mean its caller
// scores): am[p] = argmax, the lowest class index among equal maxima (torch.argmax).  LAB: with the
// labels t[p] (pixels p >= n lie outside the row), lsum += the CE terms in pixel order,
// -log softmax(v)[t], or -log v[t] when v holds mean probabilities (PROBS), and the (target,
// prediction) cells are counted in hist_s.
template <int K, int PX, bool LAB, bool PROBS>
__device__ __forceinline__ void seg_score(const float (&v)[PX][K], const int* t, int n, int ignore,
                                          unsigned* __restrict__ hist_s, double& lsum, int (&am)[PX]) {
    int cell_prev = -1;
    unsigned run = 0;
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        float m = v[p][0];
        int a = 0;
#pragma unroll
        for (int k = 1; k < K; ++k)
            if (v[p][k] > m) {
                m = v[p][k];
                a = k;
            }
        am[p] = a;
        if constexpr (LAB) {
            const int tp = t[p];
            const bool valid = p < n && tp != ignore && tp >= 0 && tp < K;
            if (valid) {
                float vt = 0.f, s = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    vt = k == tp ? v[p][k] : vt;
                    if constexpr (!PROBS) s += __expf(v[p][k] - m);
                }
                if constexpr (PROBS) lsum += (double)(-__logf(vt));
                else lsum += (double)(__logf(s) - (vt - m));  // as dclip_upsample_ce
            }
            // runs of equal (target, prediction) cells among the pixels: one LDS add each
            const int cell = valid ? tp * K + a : -1;
            if (cell != cell_prev) {
                if (cell_prev >= 0) atomicAdd(&hist_s[cell_prev], run);
                cell_prev = cell;
                run = 0;
            }
            ++run;
        }
    }
    if constexpr (LAB) {
        if (cell_prev >= 0) atomicAdd(&hist_s[cell_prev], run);
    }
}

// The chunked form of seg_score, for a class count too wide for one thread's registers: the classes
// arrive CK at a time, in ascending order, and SegRun carries what the scan needs between chunks:
// the running (max, argmax) and, with labels, the running sum of exp(v - max) and the target's value.
template <int PX>
struct SegRun {
    float m[PX], s[PX], vt[PX];
    int a[PX];
    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            m[p] = -INFINITY;
            s[p] = 0.f;
            vt[p] = 0.f;
            a[p] = 0;
        }
    }
};

// classes [k0, k0 + kc) of PX pixels, kc <= CK: a strict > keeps the lowest index among equal maxima,
// within a chunk and across chunks; the sum is rescaled whenever the maximum moves (exp(-inf) = 0
// covers the first chunk)
template <int CK, int PX, bool LAB>
__device__ __forceinline__ void seg_score_chunk(const float (&v)[PX][CK], int k0, int kc, const int* t,
                                                SegRun<PX>& r) {
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        float m = r.m[p];
        int a = r.a[p];
#pragma unroll
        for (int k = 0; k < CK; ++k)
            if (k < kc && v[p][k] > m) {
                m = v[p][k];
                a = k0 + k;
            }
        r.a[p] = a;
        if constexpr (LAB) {
            const int tk = t[p] - k0;
            float s = r.s[p] * __expf(r.m[p] - m), vt = r.vt[p];
#pragma unroll
            for (int k = 0; k < CK; ++k) {
                if (k < kc) s += __expf(v[p][k] - m);
                vt = k == tk ? v[p][k] : vt;
            }
            r.s[p] = s;
            r.vt[p] = vt;
        }
        r.m[p] = m;
    }
}

// after the last chunk: am[p], and with labels the CE terms in pixel order and the (target,
// prediction) cells, one integer add per run of equal cells, into `hist` (K x K u32; LDS or global:
// integer adds are exact in any order); nvalid += the pixels scored
template <int PX, bool LAB>
__device__ __forceinline__ void seg_score_finish(const SegRun<PX>& r, int K, const int* t, int n, int ignore,
                                                 unsigned* __restrict__ hist, double& lsum, unsigned& nvalid,
                                                 int (&am)[PX]) {
    int cell_prev = -1;
    unsigned run = 0;
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        am[p] = r.a[p];
        if constexpr (LAB) {
            const int tp = t[p];
            const bool valid = p < n && tp != ignore && tp >= 0 && tp < K;  // ignore first: it may lie below K
            if (valid) {
                lsum += (double)(__logf(r.s[p]) - (r.vt[p] - r.m[p]));
                ++nvalid;
            }
            const int cell = valid ? tp * K + r.a[p] : -1;
            if (cell != cell_prev) {
                if (cell_prev >= 0) atomicAdd(&hist[cell_prev], run);
                cell_prev = cell;
                run = 0;
            }
            ++run;
        }
    }
    if constexpr (LAB) {
        if (cell_prev >= 0) atomicAdd(&hist[cell_prev], run);
    }
}

// stage_patch for the classes [k0, k0 + kc) of a K-class map alone
template <typename TL>
__device__ __forceinline__ void stage_patch_chunk(float* __restrict__ low_s, const TL* __restrict__ low, int b, int K,
                                                  int k0, int kc, int h, int w, int ilo, int nr, int jlo, int nc,
                                                  int nrow, int ncol) {
    const int per = nr * nc;
    for (int e = threadIdx.x; e < kc * per; e += blockDim.x) {
        const int k = e / per, r = (e % per) / nc, c = e % nc;
        low_s[(k * nrow + r) * ncol + c] = (float)low[(((int64_t)b * K + k0 + k) * h + ilo + r) * w + jlo + c];
    }
}

// 4 class ids of one row; `vec`: the row segment is aligned for one dword
__device__ __forceinline__ void store_pred4(uint8_t* __restrict__ pred, int64_t pix, int n, bool vec,
                                            const int (&am)[4]) {
    if (pred == nullptr) return;
    if (vec) {
        *(uint32_t*)(pred + pix) =
            (uint32_t)am[0] | ((uint32_t)am[1] << 8) | ((uint32_t)am[2] << 16) | ((uint32_t)am[3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (p < n) pred[pix + p] = (uint8_t)am[p];
    }
}

// the workgroup's record: its CE partial, #valid and its histogram
template <int K>
__device__ __forceinline__ void seg_flush(const unsigned* __restrict__ hist_s, double lsum, double* __restrict__ red_s,
                                          char* __restrict__ ws) {
    char* rec = ws + (int64_t)blockIdx.x * record_bytes(K);
    double a[1] = {lsum};
    wg_partials<1>(a, red_s, (double*)rec);  // __syncthreads inside: every LDS add has landed after it
    unsigned* hist = (unsigned*)(rec + NSUM * 8);
    if (threadIdx.x == 0) {
        unsigned c = 0;
        for (int e = 0; e < K * K; ++e) c += hist_s[e];
        hist[K * K] = c;  // #valid
    }
    for (int e = threadIdx.x; e < K * K; e += blockDim.x) hist[e] = hist_s[e];
}

// ----------------------------------------------------------------------------- depth epilogue
// 4 resized depths of one row; `vec`: the row segment is aligned for one vector store
__device__ __forceinline__ void store_up4(float* __restrict__ up, int64_t pix, int n, bool vec, const float (&u)[4]) {
    if (up == nullptr) return;
    if (vec) {
        *(float4*)(up + pix) = make_float4(u[0], u[1], u[2], u[3]);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (p < n) up[pix + p] = u[p];
    }
}

// A thread's share of the 12 sums of dclip.h: sums[1..4], [9..11] in f64, in the order its pixels are
// scored; the counts [0], [5..8] as integers (exact), widened at the end.
struct DepthSums {
    double s_sq = 0.0, s_log = 0.0, s_abs = 0.0, s_sqrel = 0.0, s_msq = 0.0, s_d = 0.0, s_d2 = 0.0;
    unsigned n_eval = 0, n_a1 = 0, n_a2 = 0, n_a3 = 0, n_mask = 0;

    // 4 pixels of one row with the resized predictions u; `vec`: gt and mask are aligned for one
    // vector load each
    __device__ __forceinline__ void score4(const float (&u)[4], const float* __restrict__ gt,
                                           const uint8_t* __restrict__ mask, int64_t pix, int n, bool vec, float dmin,
                                           float dmax, int clamp_pred, float eps) {
        float tg[4] = {0.f, 0.f, 0.f, 0.f};
        bool tm[4];
        if (vec) {
            const float4 a = *(const float4*)(gt + pix);
            tg[0] = a.x; tg[1] = a.y; tg[2] = a.z; tg[3] = a.w;
            const uint32_t mk = mask ? *(const uint32_t*)(mask + pix) : 0x01010101u;
#pragma unroll
            for (int p = 0; p < 4; ++p) tm[p] = ((mk >> (8 * p)) & 0xffu) != 0;
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                tm[p] = false;
                if (p < n) {
                    tg[p] = gt[pix + p];
                    tm[p] = mask == nullptr || mask[pix + p] != 0;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (!tm[p]) continue;
            const float gtv = tg[p];
            // the trainer's masked RMSE (unclamped) and the SILog pass-0 sums, d as dclip_upsample_silog
            ++n_mask;
            const float dm = gtv - u[p];
            s_msq += (double)(dm * dm);
            // selects, not fmaxf (which returns eps for a NaN): a NaN depth or target reaches sum d, sum d^2
            const float d = logf(u[p] < eps ? eps : u[p]) - logf(gtv < eps ? eps : gtv);
            s_d += (double)d;
            s_d2 += (double)d * (double)d;
            // compute_depth_errors: mask && min <= gt <= max, optionally clamped prediction
            if (!(gtv >= dmin && gtv <= dmax)) continue;
            const float pr = clamp_pred ? fminf(fmaxf(u[p], dmin), dmax) : u[p];
            ++n_eval;
            const float thr = fmaxf(gtv / pr, pr / gtv);
            n_a1 += thr < 1.25f ? 1u : 0u;
            n_a2 += thr < 1.5625f ? 1u : 0u;
            n_a3 += thr < 1.953125f ? 1u : 0u;
            const float df = gtv - pr;
            const float dl = logf(gtv) - logf(pr);
            s_sq += (double)(df * df);
            s_log += (double)(dl * dl);
            s_abs += (double)(fabsf(df) / gtv);
            s_sqrel += (double)(df * df / gtv);
        }
    }

    // the workgroup's record: its 12 partials
    __device__ __forceinline__ void flush(double* __restrict__ red_s, char* __restrict__ ws) const {
        double a[NSUM] = {(double)n_eval, s_sq,          s_log,          s_abs, s_sqrel, (double)n_a1,
                          (double)n_a2,   (double)n_a3, (double)n_mask, s_msq, s_d,     s_d2};
        wg_partials<NSUM>(a, red_s, (double*)(ws + (int64_t)blockIdx.x * record_bytes(1)));
    }
};

// cm / count / loss_sum += the workgroups' records, in workgroup order
__global__ __launch_bounds__(256) void eval_seg_fold_kernel(const char* __restrict__ ws, int nwg, int K,
                                                            int64_t* __restrict__ cm, double* __restrict__ loss_sum,
                                                            unsigned long long* __restrict__ count) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const int64_t rb = record_bytes(K);
    for (int c = t; c < K * K + 1; c += 256) {
        unsigned long long s = 0;
        for (int e = 0; e < nwg; ++e) s += ((const unsigned*)(ws + e * rb + NSUM * 8))[c];
        if (c < K * K) cm[c] += (int64_t)s;
        else count[0] += s;
    }
    double s = 0.0;
    for (int e = t; e < nwg; e += 256) s += ((const double*)(ws + e * rb))[0];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) loss_sum[0] += red[0];
}

// sums[c] += the workgroups' partials, in workgroup order within each thread's stripe, then a fixed
// LDS tree (the counts are integers below 2^53: exact)
__global__ __launch_bounds__(256) void eval_depth_fold_kernel(const char* __restrict__ ws, int nwg,
                                                              double* __restrict__ sums) {
    __shared__ double red[NSUM][256];
    const int t = threadIdx.x;
    const int64_t rb = record_bytes(1);
    double s[NSUM];
#pragma unroll
    for (int c = 0; c < NSUM; ++c) s[c] = 0.0;
    for (int e = t; e < nwg; e += 256)
#pragma unroll
        for (int c = 0; c < NSUM; ++c) s[c] += ((const double*)(ws + e * rb))[c];
#pragma unroll
    for (int c = 0; c < NSUM; ++c) red[c][t] = s[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o)
#pragma unroll
            for (int c = 0; c < NSUM; ++c) red[c][t] += red[c][t + o];
        __syncthreads();
    }
    if (t < NSUM) sums[t] += red[t][0];
}

// ----------------------------------------------------------------------------- host side
// whether the 4-pixel row segments of an image of width W are aligned for one vector access
inline int labels_aligned(const void* lab, int lab_dt, int W) {
    const int lab_align = lab_dt == 0 ? 16 : lab_dt == 1 ? 16 : 4;
    return lab != nullptr && W % 4 == 0 && (uintptr_t)lab % lab_align == 0;
}
inline int pred_aligned(const uint8_t* pred, int W) {
    return pred != nullptr && W % 4 == 0 && (uintptr_t)pred % 4 == 0;
}
inline int depth_aligned(const float* gt, const uint8_t* mask, const float* up, int W) {
    return W % 4 == 0 && (gt == nullptr || (uintptr_t)gt % 16 == 0) && (mask == nullptr || (uintptr_t)mask % 4 == 0) &&
           (up == nullptr || (uintptr_t)up % 16 == 0);
}

// the outputs of a segmentation entry point `name`: with labels, or the class map alone
inline int check_seg_outputs(const char* name, const void* labels, int lab_dt, const uint8_t* pred, const int64_t* cm,
                             const double* loss_sum, const unsigned long long* count) {
    if (labels != nullptr) {
        DCLIP_HOST_CHECK(lab_dt >= 0 && lab_dt <= 2, "%s: lab_dt=%d: labels int64 (0), int32 (1) or uint8 (2)", name,
                         lab_dt);
        DCLIP_HOST_CHECK(cm && loss_sum && count, "%s: cm, loss_sum and count required with labels", name);
    } else {
        DCLIP_HOST_CHECK(!cm && !loss_sum && !count, "%s: cm, loss_sum and count must be null without labels", name);
        DCLIP_HOST_CHECK(pred != nullptr, "%s: nothing to do (no labels, no pred)", name);
    }
    return 0;
}
// the outputs of a depth entry point `name` whose target is optional: without one (prediction only)
// mask and sums are not touched
inline int check_depth_outputs(const char* name, const float* target, const double* sums, const float* up) {
    if (target != nullptr) DCLIP_HOST_CHECK(sums != nullptr, "%s: sums required with a target", name);
    else DCLIP_HOST_CHECK(up != nullptr, "%s: nothing to do (no target, no up)", name);
    return 0;
}

// runs the statement with TL = the element type of the low-res maps (low_dt checked by the caller)
#define EVAL_DISPATCH_LOW(low_dt, ...)      \
    do {                                    \
        if ((low_dt) == DCLIP_F32) {        \
            using TL = float;               \
            __VA_ARGS__;                    \
        } else if ((low_dt) == DCLIP_BF16) { \
            using TL = bf16;                \
            __VA_ARGS__;                    \
        } else {                            \
            using TL = f16;                 \
            __VA_ARGS__;                    \
        }                                   \
    } while (0)

}  // namespace
