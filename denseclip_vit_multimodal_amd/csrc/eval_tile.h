// The tile machinery shared by the fused head evaluation kernels (headeval.hip: one low-res map per
// output pixel; headensemble.hip: V of them; headslide.hip: the windows that cover it;
// headslidetta.hip: the windows of V views): the resize's
// source index, the low-res patch of an 8 x TW output tile and its LDS staging, the interpolation
// with its fused multiply-adds spelled out (the ensemble's and the sliding windows'), the windows'
// rounded division and host-side coverage check, the 4-pixel
// label load, the per-workgroup record in the caller's workspace and the one-workgroup folds.
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
__device__ __forceinline__ TileGeom tile_geom(int tile, int tiles_x, int tiles_y, int tw, int h, int w, int H, int W,
                                              int nrow, int ncol) {
    TileGeom g;
    g.b = tile / (tiles_x * tiles_y);
    g.y0 = ((tile / tiles_x) % tiles_y) * TH;
    g.x0 = (tile % tiles_x) * tw;
    const int y1 = g.y0 + TH - 1 < H ? g.y0 + TH - 1 : H - 1;
    const int x1 = g.x0 + tw - 1 < W ? g.x0 + tw - 1 : W - 1;
    g.ilo = lerp_index(g.y0, h, H).i0;
    g.jlo = lerp_index(g.x0, w, W).i0;
    g.nr = lerp_index(y1, h, H).i1 - g.ilo + 1;
    g.nc = lerp_index(x1, w, W).i1 - g.jlo + 1;
    g.nr = g.nr < nrow ? g.nr : nrow;  // low_span() bounds both; never index LDS past the patch
    g.nc = g.nc < ncol ? g.nc : ncol;
    return g;
}

// One interpolated value, with every fused multiply-add spelled out.  headeval.hip leaves
// Y.l0 * (X.l0 * a00 + X.l1 * a01) + Y.l1 * (...) to the compiler's contraction, and the compiler
// does not fuse a thread's four pixels (slots) alike.  Here a flipped view must be the exact mirror
// of the plain one, and a pixel and its mirror sit in different slots, so the roundings are fixed.
//   bilerp:       the form of most of headeval's slots, for every slot (the segmentation kernel).
//   bilerp_depth: the forms eval_depth_kernel compiles to on gfx950, per slot, read from its
//                 assembly: slot 0 fuses the outer sum on the bottom row, slot 1 the top row's sum
//                 on its right tap, everything else as bilerp.  With these, one plain view is
//                 bitwise dclip_upsample_eval_depth (test_gpu_tta.py pins it; a compiler that fuses
//                 headeval.hip otherwise shows up there).  The depth kernel keeps a source column
//                 in the slot column % 4, flipped or not, so the mirror stays exact.
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

}  // namespace
