// What the chunked fused CE (classes.hip) and its optioned form (celossopt.hip) share: the band geometry,
// the label load, the per-chunk staging of the band's two low-res rows, the layout of the gradient tiles in
// the workspace and the launch that merges them.  One definition, so that a change to the banding or to the
// merge order reaches both kernels.  (headloss.hip's 19-class kernel keeps its own tile layout and merge.)
#pragma once
#include "eval_tile.h"

namespace {

constexpr int CK = 16;    // classes per chunk
constexpr int JW = 32;    // low-res columns per workgroup chunk
constexpr int NTH = 256;  // 32 low-res columns x 8 column slices
constexpr int YB = 8;     // rows of one column a thread carries through the class chunks

// conservative output range [lo, hi] whose i0 may equal i (headloss.hip's)
__device__ __forceinline__ void band_range(int i, int in, int out, int* lo, int* hi) {
    const float inv = (float)out / (float)in;
    int a = (int)floorf(((float)i + 0.5f) * inv - 0.5f) - 2;
    int b = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 2;
    *lo = (a < 0 || i == 0) ? 0 : a;
    *hi = (b > out - 1 || i == in - 1) ? out - 1 : b;
}

// a label as an int; what no int holds is no class
__device__ __forceinline__ int load_label(const void* lab, int dt, int64_t i) {
    if (dt == 0) {
        const int64_t v = ((const int64_t*)lab)[i];
        return (v < 0 || v > 0x7fffffff) ? -1 : (int)v;
    }
    if (dt == 1) return ((const int32_t*)lab)[i];
    return ((const uint8_t*)lab)[i];
}

// the gradient tiles of one band: [2 rows][w + chunks - 1 columns][K]; chunk c owns the columns
// [33 c, 33 c + min(33, w - 32 c)): its 32 low-res columns and, unless it is the last, the first of
// the next chunk
__host__ __device__ inline int64_t band_cols(int w, int chunks) { return (int64_t)w + chunks - 1; }

// the band's two low-res rows over the chunk's columns, classes [k0, k0 + CK): zeros past K or w
template <typename TL>
__device__ __forceinline__ void stage_band(float (&low_s)[2][CK][JW + 1], const TL* __restrict__ low, int b, int K,
                                           int k0, int h, int w, int i, int i1, int jc, int ncol) {
    for (int e = threadIdx.x; e < 2 * CK * (JW + 1); e += NTH) {
        const int r = e / (CK * (JW + 1)), k = (e / (JW + 1)) % CK, jx = e % (JW + 1);
        const int kk = k0 + k;
        low_s[r][k][jx] =
            (jx < ncol && kk < K) ? (float)low[(((int64_t)b * K + kk) * h + (r ? i1 : i)) * w + jc + jx] : 0.f;
    }
}

// grad[b][k][y][x] += the <= 4 tiles covering it, in a fixed order: band y / chunk x / 32 (upper
// row), chunk x / 32 - 1's 33rd column, band y - 1 (lower row), band y - 1's previous chunk
__global__ __launch_bounds__(256) void ce_classes_merge_kernel(const float* __restrict__ tiles, int B, int K, int h,
                                                               int w, int chunks, float* __restrict__ grad) {
    const int64_t total = (int64_t)B * K * h * w;
    const int64_t bc = band_cols(w, chunks);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(idx % w);
        const int y = (int)((idx / w) % h);
        const int k = (int)((idx / ((int64_t)w * h)) % K);
        const int b = (int)(idx / ((int64_t)w * h * K));
        const int c0 = x / JW, jx = x % JW;
        auto at = [&](int band, int c, int r, int j) {
            return tiles[((((int64_t)b * h + band) * 2 + r) * bc + (int64_t)c * (JW + 1) + j) * K + k];
        };
        float v = at(y, c0, 0, jx);
        if (jx == 0 && c0 > 0) v += at(y, c0 - 1, 0, JW);
        if (y > 0) {
            v += at(y - 1, c0, 1, jx);
            if (jx == 0 && c0 > 0) v += at(y - 1, c0 - 1, 1, JW);
        }
        grad[idx] += v;
    }
}

}  // namespace
