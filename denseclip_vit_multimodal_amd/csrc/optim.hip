// Multi-tensor AdamW step with global-norm clipping, gradient-accumulation scaling and a device-
// resident learning rate (dclip.h: dclip_adamw_*; train.FusedAdamW).
//
// Two passes over HBM instead of torch's fused AdamW + clip_grad_norm_'s norm and multiply passes
// + the inf-norm check + weight_refresh_kernel:
//   norm pass    one workgroup per tile reads its gradients once (4 B / parameter) and writes ONE
//                fp64 partial: per element the exact fp64 square of the fp32 value, summed per
//                thread in element order, then a fixed wave butterfly, then the waves in order.
//   fold         one workgroup adds the partials in a fixed order (thread t takes partials t,
//                t + 256, ..; the 256 thread sums are added in thread order) and writes the step's
//                scalars into the optimizer's state buffer: nothing races, no workgroup elects itself.
//   update pass  one workgroup per tile reads p, g, m, v once, writes p, m, v and the 16-bit plain
//                and transposed (through LDS) copies the next forward / backward read
//                (28 B / parameter of fp32 traffic + 2 B per copy element).
// No atomics of any kind, so every result is bitwise reproducible.
//
// Tiles (as misc.hip's weight_refresh_kernel): a parameter WITH a transposed copy is viewed as
// (rows, cols) = (shape[0], numel / shape[0]) and cut into 64 x 64 tiles; every other parameter
// (column tiles = 0 in the descriptor) is walked as flat chunks of 4096 elements.
// The gradient addresses change every eager step (autograd hands over fresh tensors), so they
// are NOT in the device descriptor: they travel as kernel arguments, ADAMW_CHUNK entries per
// launch — copied by value at launch time, no host buffer that a later step could overwrite
// while an earlier launch still reads it, and nothing to synchronise.
#include "common.h"

namespace {

constexpr int ADAMW_CHUNK = DCLIP_ADAMW_CHUNK;     // descriptor entries per launch
constexpr int DW = DCLIP_ADAMW_DESC_WORDS;         // int64 per descriptor entry
constexpr int SH = DCLIP_ADAMW_STATE_HEAD;         // floats before the rows in the state
constexpr int SR = DCLIP_ADAMW_STATE_ROW_FLOATS;   // floats per state row
constexpr int HR = DCLIP_ADAMW_HP_FLOATS;          // floats per hyper-parameter row
constexpr int FLAT = 4096;                         // elements per flat chunk

struct GradArgs {
    const float* g[ADAMW_CHUNK];
};

// the entry in [0, n) whose tile range holds `blk` (d[7] = first tile, ascending)
__device__ __forceinline__ int find_entry(const int64_t* __restrict__ desc, int n, int64_t blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(int64_t)mid * DW + 7] <= blk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Where the 4 consecutive elements of a lane's i-th access (i in [0, 4)) start, and how many of
// them exist: flat chunks (tcn == 0) or a 64 x 64 tile of a (rows, cols) matrix.
struct Tile {
    int64_t rows, cols, rb, cb, base;  // base: first element of a flat chunk
    bool flat;
    __device__ __forceinline__ Tile(const int64_t* __restrict__ d, int64_t blk) {
        rows = d[5];
        cols = d[6];
        const int64_t local = blk - d[7], tcn = d[8];
        flat = tcn == 0;
        rb = flat ? 0 : (local / tcn) * 64;
        cb = flat ? 0 : (local % tcn) * 64;
        base = flat ? local * FLAT : 0;
    }
    // element offset of access i and the count (0..4) of valid elements from it
    __device__ __forceinline__ int64_t at(int i, int& cnt) const {
        const int t = threadIdx.x;
        if (flat) {
            const int64_t o = base + 4 * t + 1024 * i, numel = rows * cols;
            cnt = o >= numel ? 0 : (int)(numel - o < 4 ? numel - o : 4);
            return o;
        }
        const int64_t row = rb + (t >> 4) + 16 * i, col = cb + 4 * (t & 15);
        cnt = (row >= rows || col >= cols) ? 0 : (int)(cols - col < 4 ? cols - col : 4);
        return row * cols + col;
    }
    // whether 4-element accesses are 16-byte aligned for 16-byte aligned bases
    __device__ __forceinline__ bool vec_ok() const { return flat || (cols & 3) == 0; }
};

__device__ __forceinline__ f32x4 load4(const float* __restrict__ p, int64_t o, int cnt, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec && cnt == 4) return *(const f32x4*)(p + o);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < cnt) v[e] = p[o + e];
    return v;
}

__device__ __forceinline__ void store4(float* __restrict__ p, int64_t o, int cnt, bool vec, f32x4 v) {
    if (vec && cnt == 4) {
        *(f32x4*)(p + o) = v;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < cnt) p[o + e] = v[e];
}

template <typename TO>
__device__ __forceinline__ void store4_lp(TO* __restrict__ p, int64_t o, int cnt, bool vec, f32x4 v) {
    if (vec && cnt == 4) {
        typedef TO to4 __attribute__((ext_vector_type(4)));
        const to4 q = {(TO)v[0], (TO)v[1], (TO)v[2], (TO)v[3]};
        *(to4*)(p + o) = q;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < cnt) p[o + e] = (TO)v[e];
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// ----------------------------------------------------------------------------- norm pass
// part[blk] = sum of g^2 over the tile (0 for an entry without a gradient)
__global__ __launch_bounds__(256) void adamw_norm_kernel(const int64_t* __restrict__ desc, int e0, int ne,
                                                         int64_t tile0, GradArgs ga, double* __restrict__ part) {
    __shared__ double red[4];
    const int64_t blk = tile0 + blockIdx.x;
    const int le = find_entry(desc + (int64_t)e0 * DW, ne, blk);
    const float* __restrict__ g = ga.g[le];
    double s = 0.0;
    if (g != nullptr) {  // block-uniform
        const Tile tl(desc + (int64_t)(e0 + le) * DW, blk);
        const bool vec = tl.vec_ok() && aligned16(g, nullptr, nullptr, nullptr);
        f32x4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // the four loads in flight before any is used
            int cnt;
            const int64_t o = tl.at(i, cnt);
            v[i] = load4(g, o, cnt, vec);  // absent elements read as 0
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) s += (double)v[i][e] * (double)v[i][e];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ----------------------------------------------------------------------------- fold
// state (f32): [0] total_norm  [1] clip coefficient  [2] found_inf  [3] step count (steps applied; written
// by the update)  [4] the count of the prepared step  [5..8) unused,
// then per hyper-parameter row r at SH + SR * r:
//   [0] lr  [1] lr * wd  [2] lr / (1 - b1^t)  [3] 1 / sqrt(1 - b2^t)  [4] 1 - b1  [5] b2  [6] 1 - b2
//   [7] eps  [8] c = coef * inv_accum
__global__ __launch_bounds__(256) void adamw_fold_kernel(const double* __restrict__ part, int64_t tiles,
                                                         const float* __restrict__ hp, int n_rows,
                                                         const float* __restrict__ ext, float* __restrict__ state) {
    __shared__ double red[256];
    __shared__ double sh_coef, sh_t;
    const int t = threadIdx.x;
    double s = 0.0;
    if (part != nullptr)
        for (int64_t e = t; e < tiles; e += 256) s += part[e];
    red[t] = s;
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int i = 0; i < 256; ++i) sum += red[i];
        const double max_norm = (double)hp[5], inv_accum = (double)hp[6];
        const bool bad = !(fabs(sum) <= 1.79769313486231570e308) || (ext != nullptr && *ext != 0.f);
        const double norm = sqrt(sum) * inv_accum;
        const double coef = max_norm > 0.0 ? fmin(1.0, max_norm / (norm + 1e-6)) : 1.0;
        double step = (double)state[3];
        if (!bad) step += 1.0;
        state[0] = (float)norm;
        state[1] = (float)coef;
        state[2] = bad ? 1.f : 0.f;
        state[4] = (float)step;  // the count this step will have once applied: the update commits it to [3]
        sh_coef = coef;
        sh_t = step;
    }
    __syncthreads();
    for (int r = t; r < n_rows; r += 256) {
        const float* h = hp + (int64_t)r * HR;
        float* o = state + SH + (int64_t)r * SR;
        // the table holds 1 - beta: 1 - 0.999 keeps its digits in fp32, 0.999 would lose those of 1 - beta2
        const double lr = (double)h[0], b1 = 1.0 - (double)h[1], b2 = 1.0 - (double)h[2], wd = (double)h[4];
        const double tt = sh_t < 1.0 ? 1.0 : sh_t;  // a skipped first step: the rows are not used
        o[0] = h[0];
        o[1] = (float)(lr * wd);
        o[2] = (float)(lr / (1.0 - pow(b1, tt)));
        o[3] = (float)(1.0 / sqrt(1.0 - pow(b2, tt)));
        o[4] = h[1];
        o[5] = (float)b2;
        o[6] = h[2];
        o[7] = h[3];
        o[8] = (float)(sh_coef * (double)h[6]);
    }
}

// ----------------------------------------------------------------------------- update pass
// fp32 per element, torch's AdamW order (the gradient is never rewritten):
//   g' = g c;  p = p - (lr wd) p  [= p (1 - lr wd), one rounding];  m = m + (1 - b1)(g' - m);
//   v = b2 v + (1 - b2) g'^2;  p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
struct Row {
    float lr_wd, step, isbc2, omb1, b2, omb2, eps, c;
};

__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const Row& h) {
    const float gp = g * h.c;
    p = fmaf(-h.lr_wd, p, p);
    m = m + h.omb1 * (gp - m);
    v = h.b2 * v + h.omb2 * (gp * gp);
    const float denom = sqrtf(v) * h.isbc2 + h.eps;
    p = p - h.step * (m / denom);
}

__global__ __launch_bounds__(256) void adamw_update_kernel(const int64_t* __restrict__ desc, int e0, int ne,
                                                           int64_t tile0, GradArgs ga,
                                                           float* __restrict__ state) {
    __shared__ float tile[64][65];
    if (state[2] != 0.f) return;  // found_inf: the step is skipped, nothing is written
    const int64_t blk = tile0 + blockIdx.x;
    // the step counts once it is applied: tile 0's workgroup commits the prepared count (no other
    // workgroup reads [3]; preparing twice, or preparing without updating, counts nothing)
    if (blk == 0 && threadIdx.x == 0) state[3] = state[4];
    const int le = find_entry(desc + (int64_t)e0 * DW, ne, blk);
    const float* __restrict__ g = ga.g[le];
    if (g == nullptr) return;  // block-uniform: no gradient this step
    const int64_t* d = desc + (int64_t)(e0 + le) * DW;
    float* __restrict__ p = (float*)d[0];
    float* __restrict__ m = (float*)d[1];
    float* __restrict__ v = (float*)d[2];
    void* dp = (void*)d[3];
    void* dt = (void*)d[4];
    const int cdt = (int)d[10];
    const float* st = state + SH + d[9] * SR;
    const Row h = {st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8]};
    const Tile tl(d, blk);
    const bool vec = tl.vec_ok() && aligned16(p, g, m, v);
    f32x4 vp[4], vg[4], vm[4], vv[4];
    int64_t off[4];
    int cnt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // 16 16-byte loads in flight per lane
        off[i] = tl.at(i, cnt[i]);
        vp[i] = load4(p, off[i], cnt[i], vec);
        vg[i] = load4(g, off[i], cnt[i], vec);
        vm[i] = load4(m, off[i], cnt[i], vec);
        vv[i] = load4(v, off[i], cnt[i], vec);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = vp[i][e], me = vm[i][e], ve = vv[i][e];
            adamw1(pe, vg[i][e], me, ve, h);
            vp[i][e] = pe;
            vm[i][e] = me;
            vv[i][e] = ve;
        }
        store4(p, off[i], cnt[i], vec, vp[i]);
        store4(m, off[i], cnt[i], vec, vm[i]);
        store4(v, off[i], cnt[i], vec, vv[i]);
        if (dp != nullptr) {  // the plain copy has the parameter's own layout (8-byte stores)
            if (cdt == DCLIP_BF16) store4_lp((bf16*)dp, off[i], cnt[i], vec, vp[i]);
            else store4_lp((f16*)dp, off[i], cnt[i], vec, vp[i]);
        }
    }
    if (dt == nullptr || tl.flat) return;  // block-uniform
    const int t = threadIdx.x, c4 = t & 15, r = t >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[r + 16 * i][4 * c4 + e] = vp[i][e];
    __syncthreads();
    // transposed copy (cols, rows): row c of it = column c of the tile, 8 source rows per lane
    const int j = t & 7, oc = t >> 3;
    const int64_t rows = tl.rows, cols = tl.cols;
    const bool tvec = (rows & 7) == 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = oc + 32 * i;
        const int64_t gc = tl.cb + c, gr = tl.rb + 8 * j;
        if (gc >= cols || gr >= rows) continue;
        if (cdt == DCLIP_BF16) {
            bf16* o = (bf16*)dt + gc * rows + gr;
            if (tvec && gr + 8 <= rows) {
                bf16x8 q;
#pragma unroll
                for (int e = 0; e < 8; ++e) q[e] = (bf16)tile[8 * j + e][c];
                *(bf16x8*)o = q;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (gr + e < rows) o[e] = (bf16)tile[8 * j + e][c];
            }
        } else {
            f16* o = (f16*)dt + gc * rows + gr;
            if (tvec && gr + 8 <= rows) {
                f16x8 q;
#pragma unroll
                for (int e = 0; e < 8; ++e) q[e] = (f16)tile[8 * j + e][c];
                *(f16x8*)o = q;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (gr + e < rows) o[e] = (f16)tile[8 * j + e][c];
            }
        }
    }
}

// the arguments both entry points share; the host descriptor is read here, never by a kernel
int check_common(const char* who, const int64_t* desc, const int64_t* desc_host, const void* const* grads, int n,
                 int64_t tiles) {
    DCLIP_HOST_CHECK(desc != nullptr && desc_host != nullptr && grads != nullptr, "%s: null descriptor", who);
    DCLIP_HOST_CHECK(n > 0 && tiles > 0, "%s: empty descriptor (n=%d, tiles=%lld)", who, n, (long long)tiles);
    DCLIP_HOST_CHECK(tiles < (1ll << 31), "%s: tiles=%lld must be below 2^31", who, (long long)tiles);
    int64_t next = 0;
    for (int e = 0; e < n; ++e) {
        const int64_t* d = desc_host + (int64_t)e * DW;
        DCLIP_HOST_CHECK(d[0] != 0 && d[1] != 0 && d[2] != 0, "%s: entry %d has a null p, m or v", who, e);
        DCLIP_HOST_CHECK(d[5] > 0 && d[6] > 0 && d[8] >= 0, "%s: entry %d has an empty shape", who, e);
        DCLIP_HOST_CHECK((d[3] == 0 && d[4] == 0) || d[10] == DCLIP_BF16 || d[10] == DCLIP_F16,
                         "%s: entry %d: copy dtype %lld (16-bit copies only: bf16 or fp16)", who, e, (long long)d[10]);
        DCLIP_HOST_CHECK(d[4] == 0 || d[8] != 0, "%s: entry %d has a transposed copy but no 64 x 64 tiling", who, e);
        DCLIP_HOST_CHECK(d[8] == 0 || d[8] == (d[6] + 63) / 64,
                         "%s: entry %d has %lld column tiles, its %lld columns need %lld (or 0: flat chunks)", who, e,
                         (long long)d[8], (long long)d[6], (long long)((d[6] + 63) / 64));
        DCLIP_HOST_CHECK(d[7] == next, "%s: entry %d starts at tile %lld, expected %lld", who, e, (long long)d[7],
                         (long long)next);
        next += d[8] == 0 ? (d[5] * d[6] + FLAT - 1) / FLAT : ((d[5] + 63) / 64) * d[8];
        DCLIP_HOST_CHECK(d[9] >= 0, "%s: entry %d names hyper-parameter row %lld", who, e, (long long)d[9]);
    }
    DCLIP_HOST_CHECK(next == tiles, "%s: the descriptor covers %lld tiles, tiles=%lld", who, (long long)next,
                     (long long)tiles);
    return DCLIP_OK;
}

// one launch per ADAMW_CHUNK entries: launch(e0, ne, tile0, ntile, args)
template <typename F>
void for_chunks(const int64_t* desc_host, const void* const* grads, int n, int64_t tiles, F&& launch) {
    for (int e0 = 0; e0 < n; e0 += ADAMW_CHUNK) {
        const int ne = n - e0 < ADAMW_CHUNK ? n - e0 : ADAMW_CHUNK;
        GradArgs ga;
        for (int i = 0; i < ADAMW_CHUNK; ++i) ga.g[i] = i < ne ? (const float*)grads[e0 + i] : nullptr;
        const int64_t t0 = desc_host[(int64_t)e0 * DW + 7];
        const int64_t t1 = e0 + ne < n ? desc_host[(int64_t)(e0 + ne) * DW + 7] : tiles;
        if (t1 > t0) launch(e0, ne, t0, (unsigned)(t1 - t0), ga);
    }
}

}  // namespace

extern "C" int64_t dclip_adamw_ws_bytes(int64_t tiles) { return tiles > 0 ? tiles * (int64_t)sizeof(double) : 0; }

extern "C" int dclip_adamw_prepare(const int64_t* desc, const int64_t* desc_host, const void* const* grads, int n,
                                   int64_t tiles, const float* hp, int n_rows, const float* found_inf, float* state,
                                   void* ws, int with_norm, void* stream) {
    if (int rc = check_common("dclip_adamw_prepare", desc, desc_host, grads, n, tiles)) return rc;
    DCLIP_HOST_CHECK(hp != nullptr && n_rows > 0, "dclip_adamw_prepare: null or empty hyper-parameter table");
    for (int e = 0; e < n; ++e)
        DCLIP_HOST_CHECK(desc_host[(int64_t)e * DW + 9] < n_rows, "dclip_adamw_prepare: entry %d names row %lld of %d",
                         e, (long long)desc_host[(int64_t)e * DW + 9], n_rows);
    DCLIP_HOST_CHECK(state != nullptr, "dclip_adamw_prepare: null state");
    DCLIP_HOST_CHECK(!with_norm || ws != nullptr, "dclip_adamw_prepare: null ws (dclip_adamw_ws_bytes)");
    hipStream_t st = (hipStream_t)stream;
    if (with_norm)
        for_chunks(desc_host, grads, n, tiles, [&](int e0, int ne, int64_t t0, unsigned nt, const GradArgs& ga) {
            adamw_norm_kernel<<<nt, 256, 0, st>>>(desc, e0, ne, t0, ga, (double*)ws);
        });
    adamw_fold_kernel<<<1, 256, 0, st>>>(with_norm ? (const double*)ws : nullptr, tiles, hp, n_rows, found_inf, state);
    DCLIP_LAUNCH_CHECK();
    return DCLIP_OK;
}

extern "C" int dclip_adamw_update(const int64_t* desc, const int64_t* desc_host, const void* const* grads, int n,
                                  int64_t tiles, float* state, void* stream) {
    if (int rc = check_common("dclip_adamw_update", desc, desc_host, grads, n, tiles)) return rc;
    DCLIP_HOST_CHECK(state != nullptr, "dclip_adamw_update: null state");
    hipStream_t st = (hipStream_t)stream;
    for_chunks(desc_host, grads, n, tiles, [&](int e0, int ne, int64_t t0, unsigned nt, const GradArgs& ga) {
        adamw_update_kernel<<<nt, 256, 0, st>>>(desc, e0, ne, t0, ga, state);
    });
    DCLIP_LAUNCH_CHECK();
    return DCLIP_OK;
}
