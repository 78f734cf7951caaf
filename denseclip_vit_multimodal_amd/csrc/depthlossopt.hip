// The fused upsample + depth loss (+ gradient) with the terms the reference's trainer chooses between
// (configs/denseclip_multitask_cityscapes.yaml:67-70 "Choose 'silog', 'berhu', or 'l1'",
// train_denseclip.py:1276-1312 "the sum of depth components"): any weighted sum of SILog, L1 and BerHu
// on the resized prediction, which exists only in registers.  headloss.hip's SILog pair stays where it is,
// untouched; these kernels keep its band geometry at K = 1 (one low-res row x 32 low-res columns per
// workgroup, 32 x 8 threads, band_range and the thread-to-pixel map of ce_band.h), its per-pixel
// arithmetic for p = up(X) and d, and its fixed summation orders.
//
// On the mask M (a non-zero byte; every pixel without a mask), r = p - gt, e = |r|, T = #M, T' = max(T, 1):
//     silog = sum d^2 / T' - lambd (sum d)^2 / T'^2       d = log(max(p, eps)) - log(max(gt, eps))
//     l1    = sum e / T'
//     berhu = sum b(e) / T'    b(e) = e if e <= c, else (e^2 + c^2) / (2 c);   c = theta max_M e
// c is a constant of the call (Laina et al.): no gradient flows through the maximum.  So any
// combination of terms takes at most two passes over the pixels:
//     stats   (PASS 0)  sum d, sum d^2, T, sum e, max e: only the selected terms' sums.  Each workgroup
//                       writes one record of partials; depth_stats_fold_kernel adds them in workgroup
//                       order and takes the maximum (exact in any order).
//     finish  (PASS 1, 2) reads the complete stats, takes c from them, writes sum b(e) and, in PASS 2, the
//                       weighted gradient w_s silog' + w_1 sign(r) / T' + w_b (sign(r) / T' if e <= c else
//                       r / (c T')) folded through the transposed interpolation into per-workgroup tiles
//                       (classes.hip's layout), which ce_band.h's merge launch adds in its fixed order.
//                       PASS 1 is the forward-only form: no tiles, no merge.
// No float atomics: two runs are bitwise equal.  NaN follows dclip.h's rule for SILog: the clamps and the
// maximum are selects that keep a NaN (fmaxf would drop it), so one NaN among the in-mask resized
// predictions or targets makes sum e, max e and sum b NaN, while T counts the pixel all the same.
// sign(0) = 0 and e <= c takes the linear branch, so c = 0 (every e zero, or no pixel) never divides.
//
// Registers (gfx950, -O3; VGPRs, no AGPRs, no scratch anywhere; waves per SIMD in brackets), the same for
// f32, bf16 and f16 predictions:
//     depth_band_kernel PASS 0 (stats)             33 (8)
//     depth_band_kernel PASS 1 (finish, forward)   30 (8)
//     depth_band_kernel PASS 2 (finish, gradient)  51 (7)
//     depth_stats_fold_kernel 24 (8), depth_bsum_fold_kernel 8 (8), ce_classes_merge_kernel 24 (8)
// The Makefile reads the compiler's resource remarks for this file and fails the build if any kernel here
// uses scratch or falls below 2 waves per SIMD.
#include "ce_band.h"

namespace {

constexpr int NREC = 6;  // doubles per workgroup record: sum d, sum d^2, T, sum e, max e, sum b(e)
constexpr int T_SILOG = DCLIP_DEPTH_SILOG, T_L1 = DCLIP_DEPTH_L1, T_BERHU = DCLIP_DEPTH_BERHU;

// the larger of two values, a NaN in either kept (fmaxf returns the other operand)
__device__ __forceinline__ float max_keep_nan(float m, float e) { return (e > m || e != e) ? e : m; }
__device__ __forceinline__ double max_keep_nan(double m, double e) { return (e > m || e != e) ? e : m; }

struct DepthArgs {
    float eps, lambd;
    int terms;               // PASS 0: the sums to build; PASS 1, 2: the terms with a non-zero weight
    float w_s, w_1, w_b;     // PASS 1, 2
    float theta;             // PASS 1, 2
};

// part: [nwg][NREC] f64 (PASS 0 writes 0..4, PASS 1 / 2 write 5 when BerHu is on);
// tiles: [B][h][2][band_cols] f32 (PASS 2)
template <typename TL, int PASS>
__global__ __launch_bounds__(NTH) void depth_band_kernel(const TL* __restrict__ low, int h, int w, int H, int W,
                                                         int chunks, const float* __restrict__ gt,
                                                         const uint8_t* __restrict__ mask, DepthArgs a,
                                                         const double* __restrict__ stats,
                                                         double* __restrict__ part, float* __restrict__ tiles) {
    static_assert(NTH == JW * 8, "32 low-res columns x 8 column slices");
    __shared__ float low_s[2][JW + 1];  // the band's two low-res rows over the chunk (+1 column)
    __shared__ float g_s[4][JW];        // per low-res column: left-upper, right-upper, left-lower, right-lower
    __shared__ double red_s[NTH / 64][5];
    const int tid = threadIdx.x;
    const int wg = blockIdx.x;
    const int ch = wg % chunks;
    const int i = (wg / chunks) % h;
    const int b = wg / (chunks * h);
    const int jc = ch * JW;
    const int i1 = i + (i < h - 1 ? 1 : 0);
    const int ncol = (jc + JW + 1 <= w ? JW + 1 : w - jc);
    for (int e = tid; e < 2 * (JW + 1); e += NTH) {
        const int r = e / (JW + 1), jx = e % (JW + 1);
        low_s[r][jx] = jx < ncol ? (float)low[((int64_t)b * h + (r ? i1 : i)) * w + jc + jx] : 0.f;
    }
    __syncthreads();
    const bool silog = (a.terms & T_SILOG) != 0, l1 = (a.terms & T_L1) != 0, berhu = (a.terms & T_BERHU) != 0;
    // the finish passes take the call's constants from the complete stats
    float gS = 0.f, gT = 1.f, c = 0.f, k1 = 0.f, kb = 0.f, kc = 0.f;
    if constexpr (PASS != 0) {
        gS = (float)stats[0];
        gT = (float)stats[2];
        gT = gT > 0.f ? gT : 1.f;
        c = berhu ? a.theta * (float)stats[4] : 0.f;
        k1 = a.w_1 / gT;
        kb = a.w_b / gT;
        kc = c > 0.f ? a.w_b / (c * gT) : 0.f;  // c = 0: no pixel lies above it; c NaN: the select below keeps it
        kc = c != c ? c : kc;
    }
    const int jj = tid >> 3, xs = tid & 7;
    const int j0 = jc + jj;
    int ylo, yhi;
    band_range(i, h, H, &ylo, &yhi);
    double lsum = 0.0, lsum2 = 0.0, lsume = 0.0, lsumb = 0.0;
    float lmax = 0.f;
    unsigned lcnt = 0;
    float g[4] = {0.f, 0.f, 0.f, 0.f};  // folded gradient: left-upper, right-upper, left-lower, right-lower
    if (j0 < w) {
        int xlo, xhi;
        band_range(j0, w, W, &xlo, &xhi);
        for (int x = xlo + xs; x <= xhi; x += 8) {
            const Lerp X = lerp_index(x, w, W);
            if (X.i0 != j0) continue;
            const int j1 = X.i1 - jc;
            const float ut = X.l0 * low_s[0][jj] + X.l1 * low_s[0][j1];
            const float ub = X.l0 * low_s[1][jj] + X.l1 * low_s[1][j1];
            float at = 0.f, ab = 0.f;
            // the column's targets 8 rows at a time, all loads in flight together
            for (int y0 = ylo; y0 <= yhi; y0 += 8) {
                float tg[8];
                bool tm[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int y = y0 + u;
                    const int64_t pix = ((int64_t)b * H + (y <= yhi ? y : yhi)) * W + x;
                    tm[u] = y <= yhi && (mask == nullptr || mask[pix] != 0);
                    tg[u] = gt[pix];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int y = y0 + u;
                    if (y > yhi) continue;
                    const Lerp Y = lerp_index(y, h, H);
                    if (Y.i0 != i) continue;
                    if (!tm[u]) continue;
                    const float p = Y.l0 * ut + Y.l1 * ub;
                    const float r = p - tg[u];
                    const float e = fabsf(r);
                    float d = 0.f;
                    // selects, not fmaxf: a NaN depth or target must reach the sums (headloss.hip)
                    if (PASS != 1 && silog) d = logf(p < a.eps ? a.eps : p) - logf(tg[u] < a.eps ? a.eps : tg[u]);
                    if constexpr (PASS == 0) {
                        ++lcnt;
                        if (silog) {
                            lsum += (double)d;
                            lsum2 += (double)d * (double)d;
                        }
                        if (l1 || berhu) lsume += (double)e;
                        if (berhu) lmax = max_keep_nan(lmax, e);
                    } else {
                        const bool lin = e <= c;  // false for a NaN on either side: the NaN goes on
                        if (berhu) lsumb += (double)(lin ? e : (e * e + c * c) / (2.f * c));
                        if constexpr (PASS == 2) {
                            const float sg = r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f);
                            float gd = 0.f;
                            if (silog)
                                gd = a.w_s * ((2.f * d / gT - 2.f * a.lambd * gS / (gT * gT)) *
                                              (p >= a.eps ? 1.f / p : 0.f));
                            if (l1) gd += sg * k1;
                            if (berhu) gd += lin ? sg * kb : r * kc;
                            at += Y.l0 * gd;
                            ab += Y.l1 * gd;
                        }
                    }
                }
            }
            if constexpr (PASS == 2) {
                if (j1 == jj) {  // clamped right edge: both weights on one column
                    g[0] += at;
                    g[2] += ab;
                } else {
                    g[0] += X.l0 * at;
                    g[1] += X.l1 * at;
                    g[2] += X.l0 * ab;
                    g[3] += X.l1 * ab;
                }
            }
        }
    }
    if constexpr (PASS == 2) {
        // the column's 8 slices (8 adjacent lanes): a xor butterfly, the same order on every run
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v = g[q];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            if (xs == 0) g_s[q][jj] = v;
        }
    }
    // the workgroup's record: wave sums (fixed butterfly), then the 4 waves in order
    if (PASS == 0 || berhu) {
        double s0 = PASS == 0 ? lsum : lsumb, s1 = lsum2, s2 = (double)lcnt, s3 = lsume;
        float m = lmax;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s0 += __shfl_xor(s0, o, 64);
            if constexpr (PASS == 0) {
                s1 += __shfl_xor(s1, o, 64);
                s2 += __shfl_xor(s2, o, 64);
                s3 += __shfl_xor(s3, o, 64);
                m = max_keep_nan(m, __shfl_xor(m, o, 64));
            }
        }
        if ((tid & 63) == 0) {
            red_s[tid >> 6][0] = s0;
            if constexpr (PASS == 0) {
                red_s[tid >> 6][1] = s1;
                red_s[tid >> 6][2] = s2;
                red_s[tid >> 6][3] = s3;
                red_s[tid >> 6][4] = (double)m;
            }
        }
    }
    __syncthreads();  // also publishes g_s
    if constexpr (PASS == 0) {
        if (tid < 5) {
            double s = 0.0;
            for (int wv = 0; wv < NTH / 64; ++wv) s = tid == 4 ? max_keep_nan(s, red_s[wv][4]) : s + red_s[wv][tid];
            part[(int64_t)wg * NREC + tid] = s;
        }
    } else {
        if (berhu && tid == 0) {
            double s = 0.0;
            for (int wv = 0; wv < NTH / 64; ++wv) s += red_s[wv][0];
            part[(int64_t)wg * NREC + 5] = s;
        }
    }
    if constexpr (PASS == 2) {  // the chunk's gradient tile (rows i, i1 x the chunk's ncol columns)
        const int64_t bc = band_cols(w, chunks);
        float* trow = tiles + (((int64_t)b * h + i) * 2) * bc + (int64_t)ch * (JW + 1);
        for (int e = tid; e < 2 * ncol; e += NTH) {
            const int r = e / ncol, jx = e % ncol;
            float v = 0.f;
            if (!(r == 1 && i1 == i)) {
                // low-res column jx: its own left weights, then column jx - 1's right weights
                v = (jx < JW ? g_s[2 * r][jx] : 0.f) + (jx > 0 ? g_s[2 * r + 1][jx - 1] : 0.f);
                if (r == 0 && i1 == i)  // last band: the lower row is the upper row
                    v += (jx < JW ? g_s[2][jx] : 0.f) + (jx > 0 ? g_s[3][jx - 1] : 0.f);
            }
            trow[(int64_t)r * bc + jx] = v;
        }
    }
}

// stats[0..3] += the records' sums and stats[4] = max(stats[4], the records' maxima), the selected slots
// only: in workgroup order within each thread's stripe, then a fixed LDS tree.  The maximum is exact in
// any order and keeps a NaN from either side.
__global__ __launch_bounds__(256) void depth_stats_fold_kernel(const double* __restrict__ part, int nwg, int terms,
                                                               double* __restrict__ stats) {
    __shared__ double red[5][256];
    const int t = threadIdx.x;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = t; e < nwg; e += 256) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += part[(int64_t)e * NREC + q];
        s[4] = max_keep_nan(s[4], part[(int64_t)e * NREC + 4]);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) red[q][t] = s[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][t] += red[q][t + o];
            red[4][t] = max_keep_nan(red[4][t], red[4][t + o]);
        }
        __syncthreads();
    }
    if (t == 0) {
        if (terms & T_SILOG) {
            stats[0] += red[0][0];
            stats[1] += red[1][0];
        }
        stats[2] += red[2][0];
        if (terms & (T_L1 | T_BERHU)) stats[3] += red[3][0];
        if (terms & T_BERHU) stats[4] = max_keep_nan(stats[4], red[4][0]);
    }
}

// berhu_sum[0] += the records' sum b(e), in the same order
__global__ __launch_bounds__(256) void depth_bsum_fold_kernel(const double* __restrict__ part, int nwg,
                                                              double* __restrict__ berhu_sum) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int e = t; e < nwg; e += 256) s += part[(int64_t)e * NREC + 5];
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) berhu_sum[0] += red[0];
}

int64_t ws_floats(int B, int h, int w) {
    const int chunks = (w + JW - 1) / JW;
    const int64_t nwg = (int64_t)B * h * chunks;
    // the f64 records first (8-byte aligned), then the tiles
    return nwg * 2 * NREC + (int64_t)B * h * 2 * band_cols(w, chunks);
}

template <typename TL, int PASS>
void launch(const void* low, int B, int h, int w, int H, int W, const float* gt, const uint8_t* mask,
            const DepthArgs& a, double* stats, double* berhu_sum, float* grad, float* ws, hipStream_t st) {
    const int chunks = (w + JW - 1) / JW;
    const int nwg = B * h * chunks;
    double* part = (double*)ws;
    float* tiles = ws + (int64_t)nwg * 2 * NREC;
    depth_band_kernel<TL, PASS><<<nwg, NTH, 0, st>>>((const TL*)low, h, w, H, W, chunks, gt, mask, a, stats, part,
                                                     tiles);
    if constexpr (PASS == 0) {
        depth_stats_fold_kernel<<<1, 256, 0, st>>>(part, nwg, a.terms, stats);
    } else {
        if (berhu_sum != nullptr) depth_bsum_fold_kernel<<<1, 256, 0, st>>>(part, nwg, berhu_sum);
    }
    if constexpr (PASS == 2) {
        const int64_t total = (int64_t)B * h * w;
        int64_t blocks = (total + 255) / 256;
        blocks = blocks > 4096 ? 4096 : blocks;
        ce_classes_merge_kernel<<<(unsigned)blocks, 256, 0, st>>>(tiles, B, 1, h, w, chunks, grad);
    }
}

// the checks both entry points share; 0 when the geometry and the buffers are usable
int check_common(const char* fn, int low_dt, const void* pred, int B, int h, int w, const float* target, int H,
                 int W, float eps, const float* ws) {
    DCLIP_HOST_CHECK(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "%s: bad sizes", fn);
    DCLIP_HOST_CHECK(low_dt == DCLIP_F32 || low_dt == DCLIP_F16 || low_dt == DCLIP_BF16,
                     "%s: low_dt=%d (f32, f16 or bf16)", fn, low_dt);
    DCLIP_HOST_CHECK((int64_t)B * H * W < ((int64_t)1 << 31), "%s: B*H*W = %lld pixels (must be below 2^31)", fn,
                     (long long)((int64_t)B * H * W));
    DCLIP_HOST_CHECK((int64_t)B * h * ((w + JW - 1) / JW) < ((int64_t)1 << 31), "%s: too many low-res bands", fn);
    DCLIP_HOST_CHECK(eps == eps, "%s: eps is NaN", fn);
    DCLIP_HOST_CHECK(pred && target, "%s: missing buffers: pred and target required", fn);
    DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                     "%s: ws (dclip_upsample_depth_loss_ws_floats(B, h, w) f32, 8-byte aligned) required", fn);
    return 0;
}

bool weight_ok(float v) { return v >= 0.f && v <= 3.0e38f; }  // finite and not negative (NaN fails both)

}  // namespace

extern "C" int64_t dclip_upsample_depth_loss_ws_floats(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return 0;
    return ws_floats(B, h, w);
}

extern "C" int dclip_upsample_depth_stats(int low_dt, const void* pred, int B, int h, int w, const float* target,
                                          const uint8_t* mask, int H, int W, float eps, int terms, double* stats,
                                          float* ws, void* stream) {
    if (int rc = check_common("dclip_upsample_depth_stats", low_dt, pred, B, h, w, target, H, W, eps, ws)) return rc;
    DCLIP_HOST_CHECK(terms > 0 && terms <= (T_SILOG | T_L1 | T_BERHU),
                     "dclip_upsample_depth_stats: terms=%d (a non-empty set of SILog 1, L1 2, BerHu 4)", terms);
    DCLIP_HOST_CHECK(stats != nullptr, "dclip_upsample_depth_stats: missing buffers: stats (f64[6]) required");
    const DepthArgs a{eps, 0.f, terms, 0.f, 0.f, 0.f, 0.f};
    hipStream_t st = (hipStream_t)stream;
    EVAL_DISPATCH_LOW(low_dt, (launch<TL, 0>(pred, B, h, w, H, W, target, mask, a, stats, nullptr, nullptr, ws, st)));
    DCLIP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dclip_upsample_depth_finish(int low_dt, const void* pred, int B, int h, int w, const float* target,
                                           const uint8_t* mask, int H, int W, float eps, float lambd, int terms,
                                           float w_silog, float w_l1, float w_berhu, float threshold,
                                           const double* stats, double* berhu_sum, float* grad, float* ws,
                                           void* stream) {
    if (int rc = check_common("dclip_upsample_depth_finish", low_dt, pred, B, h, w, target, H, W, eps, ws)) return rc;
    DCLIP_HOST_CHECK(terms > 0 && terms <= (T_SILOG | T_L1 | T_BERHU),
                     "dclip_upsample_depth_finish: terms=%d (the set stats was built for: SILog 1, L1 2, BerHu 4)",
                     terms);
    DCLIP_HOST_CHECK(weight_ok(w_silog) && weight_ok(w_l1) && weight_ok(w_berhu),
                     "dclip_upsample_depth_finish: weights (%g, %g, %g) must be finite and >= 0", (double)w_silog,
                     (double)w_l1, (double)w_berhu);
    DCLIP_HOST_CHECK(w_silog > 0.f || w_l1 > 0.f || w_berhu > 0.f,
                     "dclip_upsample_depth_finish: every weight is zero (at least one term needed)");
    DCLIP_HOST_CHECK((w_silog == 0.f || (terms & T_SILOG)) && (w_l1 == 0.f || (terms & T_L1)) &&
                         (w_berhu == 0.f || (terms & T_BERHU)),
                     "dclip_upsample_depth_finish: a weight is non-zero for a term stats was not built for (terms=%d)",
                     terms);
    DCLIP_HOST_CHECK(lambd == lambd, "dclip_upsample_depth_finish: lambd is NaN");
    DCLIP_HOST_CHECK(w_berhu == 0.f || (threshold > 0.f && threshold <= 1.f),
                     "dclip_upsample_depth_finish: threshold=%g (0 < threshold <= 1)", (double)threshold);
    DCLIP_HOST_CHECK(stats != nullptr, "dclip_upsample_depth_finish: missing buffers: stats (f64[6]) required");
    DCLIP_HOST_CHECK((w_berhu > 0.f) == (berhu_sum != nullptr),
                     "dclip_upsample_depth_finish: berhu_sum (f64[1]) goes with a non-zero BerHu weight, and only "
                     "with one");
    DCLIP_HOST_CHECK(grad != nullptr || berhu_sum != nullptr,
                     "dclip_upsample_depth_finish: missing buffers: nothing to write (grad or berhu_sum required)");
    const int on = (w_silog > 0.f ? T_SILOG : 0) | (w_l1 > 0.f ? T_L1 : 0) | (w_berhu > 0.f ? T_BERHU : 0);
    const DepthArgs a{eps, lambd, on, w_silog, w_l1, w_berhu, threshold};
    hipStream_t st = (hipStream_t)stream;
    if (grad != nullptr)
        EVAL_DISPATCH_LOW(low_dt,
                          (launch<TL, 2>(pred, B, h, w, H, W, target, mask, a, (double*)stats, berhu_sum, grad, ws, st)));
    else
        EVAL_DISPATCH_LOW(low_dt, (launch<TL, 1>(pred, B, h, w, H, W, target, mask, a, (double*)stats, berhu_sum,
                                                 nullptr, ws, st)));
    DCLIP_LAUNCH_CHECK();
    return 0;
}
