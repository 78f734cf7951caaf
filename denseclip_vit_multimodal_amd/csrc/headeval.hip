// Fused bilinear upsample + evaluation of the two DenseCLIP heads (forward only).
//
// The reference's validate() (train_denseclip.py:294-684) resizes the segmentation logits and the
// depth prediction to the label size (F.interpolate bilinear, align_corners=False, :461-467), then
// takes argmax -> confusion matrix / pixel accuracy (denseclip/utils.py:109-139), the validation CE
// (:497), the depth errors (utils/depth_metrics.py:12-88), the masked RMSE (:589-593) and the SILog
// sums (:524): at 1024x2048 a 19-channel fp32 tensor of 1.27 GB per 8 images written by the resize
// and read back by argmax and by the loss.  Here, as in headloss.hip, the upsampled values exist
// only in registers; HBM traffic is the labels / targets, the u8 class map and the low-res maps.
//
// Work split: the output is cut into tiles of 8 rows x TW columns (TW = 128, or 64 where the
// low-res patch of a 128-wide tile would not fit in LDS).  A workgroup of 8 x TW/4 threads stages
// the low-res rows / columns its tile interpolates from in LDS (f32, [K][rows][cols]) and every
// thread evaluates 4 consecutive pixels of one row: labels, targets and masks are loaded, and class
// ids and resized depths stored, as one 4-pixel vector per thread (a dword of four u8 class ids),
// coalesced along x.  A grid of at most NWG_MAX workgroups walks the tiles with a grid stride, so
// the per-workgroup state below is flushed once per workgroup, not once per tile.
//
// Reductions (no float atomics, no global atomics at all):
//   * integer counts (confusion matrix, #valid): an LDS-private histogram per workgroup (LDS integer
//     adds: exact in any order), written as the workgroup's tile of u32 to the caller's workspace;
//   * floating sums: f32 per-pixel terms, f64 accumulators per thread in loop order, a fixed xor
//     butterfly per wave, the waves in order, one f64 partial per workgroup in the workspace;
//   * eval_fold_kernel (one workgroup) adds the workgroups' tiles and partials in workgroup order
//     into the caller's running cm / loss_sum / count / sums.  The grid is a function of the shapes
//     alone, so two runs are bitwise equal.
#include "eval_tile.h"

namespace {

Tiling make_tiling(int B, int K, int h, int w, int H, int W) {
    Tiling t;
    t.nrow = low_span(TH, h, H);
    t.tw = 128;
    t.ncol = low_span(t.tw, w, W);
    if ((int64_t)K * t.nrow * t.ncol * 4 > LDS_TILE_MAX) {
        t.tw = 64;
        t.ncol = low_span(t.tw, w, W);
    }
    t.lds = (size_t)K * t.nrow * t.ncol * 4;
    t.tiles_x = (W + t.tw - 1) / t.tw;
    t.tiles_y = (H + TH - 1) / TH;
    t.ntiles = B * t.tiles_y * t.tiles_x;  // < 2^31: B * H * W is
    t.nwg = t.ntiles < NWG_MAX ? t.ntiles : NWG_MAX;
    return t;
}

// ----------------------------------------------------------------------------- segmentation
// LAB: labels given (confusion matrix, CE sum, #valid); pred may be null then.  !LAB: pred only.
template <typename TL, int K, bool LAB>
__global__ __launch_bounds__(256) void eval_seg_kernel(const TL* __restrict__ low, int h, int w, int H, int W,
                                                       Tiling tl, const void* __restrict__ lab, int lab_dt,
                                                       int ignore, int vec_lab, int vec_pred,
                                                       uint8_t* __restrict__ pred, char* __restrict__ ws) {
    extern __shared__ float low_s[];
    __shared__ unsigned hist_s[K * K + 1];
    __shared__ double red_s[4];
    const int tid = threadIdx.x;
    const int xs = tl.tw >> 2;  // threads along x
    const int tx = tid % xs, ty = tid / xs;
    if constexpr (LAB) {
        for (int e = tid; e < K * K + 1; e += blockDim.x) hist_s[e] = 0u;
    }
    double lsum = 0.0;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const TileGeom g = tile_geom(tile, tl.tiles_x, tl.tiles_y, tl.tw, h, w, H, W, tl.nrow, tl.ncol);
        __syncthreads();  // the previous tile's readers are done (and hist_s is cleared)
        stage_patch(low_s, low, g.b, K, h, w, g.ilo, g.nr, g.jlo, g.nc, tl.nrow, tl.ncol);
        __syncthreads();
        const int y = g.y0 + ty, x = g.x0 + 4 * tx;
        if (y >= H || x >= W) continue;
        const int n = W - x < 4 ? W - x : 4;
        const int64_t pix = ((int64_t)g.b * H + y) * W + x;
        int t[4] = {-1, -1, -1, -1};
        if constexpr (LAB) load_labels4(lab, lab_dt, pix, n, vec_lab != 0, t);
        const Lerp Y = lerp_index(y, h, H);
        int r0 = Y.i0 - g.ilo, r1 = Y.i1 - g.ilo;
        r0 = r0 < g.nr ? r0 : g.nr - 1;
        r1 = r1 < g.nr ? r1 : g.nr - 1;
        Lerp X[4];
        int c0[4], c1[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            X[p] = lerp_index(x + p < W ? x + p : W - 1, w, W);
            c0[p] = X[p].i0 - g.jlo;
            c1[p] = X[p].i1 - g.jlo;
            c0[p] = c0[p] < g.nc ? c0[p] : g.nc - 1;
            c1[p] = c1[p] < g.nc ? c1[p] : g.nc - 1;
        }
        // the four pixels usually share their two low-res columns (always at the workload's x16)
        const bool same = c0[0] == c0[3] && c1[0] == c1[3];
        float v[4][K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float* top = low_s + (k * tl.nrow + r0) * tl.ncol;
            const float* bot = low_s + (k * tl.nrow + r1) * tl.ncol;
            if (same) {
                const float a00 = top[c0[0]], a01 = top[c1[0]], a10 = bot[c0[0]], a11 = bot[c1[0]];
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    v[p][k] = Y.l0 * (X[p].l0 * a00 + X[p].l1 * a01) + Y.l1 * (X[p].l0 * a10 + X[p].l1 * a11);
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    v[p][k] = Y.l0 * (X[p].l0 * top[c0[p]] + X[p].l1 * top[c1[p]]) +
                              Y.l1 * (X[p].l0 * bot[c0[p]] + X[p].l1 * bot[c1[p]]);
            }
        }
        int am[4];
        int cell_prev = -1;
        unsigned run = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            // argmax: the lowest class index among equal maxima (torch.argmax)
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
                        s += __expf(v[p][k] - m);
                    }
                    lsum += (double)(__logf(s) - (vt - m));  // -log softmax[t], as dclip_upsample_ce
                }
                // runs of equal (target, prediction) cells among the four pixels: one LDS add each
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
        if (pred != nullptr) {
            if (vec_pred) {
                *(uint32_t*)(pred + pix) = (uint32_t)am[0] | ((uint32_t)am[1] << 8) | ((uint32_t)am[2] << 16) |
                                           ((uint32_t)am[3] << 24);
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (p < n) pred[pix + p] = (uint8_t)am[p];
            }
        }
    }
    if constexpr (LAB) {
        char* rec = ws + (int64_t)blockIdx.x * record_bytes(K);
        double a[1] = {lsum};
        wg_partials<1>(a, red_s, (double*)rec);  // __syncthreads inside: every LDS add has landed after it
        unsigned* hist = (unsigned*)(rec + NSUM * 8);
        if (tid == 0) {
            unsigned c = 0;
            for (int e = 0; e < K * K; ++e) c += hist_s[e];
            hist[K * K] = c;  // #valid
        }
        for (int e = tid; e < K * K; e += blockDim.x) hist[e] = hist_s[e];
    }
}


// ----------------------------------------------------------------------------- depth
template <typename TL>
__global__ __launch_bounds__(256) void eval_depth_kernel(const TL* __restrict__ low, int h, int w, int H, int W,
                                                         Tiling tl, const float* __restrict__ gt,
                                                         const uint8_t* __restrict__ mask, float dmin, float dmax,
                                                         int clamp_pred, float eps, int vec, float* __restrict__ up,
                                                         char* __restrict__ ws) {
    extern __shared__ float low_s[];
    __shared__ double red_s[4 * NSUM];
    const int tid = threadIdx.x;
    const int xs = tl.tw >> 2;
    const int tx = tid % xs, ty = tid / xs;
    // sums[1..4], [9..11] in f64; the counts [0], [5..8] as integers (exact), widened at the end
    double s_sq = 0.0, s_log = 0.0, s_abs = 0.0, s_sqrel = 0.0, s_msq = 0.0, s_d = 0.0, s_d2 = 0.0;
    unsigned n_eval = 0, n_a1 = 0, n_a2 = 0, n_a3 = 0, n_mask = 0;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const TileGeom g = tile_geom(tile, tl.tiles_x, tl.tiles_y, tl.tw, h, w, H, W, tl.nrow, tl.ncol);
        __syncthreads();
        stage_patch(low_s, low, g.b, 1, h, w, g.ilo, g.nr, g.jlo, g.nc, tl.nrow, tl.ncol);
        __syncthreads();
        const int y = g.y0 + ty, x = g.x0 + 4 * tx;
        if (y >= H || x >= W) continue;
        const int n = W - x < 4 ? W - x : 4;
        const int64_t pix = ((int64_t)g.b * H + y) * W + x;
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
        const Lerp Y = lerp_index(y, h, H);
        int r0 = Y.i0 - g.ilo, r1 = Y.i1 - g.ilo;
        r0 = r0 < g.nr ? r0 : g.nr - 1;
        r1 = r1 < g.nr ? r1 : g.nr - 1;
        const float* top = low_s + r0 * tl.ncol;
        const float* bot = low_s + r1 * tl.ncol;
        float u[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const Lerp X = lerp_index(x + p < W ? x + p : W - 1, w, W);
            int c0 = X.i0 - g.jlo, c1 = X.i1 - g.jlo;
            c0 = c0 < g.nc ? c0 : g.nc - 1;
            c1 = c1 < g.nc ? c1 : g.nc - 1;
            u[p] = Y.l0 * (X.l0 * top[c0] + X.l1 * top[c1]) + Y.l1 * (X.l0 * bot[c0] + X.l1 * bot[c1]);
        }
        if (up != nullptr) {
            if (vec) {
                *(float4*)(up + pix) = make_float4(u[0], u[1], u[2], u[3]);
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (p < n) up[pix + p] = u[p];
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
            const float d = logf(fmaxf(u[p], eps)) - logf(fmaxf(gtv, eps));
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
    double a[NSUM] = {(double)n_eval, s_sq,          s_log,          s_abs, s_sqrel, (double)n_a1,
                      (double)n_a2,   (double)n_a3, (double)n_mask, s_msq, s_d,     s_d2};
    wg_partials<NSUM>(a, red_s, (double*)(ws + (int64_t)blockIdx.x * record_bytes(1)));
}


template <typename TL>
void launch_seg(const void* low, int B, int h, int w, int H, int W, const void* lab, int lab_dt, int ignore,
                uint8_t* pred, int64_t* cm, double* loss_sum, unsigned long long* count, void* ws, hipStream_t st) {
    constexpr int K = 19;
    const Tiling tl = make_tiling(B, K, h, w, H, W);
    const int nth = (tl.tw / 4) * TH;
    const int lab_align = lab_dt == 0 ? 16 : lab_dt == 1 ? 16 : 4;
    const int vec_lab = lab != nullptr && W % 4 == 0 && (uintptr_t)lab % lab_align == 0;
    const int vec_pred = pred != nullptr && W % 4 == 0 && (uintptr_t)pred % 4 == 0;
    if (lab != nullptr) {
        eval_seg_kernel<TL, K, true><<<tl.nwg, nth, tl.lds, st>>>((const TL*)low, h, w, H, W, tl, lab, lab_dt, ignore,
                                                                  vec_lab, vec_pred, pred, (char*)ws);
        eval_seg_fold_kernel<<<1, 256, 0, st>>>((const char*)ws, tl.nwg, K, cm, loss_sum, count);
    } else {
        eval_seg_kernel<TL, K, false><<<tl.nwg, nth, tl.lds, st>>>((const TL*)low, h, w, H, W, tl, nullptr, 0, ignore,
                                                                   0, vec_pred, pred, (char*)ws);
    }
}

template <typename TL>
void launch_depth(const void* low, int B, int h, int w, int H, int W, const float* gt, const uint8_t* mask,
                  float dmin, float dmax, int clamp_pred, float eps, float* up, double* sums, void* ws,
                  hipStream_t st) {
    const Tiling tl = make_tiling(B, 1, h, w, H, W);
    const int nth = (tl.tw / 4) * TH;
    const int vec = W % 4 == 0 && (uintptr_t)gt % 16 == 0 && (mask == nullptr || (uintptr_t)mask % 4 == 0) &&
                    (up == nullptr || (uintptr_t)up % 16 == 0);
    eval_depth_kernel<TL><<<tl.nwg, nth, tl.lds, st>>>((const TL*)low, h, w, H, W, tl, gt, mask, dmin, dmax,
                                                       clamp_pred, eps, vec, up, (char*)ws);
    eval_depth_fold_kernel<<<1, 256, 0, st>>>((const char*)ws, tl.nwg, sums);
}

}  // namespace

extern "C" int64_t dclip_upsample_eval_ws_bytes(int B, int K, int h, int w) {
    if (B <= 0 || K <= 0 || h <= 0 || w <= 0) return 0;
    return (int64_t)NWG_MAX * record_bytes(K);
}

#define EVAL_SIZE_CHECKS(NAME)                                                                                   \
    DCLIP_HOST_CHECK(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, NAME ": bad sizes");                             \
    DCLIP_HOST_CHECK(low_dt == DCLIP_F32 || low_dt == DCLIP_F16 || low_dt == DCLIP_BF16,                         \
                     NAME ": low_dt=%d (f32, f16 or bf16)", low_dt);                                             \
    DCLIP_HOST_CHECK(H >= h && W >= w, NAME ": the output (%d x %d) must not be smaller than the input (%d x %d)", \
                     H, W, h, w);                                                                                \
    DCLIP_HOST_CHECK((int64_t)B * H * W < ((int64_t)1 << 31), NAME ": B*H*W = %lld pixels (must be below 2^31)",  \
                     (long long)((int64_t)B * H * W))

extern "C" int dclip_upsample_eval_seg(int low_dt, const void* logits, int B, int K, int h, int w,
                                       const void* labels, int lab_dt, int H, int W, int ignore_index, uint8_t* pred,
                                       int64_t* cm, double* loss_sum, unsigned long long* count, void* ws,
                                       void* stream) {
    DCLIP_HOST_CHECK(K == 19, "dclip_upsample_eval_seg: K=%d (built for the 19 Cityscapes classes)", K);
    EVAL_SIZE_CHECKS("dclip_upsample_eval_seg");
    DCLIP_HOST_CHECK(logits != nullptr, "dclip_upsample_eval_seg: logits required");
    if (labels != nullptr) {
        DCLIP_HOST_CHECK(lab_dt >= 0 && lab_dt <= 2,
                         "dclip_upsample_eval_seg: lab_dt=%d: labels int64 (0), int32 (1) or uint8 (2)", lab_dt);
        DCLIP_HOST_CHECK(cm && loss_sum && count, "dclip_upsample_eval_seg: cm, loss_sum and count required with labels");
        DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                         "dclip_upsample_eval_seg: ws (dclip_upsample_eval_ws_bytes(B, K, h, w) bytes, 8-byte aligned) "
                         "required");
    } else {
        DCLIP_HOST_CHECK(!cm && !loss_sum && !count,
                         "dclip_upsample_eval_seg: cm, loss_sum and count must be null without labels");
        DCLIP_HOST_CHECK(pred != nullptr, "dclip_upsample_eval_seg: nothing to do (no labels, no pred)");
    }
    hipStream_t st = (hipStream_t)stream;
    if (low_dt == DCLIP_F32)
        launch_seg<float>(logits, B, h, w, H, W, labels, lab_dt, ignore_index, pred, cm, loss_sum, count, ws, st);
    else if (low_dt == DCLIP_BF16)
        launch_seg<bf16>(logits, B, h, w, H, W, labels, lab_dt, ignore_index, pred, cm, loss_sum, count, ws, st);
    else
        launch_seg<f16>(logits, B, h, w, H, W, labels, lab_dt, ignore_index, pred, cm, loss_sum, count, ws, st);
    DCLIP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dclip_upsample_eval_depth(int low_dt, const void* pred, int B, int h, int w, const float* target,
                                         const uint8_t* mask, int H, int W, float min_depth, float max_depth,
                                         int clamp_pred, float eps, float* up, double* sums, void* ws, void* stream) {
    EVAL_SIZE_CHECKS("dclip_upsample_eval_depth");
    DCLIP_HOST_CHECK(pred && target && sums, "dclip_upsample_eval_depth: pred, target and sums required");
    DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                     "dclip_upsample_eval_depth: ws (dclip_upsample_eval_ws_bytes(B, 1, h, w) bytes, 8-byte aligned) "
                     "required");
    hipStream_t st = (hipStream_t)stream;
    if (low_dt == DCLIP_F32)
        launch_depth<float>(pred, B, h, w, H, W, target, mask, min_depth, max_depth, clamp_pred, eps, up, sums, ws, st);
    else if (low_dt == DCLIP_BF16)
        launch_depth<bf16>(pred, B, h, w, H, W, target, mask, min_depth, max_depth, clamp_pred, eps, up, sums, ws, st);
    else
        launch_depth<f16>(pred, B, h, w, H, W, target, mask, min_depth, max_depth, clamp_pred, eps, up, sums, ws, st);
    DCLIP_LAUNCH_CHECK();
    return 0;
}
