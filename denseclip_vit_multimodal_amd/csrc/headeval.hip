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
//
// This file keeps the single-view tile walk and interpolation; what follows a thread's K values /
// 4 depths (argmax, CE, confusion counts, the depth terms, the stores and the workgroup's record)
// is eval_tile.h's scoring epilogue, shared with headensemble / headslide / headslidetta.hip.
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
    finish_tiling(t, B, H, W);
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
    if constexpr (LAB) hist_clear<K>(hist_s);
    double lsum = 0.0;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const TileGeom g = tile_geom(tile, tl, h, w, H, W);
        __syncthreads();  // the previous tile's readers are done
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
        seg_score<K, 4, LAB, false>(v, t, n, ignore, hist_s, lsum, am);
        store_pred4(pred, pix, n, vec_pred != 0, am);
    }
    if constexpr (LAB) seg_flush<K>(hist_s, lsum, red_s, ws);
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
    DepthSums acc;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const TileGeom g = tile_geom(tile, tl, h, w, H, W);
        __syncthreads();
        stage_patch(low_s, low, g.b, 1, h, w, g.ilo, g.nr, g.jlo, g.nc, tl.nrow, tl.ncol);
        __syncthreads();
        const int y = g.y0 + ty, x = g.x0 + 4 * tx;
        if (y >= H || x >= W) continue;
        const int n = W - x < 4 ? W - x : 4;
        const int64_t pix = ((int64_t)g.b * H + y) * W + x;
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
            u[p] = bilerp_depth(p, Y.l0, Y.l1, X.l0, X.l1, top[c0], top[c1], bot[c0], bot[c1]);  // slot = column % 4
        }
        store_up4(up, pix, n, vec != 0, u);
        acc.score4(u, gt, mask, pix, n, vec != 0, dmin, dmax, clamp_pred, eps);
    }
    acc.flush(red_s, ws);
}

template <typename TL>
void launch_seg(const void* low, int B, int h, int w, int H, int W, const void* lab, int lab_dt, int ignore,
                uint8_t* pred, int64_t* cm, double* loss_sum, unsigned long long* count, void* ws, hipStream_t st) {
    constexpr int K = 19;
    const Tiling tl = make_tiling(B, K, h, w, H, W);
    const int nth = (tl.tw / 4) * TH;
    const int vec_lab = labels_aligned(lab, lab_dt, W), vec_pred = pred_aligned(pred, W);
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
    const int vec = depth_aligned(gt, mask, up, W);
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
    if (int rc = check_seg_outputs("dclip_upsample_eval_seg", labels, lab_dt, pred, cm, loss_sum, count)) return rc;
    if (labels != nullptr)
        DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                         "dclip_upsample_eval_seg: ws (dclip_upsample_eval_ws_bytes(B, K, h, w) bytes, 8-byte aligned) "
                         "required");
    hipStream_t st = (hipStream_t)stream;
    EVAL_DISPATCH_LOW(low_dt, launch_seg<TL>(logits, B, h, w, H, W, labels, lab_dt, ignore_index, pred, cm, loss_sum,
                                             count, ws, st));
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
    EVAL_DISPATCH_LOW(low_dt, launch_depth<TL>(pred, B, h, w, H, W, target, mask, min_depth, max_depth, clamp_pred, eps,
                                               up, sums, ws, st));
    DCLIP_LAUNCH_CHECK();
    return 0;
}
