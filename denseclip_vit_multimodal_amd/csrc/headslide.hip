// Sliding-window inference fused into the head evaluation (forward only).
//
// mmseg's slide_inference (the reference's test_cfg mode='slide') runs the model on overlapping
// crops of the image, resizes every crop's output to the crop size, pad-adds it into an image-sized
// (B, K, H, W) fp32 accumulator beside a count map, divides and takes argmax / CE: at 1024x2048 a
// 159 MB accumulator per image, written once per window.  Here, as in headensemble.hip, the resized
// values exist only in registers: a tile of 8 x TW output pixels loops over the windows that touch
// it, stages the window's low-res patch under the part of the tile inside the window in LDS (f32,
// [K][rows][cols]), interpolates in window-local coordinates with the ensemble's arithmetic and
// adds in f32 in table order; a pixel's result is its sum divided by the number of windows that
// cover it.  HBM traffic is the windows' low-res maps, the labels / targets and the u8 class map.
//
// All windows have one size (wh x ww at the output, h x w low-res), so the LDS patch has one size.
// The window table travels by value in the kernel arguments (no device-side table, no copy), so a
// launch can be captured in a graph.  Whether a tile skips a window depends on the tile alone:
// every thread of the workgroup reaches every barrier.  Tiling, the scoring epilogue (seg_score,
// DepthSums), per-workgroup records, f64 partials and the one-workgroup folds are eval_tile.h's, as
// in headeval.hip; this file keeps the loop over the windows and the division by the count: no
// global atomics, no float atomics, the grid a function of the shapes alone, two runs bitwise
// equal.  TW drops from 128 to 64 when the patch of a 128-wide tile passes 48 KiB.
#include "eval_tile.h"

namespace {

constexpr int MAXW = DCLIP_SLIDE_MAX_WINDOWS;

struct WinTable {
    dclip_window v[MAXW];
    int n;
};
// one size for every window: low-res h x w, resized to wh x ww, placed in the H x W image
struct WinShape {
    int h, w, wh, ww, H, W;
};

Tiling make_tiling(int B, int K, const WinShape& s) {
    Tiling t;
    t.tw = 128;
    for (int pass = 0; pass < 2; ++pass) {
        t.nrow = low_span(TH, s.h, s.wh);
        t.ncol = low_span(t.tw, s.w, s.ww);
        t.lds = (size_t)K * t.nrow * t.ncol * 4;
        if (t.lds <= (size_t)LDS_TILE_MAX) break;
        t.tw = 64;
    }
    finish_tiling(t, B, s.H, s.W);
    return t;
}

// The patch of the window at (wy, wx) under the output tile at (y0, x0): tile_geom on the rows and
// columns of the tile that lie inside the window, in window-local coordinates.  False when the tile
// and the window do not intersect (a function of the tile alone: workgroup-uniform).
__device__ __forceinline__ bool win_geom(int y0, int x0, int tw, int wy, int wx, const WinShape& s, int nrow, int ncol,
                                         TileGeom& g) {
    const int y1 = y0 + TH - 1 < s.H ? y0 + TH - 1 : s.H - 1;
    const int x1 = x0 + tw - 1 < s.W ? x0 + tw - 1 : s.W - 1;
    const int ya = y0 > wy ? y0 : wy, yb = y1 < wy + s.wh - 1 ? y1 : wy + s.wh - 1;
    const int xa = x0 > wx ? x0 : wx, xb = x1 < wx + s.ww - 1 ? x1 : wx + s.ww - 1;
    if (ya > yb || xa > xb) return false;
    g.y0 = y0;
    g.x0 = x0;
    g.ilo = lerp_index(ya - wy, s.h, s.wh).i0;
    g.jlo = lerp_index(xa - wx, s.w, s.ww).i0;
    g.nr = lerp_index(yb - wy, s.h, s.wh).i1 - g.ilo + 1;
    g.nc = lerp_index(xb - wx, s.w, s.ww).i1 - g.jlo + 1;
    g.nr = g.nr < nrow ? g.nr : nrow;  // low_span() bounds both; never index LDS past the patch
    g.nc = g.nc < ncol ? g.nc : ncol;
    return true;
}

// ----------------------------------------------------------------------------- segmentation
// LAB: labels given (confusion matrix, CE sum, #valid); pred may be null then.  !LAB: pred only.
template <typename TL, int K, bool LAB>
__global__ __launch_bounds__(256) void slide_seg_kernel(WinTable wt, WinShape s, Tiling tl,
                                                        const void* __restrict__ lab, int lab_dt, int ignore,
                                                        int vec_lab, int vec_pred, uint8_t* __restrict__ pred,
                                                        char* __restrict__ ws) {
    extern __shared__ float low_s[];
    __shared__ unsigned hist_s[K * K + 1];
    __shared__ double red_s[4];
    const int tid = threadIdx.x;
    const int xs = tl.tw >> 2;  // threads along x
    const int tx = tid % xs, ty = tid / xs;
    const int H = s.H, W = s.W;
    if constexpr (LAB) hist_clear<K>(hist_s);
    double lsum = 0.0;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto [b, y0, x0] = tile_origin(tile, tl);
        const int y = y0 + ty, x = x0 + 4 * tx;
        const bool active = y < H && x < W;  // every thread stages every patch
        float v[4][K];
        int cnt[4] = {0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int k = 0; k < K; ++k) v[p][k] = 0.f;
        for (int iw = 0; iw < wt.n; ++iw) {
            const int wy = wt.v[iw].y0, wx = wt.v[iw].x0;
            TileGeom g;
            if (!win_geom(y0, x0, tl.tw, wy, wx, s, tl.nrow, tl.ncol, g)) continue;  // workgroup-uniform
            __syncthreads();  // the previous patch's readers are done
            stage_patch(low_s, (const TL*)wt.v[iw].low, b, K, s.h, s.w, g.ilo, g.nr, g.jlo, g.nc, tl.nrow, tl.ncol);
            __syncthreads();
            // the thread's pixels this window covers
            const bool in_row = active && y >= wy && y < wy + s.wh;
            bool cov[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) cov[p] = in_row && x + p >= wx && x + p < wx + s.ww;
            if (!(cov[0] || cov[1] || cov[2] || cov[3])) continue;
            const Lerp Y = lerp_index(y - wy, s.h, s.wh);
            const int r0 = clampi(Y.i0 - g.ilo, 0, g.nr - 1), r1 = clampi(Y.i1 - g.ilo, 0, g.nr - 1);
            Lerp X[4];
            int c0[4], c1[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                // an uncovered pixel evaluates the window's nearest column; its value is dropped
                X[p] = lerp_index(clampi(x + p - wx, 0, s.ww - 1), s.w, s.ww);
                c0[p] = clampi(X[p].i0 - g.jlo, 0, g.nc - 1);
                c1[p] = clampi(X[p].i1 - g.jlo, 0, g.nc - 1);
                cnt[p] += cov[p] ? 1 : 0;
            }
            // the four pixels usually share their two low-res columns (always at the workload's x16)
            const bool same = c0[0] == c0[3] && c1[0] == c1[3];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float* top = low_s + (k * tl.nrow + r0) * tl.ncol;
                const float* bot = low_s + (k * tl.nrow + r1) * tl.ncol;
                float u[4];
                if (same) {
                    const float a00 = top[c0[0]], a01 = top[c1[0]], a10 = bot[c0[0]], a11 = bot[c1[0]];
#pragma unroll
                    for (int p = 0; p < 4; ++p) u[p] = bilerp(Y.l0, Y.l1, X[p].l0, X[p].l1, a00, a01, a10, a11);
                } else {
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        u[p] = bilerp(Y.l0, Y.l1, X[p].l0, X[p].l1, top[c0[p]], top[c1[p]], bot[c0[p]], bot[c1[p]]);
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) v[p][k] = cov[p] ? add_rounded(v[p][k], u[p]) : v[p][k];
            }
        }
        if (!active) continue;
        const int n = W - x < 4 ? W - x : 4;
        const int64_t pix = ((int64_t)b * H + y) * W + x;
        int t[4] = {-1, -1, -1, -1};
        if constexpr (LAB) load_labels4(lab, lab_dt, pix, n, vec_lab != 0, t);
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (cnt[p] > 1) {  // x / 1 is x
                const float c = (float)cnt[p];
#pragma unroll
                for (int k = 0; k < K; ++k) v[p][k] = div_rounded(v[p][k], c);
            }
        int am[4];
        seg_score<K, 4, LAB, false>(v, t, n, ignore, hist_s, lsum, am);
        store_pred4(pred, pix, n, vec_pred != 0, am);
    }
    if constexpr (LAB) seg_flush<K>(hist_s, lsum, red_s, ws);
}

// ----------------------------------------------------------------------------- depth
// TGT: target given (the 12 sums); up may be null then.  !TGT: the mean map only.
template <typename TL, bool TGT>
__global__ __launch_bounds__(256) void slide_depth_kernel(WinTable wt, WinShape s, Tiling tl,
                                                          const float* __restrict__ gt,
                                                          const uint8_t* __restrict__ mask, float dmin, float dmax,
                                                          int clamp_pred, float eps, int vec, float* __restrict__ up,
                                                          char* __restrict__ ws) {
    extern __shared__ float low_s[];
    __shared__ double red_s[4 * NSUM];
    const int tid = threadIdx.x;
    const int xs = tl.tw >> 2;
    const int tx = tid % xs, ty = tid / xs;
    const int H = s.H, W = s.W;
    DepthSums acc;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto [b, y0, x0] = tile_origin(tile, tl);
        const int y = y0 + ty, x = x0 + 4 * tx;
        const bool active = y < H && x < W;
        float u[4] = {0.f, 0.f, 0.f, 0.f};
        int cnt[4] = {0, 0, 0, 0};
        for (int iw = 0; iw < wt.n; ++iw) {
            const int wy = wt.v[iw].y0, wx = wt.v[iw].x0;
            TileGeom g;
            if (!win_geom(y0, x0, tl.tw, wy, wx, s, tl.nrow, tl.ncol, g)) continue;  // workgroup-uniform
            __syncthreads();
            stage_patch(low_s, (const TL*)wt.v[iw].low, b, 1, s.h, s.w, g.ilo, g.nr, g.jlo, g.nc, tl.nrow, tl.ncol);
            __syncthreads();
            const bool in_row = active && y >= wy && y < wy + s.wh;
            if (!in_row || x + 3 < wx || x >= wx + s.ww) continue;
            const Lerp Y = lerp_index(y - wy, s.h, s.wh);
            const int r0 = clampi(Y.i0 - g.ilo, 0, g.nr - 1), r1 = clampi(Y.i1 - g.ilo, 0, g.nr - 1);
            const float* top = low_s + r0 * tl.ncol;
            const float* bot = low_s + r1 * tl.ncol;
            // bilerp_depth's roundings depend on the slot, and slot q always evaluates a window-local
            // column congruent to q mod 4, as the single-view kernel does on a map of the window's
            // size: x is a multiple of 4, so that is output pixel p = (q + wx) & 3 of the thread.
            // A window then contributes the values of its own resize, wherever it lies.
            float r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = (q + wx) & 3;
                const int xp = x + p < W ? x + p : W - 1;
                const Lerp X = lerp_index(clampi(xp - wx, 0, s.ww - 1), s.w, s.ww);
                const int c0 = clampi(X.i0 - g.jlo, 0, g.nc - 1), c1 = clampi(X.i1 - g.jlo, 0, g.nc - 1);
                r[q] = bilerp_depth(q, Y.l0, Y.l1, X.l0, X.l1, top[c0], top[c1], bot[c0], bot[c1]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = (q + wx) & 3;
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const bool hit = o == p && x + o >= wx && x + o < wx + s.ww;
                    u[o] = hit ? add_rounded(u[o], r[q]) : u[o];
                    cnt[o] += hit ? 1 : 0;
                }
            }
        }
        if (!active) continue;
        const int n = W - x < 4 ? W - x : 4;
        const int64_t pix = ((int64_t)b * H + y) * W + x;
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (cnt[p] > 1) u[p] = div_rounded(u[p], (float)cnt[p]);
        store_up4(up, pix, n, vec != 0, u);
        if constexpr (TGT) acc.score4(u, gt, mask, pix, n, vec != 0, dmin, dmax, clamp_pred, eps);
    }
    if constexpr (TGT) acc.flush(red_s, ws);
}

template <typename TL>
void launch_seg(const WinTable& wt, const WinShape& s, int B, const void* lab, int lab_dt, int ignore, uint8_t* pred,
                int64_t* cm, double* loss_sum, unsigned long long* count, void* ws, hipStream_t st) {
    constexpr int K = 19;
    const Tiling tl = make_tiling(B, K, s);
    const int nth = (tl.tw / 4) * TH;
    const int vec_lab = labels_aligned(lab, lab_dt, s.W), vec_pred = pred_aligned(pred, s.W);
    if (lab != nullptr) {
        slide_seg_kernel<TL, K, true><<<tl.nwg, nth, tl.lds, st>>>(wt, s, tl, lab, lab_dt, ignore, vec_lab, vec_pred,
                                                                   pred, (char*)ws);
        eval_seg_fold_kernel<<<1, 256, 0, st>>>((const char*)ws, tl.nwg, K, cm, loss_sum, count);
    } else {
        slide_seg_kernel<TL, K, false><<<tl.nwg, nth, tl.lds, st>>>(wt, s, tl, nullptr, 0, ignore, 0, vec_pred, pred,
                                                                    (char*)ws);
    }
}

template <typename TL>
void launch_depth(const WinTable& wt, const WinShape& s, int B, const float* gt, const uint8_t* mask, float dmin,
                  float dmax, int clamp_pred, float eps, float* up, double* sums, void* ws, hipStream_t st) {
    const Tiling tl = make_tiling(B, 1, s);
    const int nth = (tl.tw / 4) * TH;
    const int vec = depth_aligned(gt, mask, up, s.W);
    if (gt != nullptr) {
        slide_depth_kernel<TL, true><<<tl.nwg, nth, tl.lds, st>>>(wt, s, tl, gt, mask, dmin, dmax, clamp_pred, eps, vec,
                                                                  up, (char*)ws);
        eval_depth_fold_kernel<<<1, 256, 0, st>>>((const char*)ws, tl.nwg, sums);
    } else {
        slide_depth_kernel<TL, false><<<tl.nwg, nth, tl.lds, st>>>(wt, s, tl, nullptr, nullptr, dmin, dmax, clamp_pred,
                                                                   eps, vec, up, nullptr);
    }
}

// The checks shared by both entry points; fills the kernel's window table and shape.
int check_windows(const char* name, int low_dt, const dclip_window* wins, int nwin, int B, int h, int w, int wh, int ww,
                  int H, int W, WinTable& wt, WinShape& shape) {
    DCLIP_HOST_CHECK(nwin >= 1 && nwin <= MAXW, "%s: nwin=%d (1 .. %d windows)", name, nwin, MAXW);
    DCLIP_HOST_CHECK(wins != nullptr, "%s: wins required", name);
    DCLIP_HOST_CHECK(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "%s: bad sizes (B=%d, h=%d, w=%d, H=%d, W=%d)", name, B,
                     h, w, H, W);
    DCLIP_HOST_CHECK(low_dt == DCLIP_F32 || low_dt == DCLIP_F16 || low_dt == DCLIP_BF16,
                     "%s: low_dt=%d (f32, f16 or bf16)", name, low_dt);
    DCLIP_HOST_CHECK(h <= wh && wh <= H, "%s: h=%d <= wh=%d <= H=%d required (window rows)", name, h, wh, H);
    DCLIP_HOST_CHECK(w <= ww && ww <= W, "%s: w=%d <= ww=%d <= W=%d required (window columns)", name, w, ww, W);
    DCLIP_HOST_CHECK((int64_t)B * H * W < ((int64_t)1 << 31), "%s: B*H*W = %lld pixels (must be below 2^31)", name,
                     (long long)((int64_t)B * H * W));
    wt.n = nwin;
    for (int i = 0; i < MAXW; ++i) wt.v[i] = dclip_window{nullptr, 0, 0};
    for (int i = 0; i < nwin; ++i) {
        const dclip_window& v = wins[i];
        DCLIP_HOST_CHECK(v.low != nullptr, "%s: window %d: low is null", name, i);
        DCLIP_HOST_CHECK(v.y0 >= 0 && v.y0 <= H - wh, "%s: window %d: y0=%d (0 <= y0, y0 + wh=%d <= H=%d)", name, i, v.y0,
                         wh, H);
        DCLIP_HOST_CHECK(v.x0 >= 0 && v.x0 <= W - ww, "%s: window %d: x0=%d (0 <= x0, x0 + ww=%d <= W=%d)", name, i, v.x0,
                         ww, W);
        wt.v[i] = v;
    }
    int uy = 0, ux = 0;
    DCLIP_HOST_CHECK(!first_uncovered(wins, nwin, wh, ww, H, W, &uy, &ux), "%s: pixel (y=%d, x=%d) is covered by no window",
                     name, uy, ux);
    shape = WinShape{h, w, wh, ww, H, W};
    return 0;
}

}  // namespace

extern "C" int64_t dclip_slide_eval_ws_bytes(int B, int K, int nwin) {
    if (B <= 0 || K <= 0 || nwin <= 0 || nwin > MAXW) return 0;
    return (int64_t)NWG_MAX * record_bytes(K);
}

extern "C" int dclip_slide_eval_seg(int low_dt, const dclip_window* wins, int nwin, int B, int K, int h, int w, int wh,
                                    int ww, const void* labels, int lab_dt, int H, int W, int ignore_index,
                                    uint8_t* pred, int64_t* cm, double* loss_sum, unsigned long long* count, void* ws,
                                    void* stream) {
    DCLIP_HOST_CHECK(K == 19, "dclip_slide_eval_seg: K=%d (built for the 19 Cityscapes classes)", K);
    WinTable wt;
    WinShape shape;
    if (int rc = check_windows("dclip_slide_eval_seg", low_dt, wins, nwin, B, h, w, wh, ww, H, W, wt, shape)) return rc;
    if (int rc = check_seg_outputs("dclip_slide_eval_seg", labels, lab_dt, pred, cm, loss_sum, count)) return rc;
    if (labels != nullptr)
        DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                         "dclip_slide_eval_seg: ws=%p (dclip_slide_eval_ws_bytes(B, K, nwin) bytes, 8-byte aligned) "
                         "required", ws);
    hipStream_t st = (hipStream_t)stream;
    EVAL_DISPATCH_LOW(low_dt, launch_seg<TL>(wt, shape, B, labels, lab_dt, ignore_index, pred, cm, loss_sum, count, ws, st));
    DCLIP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dclip_slide_eval_depth(int low_dt, const dclip_window* wins, int nwin, int B, int h, int w, int wh,
                                      int ww, const float* target, const uint8_t* mask, int H, int W, float min_depth,
                                      float max_depth, int clamp_pred, float eps, float* up, double* sums, void* ws,
                                      void* stream) {
    WinTable wt;
    WinShape shape;
    if (int rc = check_windows("dclip_slide_eval_depth", low_dt, wins, nwin, B, h, w, wh, ww, H, W, wt, shape)) return rc;
    if (int rc = check_depth_outputs("dclip_slide_eval_depth", target, sums, up)) return rc;
    if (target != nullptr)
        DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                         "dclip_slide_eval_depth: ws=%p (dclip_slide_eval_ws_bytes(B, 1, nwin) bytes, 8-byte aligned) "
                         "required", ws);
    hipStream_t st = (hipStream_t)stream;
    EVAL_DISPATCH_LOW(low_dt, launch_depth<TL>(wt, shape, B, target, mask, min_depth, max_depth, clamp_pred, eps, up, sums,
                                               ws, st));
    DCLIP_LAUNCH_CHECK();
    return 0;
}
