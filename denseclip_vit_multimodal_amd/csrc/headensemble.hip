// Multi-scale + flip test-time ensembling fused into the head evaluation (forward only).
//
// The reference's aug_test (denseclip.py:1005-1041, test.py:91-96) resizes the output of every view
// (six ratios, each plain and mirrored) to the image size and averages the 12 full-size tensors: at
// 1024x2048 a 19-channel fp32 tensor of 159 MB per view, stacked, reduced and read back by argmax.
// Here, as in headeval.hip, the resized values exist only in registers: a tile of 8 x TW output
// pixels loops over the V views, stages each view's low-res patch in LDS (f32, [K][rows][cols]),
// interpolates with headeval's arithmetic and accumulates in f32 in view order; the class map, the
// confusion matrix, the CE sum and the depth sums are taken from the mean.  HBM traffic is the V
// low-res maps, the labels / targets and the u8 class map.
//
// A flipped view was computed on the mirrored image, so its resized map is mirrored back: output
// column x reads the view's resize at column W-1-x (F.interpolate(...).flip(-1)), and the tile
// stages the patch of its mirrored column range.
//
// Two averaging rules: the mean of the resized logits (the reference's), or the mean of the
// softmax over the classes of each view's resized logits (mmseg's).
//
// The view table travels by value in the kernel arguments (no device-side table, no copy), so a
// launch can be captured in a graph.  Tiling, the scoring epilogue (seg_score, DepthSums), per-workgroup
// records, f64 partials and the one-workgroup folds are eval_tile.h's, as in headeval.hip; this file
// keeps the loop over the views and the scaling by 1/V: no global atomics, no float atomics, the grid
// a function of the shapes alone, two runs bitwise equal.  LDS is sized for the largest view's
// patch; TW drops from 128 to 64 when any view's patch of a 128-wide tile passes 48 KiB.
#include "eval_tile.h"

namespace {

constexpr int MAXV = DCLIP_ENSEMBLE_MAX_VIEWS;

struct View {
    const void* low;
    int h, w, flip;
    int nrow, ncol;  // the LDS patch of this view: low_span of a tile's rows / columns
};
struct ViewTable {
    View v[MAXV];
    int n;
};

// tw, the grid and the LDS bytes of the largest patch; fills every view's nrow / ncol
Tiling make_tiling(int B, int K, ViewTable& vt, int H, int W) {
    Tiling t;
    t.tw = 128;
    for (int pass = 0; pass < 2; ++pass) {
        t.lds = 0;
        for (int i = 0; i < vt.n; ++i) {
            View& v = vt.v[i];
            v.nrow = low_span(TH, v.h, H);
            v.ncol = low_span(t.tw, v.w, W);
            const size_t bytes = (size_t)K * v.nrow * v.ncol * 4;
            t.lds = bytes > t.lds ? bytes : t.lds;
        }
        if (t.lds <= (size_t)LDS_TILE_MAX) break;
        t.tw = 64;
    }
    t.nrow = t.ncol = 0;  // per view, in the table
    finish_tiling(t, B, H, W);
    return t;
}

// the patch of view `v` under the output tile at (y0, x0): tile_geom on the columns the tile reads,
// [x0, x1] of a plain view and [W-1-x1, W-1-x0] of a flipped one
__device__ __forceinline__ TileGeom view_geom(int b, int y0, int x0, int tw, const View& v, int H, int W) {
    TileGeom g;
    g.b = b;
    g.y0 = y0;
    g.x0 = x0;
    const int y1 = y0 + TH - 1 < H ? y0 + TH - 1 : H - 1;
    const int x1 = x0 + tw - 1 < W ? x0 + tw - 1 : W - 1;
    const int xa = v.flip ? W - 1 - x1 : x0, xb = v.flip ? W - 1 - x0 : x1;
    g.ilo = lerp_index(y0, v.h, H).i0;
    g.jlo = lerp_index(xa, v.w, W).i0;
    g.nr = lerp_index(y1, v.h, H).i1 - g.ilo + 1;
    g.nc = lerp_index(xb, v.w, W).i1 - g.jlo + 1;
    g.nr = g.nr < v.nrow ? g.nr : v.nrow;  // low_span() bounds both; never index LDS past the patch
    g.nc = g.nc < v.ncol ? g.nc : v.ncol;
    return g;
}

// ----------------------------------------------------------------------------- segmentation
// LAB: labels given (confusion matrix, CE sum, #valid); pred may be null then.  !LAB: pred only.
// PROBS: accumulate softmax(resized logits) of every view instead of the resized logits.
template <typename TL, int K, bool LAB, bool PROBS>
__global__ __launch_bounds__(256) void ensemble_seg_kernel(ViewTable vt, int H, int W, Tiling tl,
                                                           const void* __restrict__ lab, int lab_dt, int ignore,
                                                           int vec_lab, int vec_pred, uint8_t* __restrict__ pred,
                                                           char* __restrict__ ws) {
    extern __shared__ float low_s[];
    __shared__ unsigned hist_s[K * K + 1];
    __shared__ double red_s[4];
    const int tid = threadIdx.x;
    const int xs = tl.tw >> 2;  // threads along x
    const int tx = tid % xs, ty = tid / xs;
    const float inv_v = 1.f / (float)vt.n;
    if constexpr (LAB) hist_clear<K>(hist_s);
    double lsum = 0.0;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto [b, y0, x0] = tile_origin(tile, tl);
        const int y = y0 + ty, x = x0 + 4 * tx;
        const bool active = y < H && x < W;  // every thread stages every view's patch
        float v[4][K];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int k = 0; k < K; ++k) v[p][k] = 0.f;
        for (int iv = 0; iv < vt.n; ++iv) {
            const View vw = vt.v[iv];
            const TileGeom g = view_geom(b, y0, x0, tl.tw, vw, H, W);
            __syncthreads();  // the previous patch's readers are done
            stage_patch(low_s, (const TL*)vw.low, b, K, vw.h, vw.w, g.ilo, g.nr, g.jlo, g.nc, vw.nrow, vw.ncol);
            __syncthreads();
            if (!active) continue;
            const Lerp Y = lerp_index(y, vw.h, H);
            int r0 = Y.i0 - g.ilo, r1 = Y.i1 - g.ilo;
            r0 = r0 < g.nr ? r0 : g.nr - 1;
            r1 = r1 < g.nr ? r1 : g.nr - 1;
            Lerp X[4];
            int c0[4], c1[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int xp = x + p < W ? x + p : W - 1;
                X[p] = lerp_index(vw.flip ? W - 1 - xp : xp, vw.w, W);
                c0[p] = X[p].i0 - g.jlo;
                c1[p] = X[p].i1 - g.jlo;
                c0[p] = c0[p] < g.nc ? c0[p] : g.nc - 1;
                c1[p] = c1[p] < g.nc ? c1[p] : g.nc - 1;
            }
            // the four pixels usually share their two low-res columns (always at the workload's x16)
            const bool same = c0[0] == c0[3] && c1[0] == c1[3];
            float u[4][K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float* top = low_s + (k * vw.nrow + r0) * vw.ncol;
                const float* bot = low_s + (k * vw.nrow + r1) * vw.ncol;
                if (same) {
                    const float a00 = top[c0[0]], a01 = top[c1[0]], a10 = bot[c0[0]], a11 = bot[c1[0]];
#pragma unroll
                    for (int p = 0; p < 4; ++p) u[p][k] = bilerp(Y.l0, Y.l1, X[p].l0, X[p].l1, a00, a01, a10, a11);
                } else {
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        u[p][k] = bilerp(Y.l0, Y.l1, X[p].l0, X[p].l1, top[c0[p]], top[c1[p]], bot[c0[p]],
                                         bot[c1[p]]);
                }
                if constexpr (!PROBS) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) v[p][k] = add_rounded(v[p][k], u[p][k]);
                }
            }
            if constexpr (PROBS) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    float m = u[p][0];
#pragma unroll
                    for (int k = 1; k < K; ++k) m = fmaxf(m, u[p][k]);
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        u[p][k] = __expf(u[p][k] - m);
                        s += u[p][k];
                    }
                    const float inv = 1.f / s;
#pragma unroll
                    for (int k = 0; k < K; ++k) v[p][k] += u[p][k] * inv;
                }
            }
        }
        if (!active) continue;
        const int n = W - x < 4 ? W - x : 4;
        const int64_t pix = ((int64_t)b * H + y) * W + x;
        int t[4] = {-1, -1, -1, -1};
        if constexpr (LAB) load_labels4(lab, lab_dt, pix, n, vec_lab != 0, t);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int k = 0; k < K; ++k) v[p][k] *= inv_v;
        int am[4];
        seg_score<K, 4, LAB, PROBS>(v, t, n, ignore, hist_s, lsum, am);
        store_pred4(pred, pix, n, vec_pred != 0, am);
    }
    if constexpr (LAB) seg_flush<K>(hist_s, lsum, red_s, ws);
}

// ----------------------------------------------------------------------------- depth
// TGT: target given (the 12 sums); up may be null then.  !TGT: the mean map only.
template <typename TL, bool TGT>
__global__ __launch_bounds__(256) void ensemble_depth_kernel(ViewTable vt, int H, int W, Tiling tl,
                                                             const float* __restrict__ gt,
                                                             const uint8_t* __restrict__ mask, float dmin, float dmax,
                                                             int clamp_pred, float eps, int vec,
                                                             float* __restrict__ up, char* __restrict__ ws) {
    extern __shared__ float low_s[];
    __shared__ double red_s[4 * NSUM];
    const int tid = threadIdx.x;
    const int xs = tl.tw >> 2;
    const int tx = tid % xs, ty = tid / xs;
    const float inv_v = 1.f / (float)vt.n;
    DepthSums acc;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto [b, y0, x0] = tile_origin(tile, tl);
        const int y = y0 + ty, x = x0 + 4 * tx;
        const bool active = y < H && x < W;
        float u[4] = {0.f, 0.f, 0.f, 0.f};
        for (int iv = 0; iv < vt.n; ++iv) {
            const View vw = vt.v[iv];
            const TileGeom g = view_geom(b, y0, x0, tl.tw, vw, H, W);
            __syncthreads();
            stage_patch(low_s, (const TL*)vw.low, b, 1, vw.h, vw.w, g.ilo, g.nr, g.jlo, g.nc, vw.nrow, vw.ncol);
            __syncthreads();
            if (!active) continue;
            const Lerp Y = lerp_index(y, vw.h, H);
            int r0 = Y.i0 - g.ilo, r1 = Y.i1 - g.ilo;
            r0 = r0 < g.nr ? r0 : g.nr - 1;
            r1 = r1 < g.nr ? r1 : g.nr - 1;
            const float* top = low_s + r0 * vw.ncol;
            const float* bot = low_s + r1 * vw.ncol;
            // bilerp_depth's roundings depend on the slot, so slot q always evaluates a source column
            // congruent to q mod 4 (x is a multiple of 4): column x + q of a plain view, as in headeval,
            // and of a flipped view the column W-1-(x+p) with p = (W-1-q) & 3, whose value goes to
            // output pixel p.  A source column then goes through the same arithmetic whether the view
            // is flipped or not: the flipped result is the exact column mirror.
            float r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = vw.flip ? (W - 1 - q) & 3 : q;
                const int xp = x + p < W ? x + p : W - 1;
                const Lerp X = lerp_index(vw.flip ? W - 1 - xp : xp, vw.w, W);
                int c0 = X.i0 - g.jlo, c1 = X.i1 - g.jlo;
                c0 = c0 < g.nc ? c0 : g.nc - 1;
                c1 = c1 < g.nc ? c1 : g.nc - 1;
                r[q] = bilerp_depth(q, Y.l0, Y.l1, X.l0, X.l1, top[c0], top[c1], bot[c0], bot[c1]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = vw.flip ? (W - 1 - q) & 3 : q;
#pragma unroll
                for (int o = 0; o < 4; ++o) u[o] = o == p ? add_rounded(u[o], r[q]) : u[o];
            }
        }
        if (!active) continue;
        const int n = W - x < 4 ? W - x : 4;
        const int64_t pix = ((int64_t)b * H + y) * W + x;
#pragma unroll
        for (int p = 0; p < 4; ++p) u[p] *= inv_v;
        store_up4(up, pix, n, vec != 0, u);
        if constexpr (TGT) acc.score4(u, gt, mask, pix, n, vec != 0, dmin, dmax, clamp_pred, eps);
    }
    if constexpr (TGT) acc.flush(red_s, ws);
}

template <typename TL, bool PROBS>
void launch_seg(ViewTable& vt, int B, int H, int W, const void* lab, int lab_dt, int ignore, uint8_t* pred,
                int64_t* cm, double* loss_sum, unsigned long long* count, void* ws, hipStream_t st) {
    constexpr int K = 19;
    const Tiling tl = make_tiling(B, K, vt, H, W);
    const int nth = (tl.tw / 4) * TH;
    const int vec_lab = labels_aligned(lab, lab_dt, W), vec_pred = pred_aligned(pred, W);
    if (lab != nullptr) {
        ensemble_seg_kernel<TL, K, true, PROBS><<<tl.nwg, nth, tl.lds, st>>>(vt, H, W, tl, lab, lab_dt, ignore, vec_lab,
                                                                             vec_pred, pred, (char*)ws);
        eval_seg_fold_kernel<<<1, 256, 0, st>>>((const char*)ws, tl.nwg, K, cm, loss_sum, count);
    } else {
        ensemble_seg_kernel<TL, K, false, PROBS><<<tl.nwg, nth, tl.lds, st>>>(vt, H, W, tl, nullptr, 0, ignore, 0,
                                                                              vec_pred, pred, (char*)ws);
    }
}

template <typename TL>
void launch_depth(ViewTable& vt, int B, int H, int W, const float* gt, const uint8_t* mask, float dmin, float dmax,
                  int clamp_pred, float eps, float* up, double* sums, void* ws, hipStream_t st) {
    const Tiling tl = make_tiling(B, 1, vt, H, W);
    const int nth = (tl.tw / 4) * TH;
    const int vec = depth_aligned(gt, mask, up, W);
    if (gt != nullptr) {
        ensemble_depth_kernel<TL, true><<<tl.nwg, nth, tl.lds, st>>>(vt, H, W, tl, gt, mask, dmin, dmax, clamp_pred,
                                                                     eps, vec, up, (char*)ws);
        eval_depth_fold_kernel<<<1, 256, 0, st>>>((const char*)ws, tl.nwg, sums);
    } else {
        ensemble_depth_kernel<TL, false><<<tl.nwg, nth, tl.lds, st>>>(vt, H, W, tl, nullptr, nullptr, dmin, dmax,
                                                                      clamp_pred, eps, vec, up, nullptr);
    }
}

}  // namespace

extern "C" int64_t dclip_ensemble_eval_ws_bytes(int B, int K, int nviews) {
    if (B <= 0 || K <= 0 || nviews <= 0 || nviews > MAXV) return 0;
    return (int64_t)NWG_MAX * record_bytes(K);
}

// the checks shared by both entry points; fills the kernel's view table
#define ENSEMBLE_VIEW_CHECKS(NAME)                                                                                 \
    DCLIP_HOST_CHECK(nviews >= 1 && nviews <= MAXV, NAME ": nviews=%d (1 .. %d views)", nviews, MAXV);             \
    DCLIP_HOST_CHECK(views != nullptr, NAME ": views required");                                                   \
    DCLIP_HOST_CHECK(B > 0 && H > 0 && W > 0, NAME ": bad sizes (B=%d, H=%d, W=%d)", B, H, W);                     \
    DCLIP_HOST_CHECK(low_dt == DCLIP_F32 || low_dt == DCLIP_F16 || low_dt == DCLIP_BF16,                           \
                     NAME ": low_dt=%d (f32, f16 or bf16)", low_dt);                                               \
    DCLIP_HOST_CHECK((int64_t)B * H * W < ((int64_t)1 << 31), NAME ": B*H*W = %lld pixels (must be below 2^31)",    \
                     (long long)((int64_t)B * H * W));                                                             \
    ViewTable vt;                                                                                                  \
    vt.n = nviews;                                                                                                 \
    for (int i = 0; i < MAXV; ++i) vt.v[i] = View{nullptr, 0, 0, 0, 0, 0};                                         \
    for (int i = 0; i < nviews; ++i) {                                                                             \
        const dclip_view& v = views[i];                                                                            \
        DCLIP_HOST_CHECK(v.low != nullptr, NAME ": view %d: low is null", i);                                      \
        DCLIP_HOST_CHECK(v.h > 0 && v.w > 0, NAME ": view %d: bad size %d x %d", i, v.h, v.w);                     \
        DCLIP_HOST_CHECK(v.flip == 0 || v.flip == 1, NAME ": view %d: flip=%d (0 or 1)", i, v.flip);               \
        DCLIP_HOST_CHECK(H >= v.h && W >= v.w,                                                                     \
                         NAME ": view %d: the output (%d x %d) must not be smaller than the input (%d x %d)", i,   \
                         H, W, v.h, v.w);                                                                          \
        vt.v[i] = View{v.low, v.h, v.w, v.flip, 0, 0};                                                             \
    }

extern "C" int dclip_ensemble_eval_seg(int low_dt, const dclip_view* views, int nviews, int B, int K, int average,
                                       const void* labels, int lab_dt, int H, int W, int ignore_index, uint8_t* pred,
                                       int64_t* cm, double* loss_sum, unsigned long long* count, void* ws,
                                       void* stream) {
    DCLIP_HOST_CHECK(K == 19, "dclip_ensemble_eval_seg: K=%d (built for the 19 Cityscapes classes)", K);
    DCLIP_HOST_CHECK(average == 0 || average == 1,
                     "dclip_ensemble_eval_seg: average=%d (0: mean of the logits, 1: mean of the probabilities)",
                     average);
    ENSEMBLE_VIEW_CHECKS("dclip_ensemble_eval_seg");
    if (int rc = check_seg_outputs("dclip_ensemble_eval_seg", labels, lab_dt, pred, cm, loss_sum, count)) return rc;
    if (labels != nullptr)
        DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                         "dclip_ensemble_eval_seg: ws=%p (dclip_ensemble_eval_ws_bytes(B, K, nviews) bytes, 8-byte "
                         "aligned) required", ws);
    hipStream_t st = (hipStream_t)stream;
    EVAL_DISPATCH_LOW(low_dt, (average ? launch_seg<TL, true> : launch_seg<TL, false>)(
                                  vt, B, H, W, labels, lab_dt, ignore_index, pred, cm, loss_sum, count, ws, st));
    DCLIP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dclip_ensemble_eval_depth(int low_dt, const dclip_view* views, int nviews, int B, const float* target,
                                         const uint8_t* mask, int H, int W, float min_depth, float max_depth,
                                         int clamp_pred, float eps, float* up, double* sums, void* ws, void* stream) {
    ENSEMBLE_VIEW_CHECKS("dclip_ensemble_eval_depth");
    if (int rc = check_depth_outputs("dclip_ensemble_eval_depth", target, sums, up)) return rc;
    if (target != nullptr)
        DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                         "dclip_ensemble_eval_depth: ws=%p (dclip_ensemble_eval_ws_bytes(B, 1, nviews) bytes, 8-byte "
                         "aligned) required", ws);
    hipStream_t st = (hipStream_t)stream;
    EVAL_DISPATCH_LOW(low_dt, launch_depth<TL>(vt, B, H, W, target, mask, min_depth, max_depth, clamp_pred, eps, up, sums,
                                               ws, st));
    DCLIP_LAUNCH_CHECK();
    return 0;
}
