// Sliding-window inference inside multi-scale + flip ensembling, fused into the head evaluation
// (forward only).
//
// mmseg's aug_test over slide_inference (the reference's ViT configs under test.py --aug-test)
// evaluates every scaled and mirrored view with overlapping windows: per view a (B, K, Hv, Wv) fp32
// accumulator and a count map, a copy resized to the image, a softmax copy.  Here, as in
// headensemble.hip and headslide.hip, those values exist only in registers.  A workgroup owns a tile
// of 8 x (32 PX) output pixels (PX = 1 for the 19 classes, 4 for the depth) and loops over the views;
// an output pixel reads a view's slide result S_v at up to 4 view-space taps (1 when the view has the
// image's size), and a tap is the mean, over the windows that cover it, of the window's map resized
// to the window's size.  Per view the workgroup loops over the windows that touch the tile's
// view-space footprint, stages the window's low-res patch under that footprint in LDS (f32,
// [K][rows][cols]; the footprint of a x1.75 view is about 3x the tile, its patch a few KiB), and
// every thread adds the window's value at each of its taps the window covers, in table order, with
// headslide's arithmetic (bilerp / bilerp_depth, add_rounded, one rounded division by the count).
// The 4 taps are then interpolated with bilerp (a flipped view reads column W-1-x), so the K values
// of U_v are in registers for the softmax of the "probs" rule; the views are summed as in
// headensemble.hip.
//
// The window table (up to 1024 entries of 16 B) does not fit the kernel arguments: it lives behind
// the per-workgroup records in the call's workspace and is written there by small launches of the
// call itself, 128 entries of kernel arguments each (no hipMemcpy, no pinned memory: stream-ordered
// and capturable).  The view table travels by value.  Whether a tile skips a window depends on the
// tile alone: every thread reaches every barrier.  The scoring epilogue (seg_score with one pixel a
// thread, DepthSums), records, f64 partials and the one-workgroup folds are eval_tile.h's, as in
// headeval.hip: no global atomics, the grid a function of the shapes alone, two runs
// bitwise equal.  The depth kernel keeps headslide's thread-to-pixel map (8 x 128 tiles, 4 pixels a
// thread), so one plain view at the image's size reproduces its f64 sums bit for bit.
#include "eval_tile.h"

namespace {

constexpr int MAXV = DCLIP_ENSEMBLE_MAX_VIEWS;
constexpr int MAXW = DCLIP_SLIDE_TTA_MAX_WINDOWS;
constexpr int CHUNK = 128;  // table entries per writing launch (2 KiB of kernel arguments)
constexpr int TX = 32;      // threads along x (TH rows of them)

struct SView {
    int Hv, Wv, flip, wh, ww, h, w, first, nwin;
    int ident;       // (Hv, Wv) == (H, W): S_v is read as it is
    int nrow, ncol;  // the LDS patch of one window of this view under a tile's footprint
};
struct SViewTable {
    SView v[MAXV];
    int n;
};
struct WinChunk {
    dclip_window v[CHUNK];
};

__global__ __launch_bounds__(CHUNK) void table_kernel(WinChunk c, int n, dclip_window* __restrict__ dst) {
    const int i = threadIdx.x;
    if (i < n) dst[i] = c.v[i];
}

// tw = 32 px; the grid and the LDS bytes of the largest patch; fills every view's nrow / ncol
Tiling make_tiling(int B, int K, int px, SViewTable& vt, int H, int W) {
    Tiling t;
    t.tw = TX * px;
    t.lds = 0;
    for (int i = 0; i < vt.n; ++i) {
        SView& v = vt.v[i];
        // view rows (columns) under a tile, then low-res rows (columns) of one window under those
        int fr = v.ident ? TH : low_span(TH, v.Hv, H);
        int fc = v.ident ? t.tw : low_span(t.tw, v.Wv, W);
        fr = fr < v.wh ? fr : v.wh;
        fc = fc < v.ww ? fc : v.ww;
        v.nrow = low_span(fr, v.h, v.wh);
        v.ncol = low_span(fc, v.w, v.ww);
        const size_t bytes = (size_t)K * v.nrow * v.ncol * 4;
        t.lds = bytes > t.lds ? bytes : t.lds;
    }
    t.nrow = t.ncol = 0;  // per view, in the table
    finish_tiling(t, B, H, W);
    return t;
}

__device__ __forceinline__ Lerp lerp_same(int i) {
    Lerp r;
    r.i0 = r.i1 = i;
    r.l0 = 1.f;
    r.l1 = 0.f;
    return r;
}

// U[p][k]: view `vw` at the thread's PX pixels (y, x + p) of the tile at (y0, x0): its slide result,
// resized to H x W and mirrored back.  Workgroup-collective (barriers inside): every thread calls
// it; `active` threads get values.
template <typename TL, int K, int PX, bool DEPTH>
__device__ __forceinline__ void view_values(const SView& vw, const dclip_window* __restrict__ tab,
                                            float* __restrict__ low_s, int b, int y0, int x0, int tw, int H, int W,
                                            int y, int x, bool active, float (&U)[PX][K]) {
    const int y1 = y0 + TH - 1 < H ? y0 + TH - 1 : H - 1;
    const int x1 = x0 + tw - 1 < W ? x0 + tw - 1 : W - 1;
    const int xa = vw.flip ? W - 1 - x1 : x0, xb = vw.flip ? W - 1 - x0 : x1;
    // the tile's footprint in the view (workgroup-uniform)
    int fy0 = y0, fy1 = y1, fx0 = xa, fx1 = xb;
    if (!vw.ident) {
        fy0 = lerp_index(y0, vw.Hv, H).i0;
        fy1 = lerp_index(y1, vw.Hv, H).i1;
        fx0 = lerp_index(xa, vw.Wv, W).i0;
        fx1 = lerp_index(xb, vw.Wv, W).i1;
    }
    // the thread's taps: rows Y2.i0 / Y2.i1, columns X2[p].i0 / X2[p].i1; tap t = 2 row + column
    const int nt = vw.ident ? 1 : 2;
    const int yc = y < H ? y : H - 1;
    const Lerp Y2 = vw.ident ? lerp_same(yc) : lerp_index(yc, vw.Hv, H);
    Lerp X2[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        const int xp = x + p < W ? x + p : W - 1;
        const int xs = vw.flip ? W - 1 - xp : xp;
        X2[p] = vw.ident ? lerp_same(xs) : lerp_index(xs, vw.Wv, W);
    }
    float acc[PX][4][K];
    int cnt[PX][4];
#pragma unroll
    for (int p = 0; p < PX; ++p)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            cnt[p][t] = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) acc[p][t][k] = 0.f;
        }
    const int h = vw.h, w = vw.w, wh = vw.wh, ww = vw.ww;
    for (int iw = 0; iw < vw.nwin; ++iw) {
        const dclip_window wd = tab[vw.first + iw];
        const int wy = wd.y0, wx = wd.x0;
        const int ya = fy0 > wy ? fy0 : wy, yb = fy1 < wy + wh - 1 ? fy1 : wy + wh - 1;
        const int xl = fx0 > wx ? fx0 : wx, xr = fx1 < wx + ww - 1 ? fx1 : wx + ww - 1;
        if (ya > yb || xl > xr) continue;  // workgroup-uniform
        const int ilo = lerp_index(ya - wy, h, wh).i0, jlo = lerp_index(xl - wx, w, ww).i0;
        int nr = lerp_index(yb - wy, h, wh).i1 - ilo + 1, nc = lerp_index(xr - wx, w, ww).i1 - jlo + 1;
        nr = nr < vw.nrow ? nr : vw.nrow;  // low_span() bounds both; never index LDS past the patch
        nc = nc < vw.ncol ? nc : vw.ncol;
        __syncthreads();  // the previous patch's readers are done
        stage_patch(low_s, (const TL*)wd.low, b, K, h, w, ilo, nr, jlo, nc, vw.nrow, vw.ncol);
        __syncthreads();
        if (!active) continue;
        bool rc[2];
        Lerp Yw[2];
        int r0[2], r1[2];
#pragma unroll
        for (int ry = 0; ry < 2; ++ry) {
            const int vy = ry ? Y2.i1 : Y2.i0;
            rc[ry] = ry < nt && vy >= wy && vy < wy + wh;
            Yw[ry] = lerp_index(clampi(vy - wy, 0, wh - 1), h, wh);
            r0[ry] = clampi(Yw[ry].i0 - ilo, 0, nr - 1);
            r1[ry] = clampi(Yw[ry].i1 - ilo, 0, nr - 1);
        }
        if (!(rc[0] || rc[1])) continue;
#pragma unroll
        for (int p = 0; p < PX; ++p)
#pragma unroll
            for (int rx = 0; rx < 2; ++rx) {
                const int vx = rx ? X2[p].i1 : X2[p].i0;
                if (!(rx < nt && vx >= wx && vx < wx + ww)) continue;
                const Lerp Xw = lerp_index(vx - wx, w, ww);
                const int c0 = clampi(Xw.i0 - jlo, 0, nc - 1), c1 = clampi(Xw.i1 - jlo, 0, nc - 1);
                const int slot = (vx - wx) & 3;  // bilerp_depth's roundings follow the window-local column
#pragma unroll
                for (int ry = 0; ry < 2; ++ry) {
                    if (!rc[ry]) continue;
                    const int t = 2 * ry + rx;
                    ++cnt[p][t];
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const float* top = low_s + (k * vw.nrow + r0[ry]) * vw.ncol;
                        const float* bot = low_s + (k * vw.nrow + r1[ry]) * vw.ncol;
                        const float u = DEPTH ? bilerp_depth(slot, Yw[ry].l0, Yw[ry].l1, Xw.l0, Xw.l1, top[c0], top[c1],
                                                             bot[c0], bot[c1])
                                              : bilerp(Yw[ry].l0, Yw[ry].l1, Xw.l0, Xw.l1, top[c0], top[c1], bot[c0],
                                                       bot[c1]);
                        acc[p][t][k] = add_rounded(acc[p][t][k], u);
                    }
                }
            }
    }
#pragma unroll
    for (int p = 0; p < PX; ++p) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (cnt[p][t] > 1) {  // x / 1 is x
                const float c = (float)cnt[p][t];
#pragma unroll
                for (int k = 0; k < K; ++k) acc[p][t][k] = div_rounded(acc[p][t][k], c);
            }
#pragma unroll
        for (int k = 0; k < K; ++k)
            U[p][k] = vw.ident ? acc[p][0][k]
                               : bilerp(Y2.l0, Y2.l1, X2[p].l0, X2[p].l1, acc[p][0][k], acc[p][1][k], acc[p][2][k],
                                        acc[p][3][k]);
    }
}

// ----------------------------------------------------------------------------- segmentation
// One pixel per thread.  LAB: labels given (confusion matrix, CE sum, #valid); pred may be null then.
// PROBS: accumulate softmax(U_v) of every view instead of U_v.
template <typename TL, int K, bool LAB, bool PROBS>
__global__ __launch_bounds__(256) void slide_tta_seg_kernel(SViewTable vt, const dclip_window* __restrict__ tab, int H,
                                                            int W, Tiling tl, const void* __restrict__ lab, int lab_dt,
                                                            int ignore, uint8_t* __restrict__ pred,
                                                            char* __restrict__ ws) {
    extern __shared__ float low_s[];
    __shared__ unsigned hist_s[K * K + 1];
    __shared__ double red_s[4];
    const int tid = threadIdx.x;
    const int tx = tid % TX, ty = tid / TX;
    const float inv_v = 1.f / (float)vt.n;
    if constexpr (LAB) hist_clear<K>(hist_s);
    double lsum = 0.0;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto [b, y0, x0] = tile_origin(tile, tl);
        const int y = y0 + ty, x = x0 + tx;
        const bool active = y < H && x < W;  // every thread stages every patch
        float v[1][K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[0][k] = 0.f;
        for (int iv = 0; iv < vt.n; ++iv) {
            float u[1][K];
            view_values<TL, K, 1, false>(vt.v[iv], tab, low_s, b, y0, x0, tl.tw, H, W, y, x, active, u);
            if (!active) continue;
            if constexpr (!PROBS) {
#pragma unroll
                for (int k = 0; k < K; ++k) v[0][k] = add_rounded(v[0][k], u[0][k]);
            } else {
                float m = u[0][0];
#pragma unroll
                for (int k = 1; k < K; ++k) m = fmaxf(m, u[0][k]);
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    u[0][k] = __expf(u[0][k] - m);
                    s += u[0][k];
                }
                const float inv = 1.f / s;
#pragma unroll
                for (int k = 0; k < K; ++k) v[0][k] += u[0][k] * inv;
            }
        }
        if (!active) continue;
        const int64_t pix = ((int64_t)b * H + y) * W + x;
#pragma unroll
        for (int k = 0; k < K; ++k) v[0][k] *= inv_v;
        int t[4] = {-1, -1, -1, -1};
        if constexpr (LAB) load_labels4(lab, lab_dt, pix, 1, false, t);
        int am[1];
        seg_score<K, 1, LAB, PROBS>(v, t, 1, ignore, hist_s, lsum, am);
        if (pred != nullptr) pred[pix] = (uint8_t)am[0];
    }
    if constexpr (LAB) seg_flush<K>(hist_s, lsum, red_s, ws);
}

// ----------------------------------------------------------------------------- depth
// Four pixels per thread, as headslide.hip.  TGT: target given (the 12 sums); up may be null then.
template <typename TL, bool TGT>
__global__ __launch_bounds__(256) void slide_tta_depth_kernel(SViewTable vt, const dclip_window* __restrict__ tab,
                                                              int H, int W, Tiling tl, const float* __restrict__ gt,
                                                              const uint8_t* __restrict__ mask, float dmin, float dmax,
                                                              int clamp_pred, float eps, int vec,
                                                              float* __restrict__ up, char* __restrict__ ws) {
    extern __shared__ float low_s[];
    __shared__ double red_s[4 * NSUM];
    const int tid = threadIdx.x;
    const int tx = tid % TX, ty = tid / TX;
    const float inv_v = 1.f / (float)vt.n;
    DepthSums acc;
    for (int tile = blockIdx.x; tile < tl.ntiles; tile += gridDim.x) {
        const auto [b, y0, x0] = tile_origin(tile, tl);
        const int y = y0 + ty, x = x0 + 4 * tx;
        const bool active = y < H && x < W;
        float u[4] = {0.f, 0.f, 0.f, 0.f};
        for (int iv = 0; iv < vt.n; ++iv) {
            float r[4][1];
            view_values<TL, 1, 4, true>(vt.v[iv], tab, low_s, b, y0, x0, tl.tw, H, W, y, x, active, r);
            if (!active) continue;
#pragma unroll
            for (int p = 0; p < 4; ++p) u[p] = add_rounded(u[p], r[p][0]);
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

// the window table behind the K-class records of `ws`
dclip_window* table_of(void* ws, int K) { return (dclip_window*)((char*)ws + (int64_t)NWG_MAX * record_bytes(K)); }

void write_table(const dclip_window* wins, int nwin_total, dclip_window* tab, hipStream_t st) {
    for (int c = 0; c < nwin_total; c += CHUNK) {
        WinChunk ch;
        const int n = nwin_total - c < CHUNK ? nwin_total - c : CHUNK;
        for (int i = 0; i < CHUNK; ++i) ch.v[i] = i < n ? wins[c + i] : dclip_window{nullptr, 0, 0};
        table_kernel<<<1, CHUNK, 0, st>>>(ch, n, tab + c);
    }
}

template <typename TL, bool PROBS>
void launch_seg(const SViewTable& vt, const Tiling& tl, const dclip_window* tab, int H, int W, const void* lab,
                int lab_dt, int ignore, uint8_t* pred, int64_t* cm, double* loss_sum, unsigned long long* count,
                void* ws, hipStream_t st) {
    constexpr int K = 19;
    if (lab != nullptr) {
        slide_tta_seg_kernel<TL, K, true, PROBS><<<tl.nwg, 256, tl.lds, st>>>(vt, tab, H, W, tl, lab, lab_dt, ignore,
                                                                              pred, (char*)ws);
        eval_seg_fold_kernel<<<1, 256, 0, st>>>((const char*)ws, tl.nwg, K, cm, loss_sum, count);
    } else {
        slide_tta_seg_kernel<TL, K, false, PROBS><<<tl.nwg, 256, tl.lds, st>>>(vt, tab, H, W, tl, nullptr, 0, ignore,
                                                                               pred, (char*)ws);
    }
}

template <typename TL>
void launch_depth(const SViewTable& vt, const Tiling& tl, const dclip_window* tab, int H, int W, const float* gt,
                  const uint8_t* mask, float dmin, float dmax, int clamp_pred, float eps, float* up, double* sums,
                  void* ws, hipStream_t st) {
    const int vec = depth_aligned(gt, mask, up, W);
    if (gt != nullptr) {
        slide_tta_depth_kernel<TL, true><<<tl.nwg, 256, tl.lds, st>>>(vt, tab, H, W, tl, gt, mask, dmin, dmax,
                                                                      clamp_pred, eps, vec, up, (char*)ws);
        eval_depth_fold_kernel<<<1, 256, 0, st>>>((const char*)ws, tl.nwg, sums);
    } else {
        slide_tta_depth_kernel<TL, false><<<tl.nwg, 256, tl.lds, st>>>(vt, tab, H, W, tl, nullptr, nullptr, dmin, dmax,
                                                                       clamp_pred, eps, vec, up, (char*)ws);
    }
}

// The checks shared by both entry points, before any launch; fills the kernel's view table and tiling.
int check_tables(const char* name, int low_dt, const dclip_slide_view* views, int nviews, const dclip_window* wins,
                 int nwin_total, int B, int K, int px, int H, int W, const void* ws, SViewTable& vt, Tiling& tl) {
    DCLIP_HOST_CHECK(nviews >= 1 && nviews <= MAXV, "%s: nviews=%d (1 .. %d views)", name, nviews, MAXV);
    DCLIP_HOST_CHECK(nwin_total >= 1 && nwin_total <= MAXW, "%s: nwin_total=%d (1 .. %d windows over all views)", name,
                     nwin_total, MAXW);
    DCLIP_HOST_CHECK(views != nullptr, "%s: views required", name);
    DCLIP_HOST_CHECK(wins != nullptr, "%s: wins required", name);
    DCLIP_HOST_CHECK(B > 0 && H > 0 && W > 0, "%s: bad sizes (B=%d, H=%d, W=%d)", name, B, H, W);
    DCLIP_HOST_CHECK(low_dt == DCLIP_F32 || low_dt == DCLIP_F16 || low_dt == DCLIP_BF16,
                     "%s: low_dt=%d (f32, f16 or bf16)", name, low_dt);
    DCLIP_HOST_CHECK((int64_t)B * H * W < ((int64_t)1 << 31), "%s: B*H*W = %lld pixels (must be below 2^31)", name,
                     (long long)((int64_t)B * H * W));
    vt.n = nviews;
    for (int i = 0; i < MAXV; ++i) vt.v[i] = SView{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < nviews; ++i) {
        const dclip_slide_view& v = views[i];
        DCLIP_HOST_CHECK(v.Hv > 0 && v.Wv > 0 && v.h > 0 && v.w > 0, "%s: view %d: bad sizes (Hv=%d, Wv=%d, h=%d, w=%d)",
                         name, i, v.Hv, v.Wv, v.h, v.w);
        DCLIP_HOST_CHECK(v.flip == 0 || v.flip == 1, "%s: view %d: flip=%d (0 or 1)", name, i, v.flip);
        DCLIP_HOST_CHECK(v.h <= v.wh && v.wh <= v.Hv, "%s: view %d: h=%d <= wh=%d <= Hv=%d required (window rows)", name,
                         i, v.h, v.wh, v.Hv);
        DCLIP_HOST_CHECK(v.w <= v.ww && v.ww <= v.Wv, "%s: view %d: w=%d <= ww=%d <= Wv=%d required (window columns)",
                         name, i, v.w, v.ww, v.Wv);
        DCLIP_HOST_CHECK((int64_t)B * v.Hv * v.Wv < ((int64_t)1 << 31),
                         "%s: view %d: B*Hv*Wv = %lld pixels (must be below 2^31)", name, i,
                         (long long)((int64_t)B * v.Hv * v.Wv));
        DCLIP_HOST_CHECK(v.nwin >= 1 && v.first >= 0 && (int64_t)v.first + v.nwin <= nwin_total,
                         "%s: view %d: windows [%d, %d + %d) outside the table of %d", name, i, v.first, v.first, v.nwin,
                         nwin_total);
        for (int j = v.first; j < v.first + v.nwin; ++j) {
            const dclip_window& wd = wins[j];
            DCLIP_HOST_CHECK(wd.low != nullptr, "%s: view %d: window %d: low is null", name, i, j);
            DCLIP_HOST_CHECK(wd.y0 >= 0 && wd.y0 <= v.Hv - v.wh,
                             "%s: view %d: window %d: y0=%d (0 <= y0, y0 + wh=%d <= Hv=%d)", name, i, j, wd.y0, v.wh,
                             v.Hv);
            DCLIP_HOST_CHECK(wd.x0 >= 0 && wd.x0 <= v.Wv - v.ww,
                             "%s: view %d: window %d: x0=%d (0 <= x0, x0 + ww=%d <= Wv=%d)", name, i, j, wd.x0, v.ww,
                             v.Wv);
        }
        int uy = 0, ux = 0;
        DCLIP_HOST_CHECK(!first_uncovered(wins + v.first, v.nwin, v.wh, v.ww, v.Hv, v.Wv, &uy, &ux),
                         "%s: view %d: pixel (y=%d, x=%d) is covered by no window", name, i, uy, ux);
        vt.v[i] = SView{v.Hv, v.Wv, v.flip, v.wh, v.ww, v.h, v.w, v.first, v.nwin, v.Hv == H && v.Wv == W, 0, 0};
    }
    tl = make_tiling(B, K, px, vt, H, W);
    DCLIP_HOST_CHECK(tl.lds <= (size_t)LDS_TILE_MAX,
                     "%s: a window's low-res patch under one output tile takes %lld bytes of LDS (at most %d): the view "
                     "is too large for the image", name, (long long)tl.lds, LDS_TILE_MAX);
    DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 8) == 0,
                     "%s: ws=%p (dclip_slide_tta_eval_ws_bytes(B, K, nviews, nwin_total) bytes, 8-byte aligned) "
                     "required: it holds the window table", name, ws);
    return 0;
}

}  // namespace

extern "C" int64_t dclip_slide_tta_eval_ws_bytes(int B, int K, int nviews, int nwin_total) {
    if (B <= 0 || K <= 0 || nviews <= 0 || nviews > MAXV || nwin_total <= 0 || nwin_total > MAXW) return 0;
    return (int64_t)NWG_MAX * record_bytes(K) + (int64_t)nwin_total * (int64_t)sizeof(dclip_window);
}

extern "C" int dclip_slide_tta_eval_seg(int low_dt, const dclip_slide_view* views, int nviews, const dclip_window* wins,
                                        int nwin_total, int B, int K, int average, const void* labels, int lab_dt,
                                        int H, int W, int ignore_index, uint8_t* pred, int64_t* cm, double* loss_sum,
                                        unsigned long long* count, void* ws, void* stream) {
    DCLIP_HOST_CHECK(K == 19, "dclip_slide_tta_eval_seg: K=%d (built for the 19 Cityscapes classes)", K);
    DCLIP_HOST_CHECK(average == 0 || average == 1,
                     "dclip_slide_tta_eval_seg: average=%d (0: mean of the logits, 1: mean of the probabilities)",
                     average);
    SViewTable vt;
    Tiling tl;
    if (int rc = check_tables("dclip_slide_tta_eval_seg", low_dt, views, nviews, wins, nwin_total, B, K, 1, H, W, ws, vt,
                              tl))
        return rc;
    if (int rc = check_seg_outputs("dclip_slide_tta_eval_seg", labels, lab_dt, pred, cm, loss_sum, count)) return rc;
    hipStream_t st = (hipStream_t)stream;
    dclip_window* tab = table_of(ws, K);
    write_table(wins, nwin_total, tab, st);
    EVAL_DISPATCH_LOW(low_dt, (average ? launch_seg<TL, true> : launch_seg<TL, false>)(
                                  vt, tl, tab, H, W, labels, lab_dt, ignore_index, pred, cm, loss_sum, count, ws, st));
    DCLIP_LAUNCH_CHECK();
    return 0;
}

extern "C" int dclip_slide_tta_eval_depth(int low_dt, const dclip_slide_view* views, int nviews,
                                          const dclip_window* wins, int nwin_total, int B, const float* target,
                                          const uint8_t* mask, int H, int W, float min_depth, float max_depth,
                                          int clamp_pred, float eps, float* up, double* sums, void* ws, void* stream) {
    SViewTable vt;
    Tiling tl;
    if (int rc = check_tables("dclip_slide_tta_eval_depth", low_dt, views, nviews, wins, nwin_total, B, 1, 4, H, W, ws,
                              vt, tl))
        return rc;
    if (int rc = check_depth_outputs("dclip_slide_tta_eval_depth", target, sums, up)) return rc;
    hipStream_t st = (hipStream_t)stream;
    dclip_window* tab = table_of(ws, 1);
    write_table(wins, nwin_total, tab, st);
    EVAL_DISPATCH_LOW(low_dt, launch_depth<TL>(vt, tl, tab, H, W, target, mask, min_depth, max_depth, clamp_pred, eps, up,
                                               sums, ws, st));
    DCLIP_LAUNCH_CHECK();
    return 0;
}
