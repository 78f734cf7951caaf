// ADE20K batch preparation on the GPU (the reference's datasets/ade20k.py:57-185 per sample).
//
// The host uploads the decoded planes of B samples of ANY sizes as one packed uint8 buffer of RGB
// images and one of label planes, and a geometry table (DCLIP_ADE_GEOM_WORDS int64 per image: the
// planes' byte offsets, the sizes of the source and of both resizes, the crop origin, the flip).
// The kernels then run, per image,
//   * PIL's 8-bit BILINEAR resize, up to twice (the random scale, then the resize up to the crop when
//     a side fell below it): separable, the horizontal pass first, every pass rounding to uint8
//     (so the passes cannot be merged), a pass between equal sizes skipped;
//   * PIL's NEAREST resize of the labels through the same two sizes, as one composed index table per
//     axis (source index int(xo), xo accumulated serially by one add per output coordinate);
//   * the crop, the optional mirror, the label map (v > 0 -> v - 1, 0 -> ignore) and
//     float32(u8) / 255 -> (. - mean) / std in f64 -> CHW.
// Only what the crop window needs is computed: the window's rows / columns are walked back through
// the bounds [xmin, xmin + n) of each pass down to the source (ade_plan), and each pass fills just
// that region of its uint8 intermediate.
//
// Launches (all on the caller's stream, no host synchronisation, no device -> host copy):
//   ade_plan_kernel   per (image, pass, output coordinate): bounds and 22-bit integer coefficients, f64 with
//                     no contraction, Pillow's operation order; per (image, axis): the composed nearest table
//   ade_pass_kernel   one launch per pass that any image needs (at most four): one thread per pixel
//   ade_emit_kernel   crop, flip, label gather + map, normalisation, CHW store
// ade_plan() is one function compiled for both sides: the host runs it on its copy of the table to
// validate every entry and to size the grids and the workspace; every workgroup runs it on the
// device copy and leaves at once when that copy does not pass the same checks (limits of the
// packed buffers and of the per-image workspace slice included), so no table value can index
// outside a buffer even if the two copies disagree.  Integer arithmetic, fixed accumulation order,
// no atomics: two runs are bitwise equal.
#include "common.h"

#include <math.h>

namespace {

constexpr int GW = DCLIP_ADE_GEOM_WORDS;
constexpr int ADE_MAX_SIDE = 1 << 14;  // of the source and of both resizes: pixel offsets of a plane stay in int32
constexpr int ADE_MAX_TAPS = 131;      // ksize = 2 ceil(max(in / out, 1)) + 1: a pass may shrink by up to 65x
constexpr int PRECISION_BITS = 22;

// Pillow's precompute_coeffs for BILINEAR (support 1): the source range [xmin, xmin + n) of output xx
__host__ __device__ inline void ade_bounds(int inS, int outS, int xx, int& xmin, int& n) {
#pragma clang fp contract(off)
    const double scale = (double)inS / (double)outS;
    const double support = scale < 1.0 ? 1.0 : scale;
    const double center = (xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > inS) hi = inS;
    xmin = lo;
    n = hi - lo;
}

__host__ __device__ inline int ade_ksize(int inS, int outS) {
    const double scale = (double)inS / (double)outS;
    return (int)ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
}

// a uint8 RGB region: pixel (r, c) of the stage's image at base + off + ((r - r0) pitch + (c - c0)) 3
struct AdeView {
    int64_t off;   // bytes from the packed image buffer (ws == 0) or from the image's workspace slice
    int ws;
    int pitch, r0, c0, nr, nc;
};

struct AdePass {
    int skip;            // equal sizes: the output view is the input view
    int inS, outS;       // of the pass's axis (0, 2: columns; 1, 3: rows)
    int lo, cnt;         // output coordinates [lo, lo + cnt) the later stages need
    int ksize;           // coefficient row: xmin, n, k[ksize]
    int64_t tab_off;     // bytes into the workspace slice
};

struct AdePlan {
    AdeView view[5];     // 0: the source; p + 1: after pass p
    AdePass pass[4];     // 0: W0 -> W1, 1: H0 -> H1, 2: W1 -> W2, 3: H1 -> H2
    int64_t img_off, lab_off, ytab_off, xtab_off, need;  // need: bytes of the workspace slice
    int H0, W0, H1, W1, H2, W2, y0, x0, flip;
};

struct AdeLimits {
    int64_t img_bytes, lab_bytes, ws_stride;  // ws_stride: bytes of one image's workspace slice
};

__host__ __device__ inline int64_t ade_align(int64_t v) { return (v + 15) & ~(int64_t)15; }

// The plan of one image from its geometry row; nullptr when it is valid, else what is wrong with it.
// lim: every extent is checked against it (ws_stride < 0: the slice is being sized, not checked).
__host__ __device__ inline const char* ade_plan(const int64_t* g, int h, int w, const AdeLimits& lim, AdePlan& P) {
    for (int i = 2; i < 8; ++i)
        if (g[i] < 1 || g[i] > ADE_MAX_SIDE) return "a side of the source or of a resize is below 1 or above 16384";
    P.img_off = g[0], P.lab_off = g[1];
    P.H0 = (int)g[2], P.W0 = (int)g[3], P.H1 = (int)g[4], P.W1 = (int)g[5], P.H2 = (int)g[6], P.W2 = (int)g[7];
    const int64_t px = (int64_t)P.H0 * P.W0;
    if (g[0] < 0 || g[0] > lim.img_bytes || px * 3 > lim.img_bytes - g[0]) return "image plane outside the packed image buffer";
    if (g[1] < 0 || g[1] > lim.lab_bytes || px > lim.lab_bytes - g[1]) return "label plane outside the packed label buffer";
    if (g[8] < 0 || g[9] < 0 || g[8] > P.H2 - h || g[9] > P.W2 - w) return "crop window outside the resized image";
    P.y0 = (int)g[8], P.x0 = (int)g[9], P.flip = g[10] != 0;
    const int inS[4] = {P.W0, P.H0, P.W1, P.H1}, outS[4] = {P.W1, P.H1, P.W2, P.H2};
    // backwards: the rows / columns each stage must hold
    int r0 = P.y0, nr = h, c0 = P.x0, nc = w;
    int R0[5], NR[5], C0[5], NC[5];
    R0[4] = r0, NR[4] = nr, C0[4] = c0, NC[4] = nc;
    for (int p = 3; p >= 0; --p) {
        AdePass& q = P.pass[p];
        q.inS = inS[p], q.outS = outS[p], q.skip = inS[p] == outS[p];
        q.ksize = ade_ksize(inS[p], outS[p]);
        if (q.ksize > ADE_MAX_TAPS) return "a resize shrinks a side by more than 65x";
        int& o0 = (p & 1) ? r0 : c0;
        int& on = (p & 1) ? nr : nc;
        q.lo = o0, q.cnt = on;
        if (!q.skip) {
            int a, na, b, nb;
            ade_bounds(q.inS, q.outS, o0, a, na);
            ade_bounds(q.inS, q.outS, o0 + on - 1, b, nb);
            if (na < 1 || nb < 1 || b < a || b + nb > q.inS) return "empty filter support";
            o0 = a, on = b + nb - a;
        }
        R0[p] = r0, NR[p] = nr, C0[p] = c0, NC[p] = nc;
    }
    // forwards: the workspace slice — coefficient tables, nearest tables, then the uint8 regions
    int64_t at = 0;
    for (int p = 0; p < 4; ++p) {
        P.pass[p].tab_off = at;
        if (!P.pass[p].skip) at = ade_align(at + (int64_t)P.pass[p].cnt * (2 + P.pass[p].ksize) * 4);
    }
    P.ytab_off = at, at = ade_align(at + (int64_t)h * 4);
    P.xtab_off = at, at = ade_align(at + (int64_t)w * 4);
    P.view[0] = AdeView{P.img_off, 0, P.W0, 0, 0, P.H0, P.W0};
    for (int p = 0; p < 4; ++p) {
        if (P.pass[p].skip) {
            P.view[p + 1] = P.view[p];
            continue;
        }
        P.view[p + 1] = AdeView{at, 1, NC[p + 1], R0[p + 1], C0[p + 1], NR[p + 1], NC[p + 1]};
        at = ade_align(at + (int64_t)NR[p + 1] * NC[p + 1] * 3);
    }
    P.need = at;
    if (lim.ws_stride >= 0 && at > lim.ws_stride) return "workspace slice too small";
    // every later stage's region lies inside the one before it (the walk above made it so; a view of a
    // skipped pass is the larger region of an earlier stage)
    for (int p = 0; p <= 4; ++p) {
        const AdeView& v = P.view[p];
        if (R0[p] < v.r0 || R0[p] + NR[p] > v.r0 + v.nr || C0[p] < v.c0 || C0[p] + NC[p] > v.c0 + v.nc)
            return "a stage's region leaves the stage before it";
    }
    return nullptr;
}

__device__ __forceinline__ bool ade_block_plan(const int64_t* __restrict__ geom, int h, int w, const AdeLimits& lim,
                                               AdePlan& P, int& ok) {
    if (threadIdx.x == 0) ok = ade_plan(geom + (int64_t)blockIdx.y * GW, h, w, lim, P) == nullptr;
    __syncthreads();
    return ok != 0;
}

// coefficient row of output coordinate xx of a pass: xmin, n, then n 22-bit integers (Pillow's
// precompute_coeffs + normalize_coeffs_8bpc, every operation in f64 in its order)
__device__ void ade_coeffs(const AdePass& q, int xx, int* __restrict__ row) {
#pragma clang fp contract(off)
    const double scale = (double)q.inS / (double)q.outS;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / fs;
    int xmin, n;
    ade_bounds(q.inS, q.outS, xx, xmin, n);
    n = min(max(n, 0), q.ksize);
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        double v = (x + xmin - center + 0.5) * ss;
        if (v < 0.0) v = -v;
        ww += v < 1.0 ? 1.0 - v : 0.0;
    }
    row[0] = xmin;
    row[1] = n;
    for (int x = 0; x < n; ++x) {
        double v = (x + xmin - center + 0.5) * ss;
        if (v < 0.0) v = -v;
        double k = v < 1.0 ? 1.0 - v : 0.0;
        if (ww != 0.0) k /= ww;
        row[2 + x] = k < 0.0 ? (int)(-0.5 + k * (double)(1 << PRECISION_BITS)) : (int)(0.5 + k * (double)(1 << PRECISION_BITS));
    }
}

// composed NEAREST table of one axis: out[j] = tab1[tab2[o0 + j]], tab(in -> out)[x] = int(xo), xo = a / 2 + x adds
// of a = in / out, accumulated serially as Pillow's ImagingScaleAffine does (both tables are non-decreasing, so one
// cursor walks tab1 while j walks tab2); an identity resize accumulates 0.5 + 1 + 1 ... exactly
__device__ void ade_nearest(int S0, int S1, int S2, int o0, int cnt, int* __restrict__ out) {
#pragma clang fp contract(off)
    const double a1 = (double)S0 / (double)S1, a2 = (double)S1 / (double)S2;
    double x1 = a1 * 0.5, x2 = a2 * 0.5;
    int i = 0;
    for (int j = 0; j < o0 + cnt; ++j) {
        const int t2 = min((int)x2, S1 - 1);
        x2 += a2;
        while (i < t2) {
            x1 += a1;
            ++i;
        }
        if (j >= o0) out[j - o0] = min(max((int)x1, 0), S0 - 1);
    }
}

__global__ __launch_bounds__(256) void ade_plan_kernel(const int64_t* __restrict__ geom, int h, int w, AdeLimits lim,
                                                       uint8_t* __restrict__ ws) {
    __shared__ AdePlan P;
    __shared__ int ok;
    if (!ade_block_plan(geom, h, w, lim, P, ok)) return;
    uint8_t* slice = ws + (int64_t)blockIdx.y * lim.ws_stride;
    // items 0, 1: the nearest tables (serial); then one item per coefficient row of the passes in order
    const int n0 = P.pass[0].skip ? 0 : P.pass[0].cnt, n1 = P.pass[1].skip ? 0 : P.pass[1].cnt;
    const int n2 = P.pass[2].skip ? 0 : P.pass[2].cnt, n3 = P.pass[3].skip ? 0 : P.pass[3].cnt;
    const int items = 2 + n0 + n1 + n2 + n3;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < items; i += gridDim.x * blockDim.x) {
        if (i == 0) {
            ade_nearest(P.H0, P.H1, P.H2, P.y0, h, (int*)(slice + P.ytab_off));
        } else if (i == 1) {
            ade_nearest(P.W0, P.W1, P.W2, P.x0, w, (int*)(slice + P.xtab_off));
        } else {
            int e = i - 2, p = 0;
            if (e >= n0) { e -= n0; p = 1;
                if (e >= n1) { e -= n1; p = 2;
                    if (e >= n2) { e -= n2; p = 3; } } }
            const AdePass& q = P.pass[p];
            ade_coeffs(q, q.lo + e, (int*)(slice + q.tab_off) + (int64_t)e * (2 + q.ksize));
        }
    }
}

__device__ __forceinline__ const uint8_t* ade_view_base(const AdeView& v, const uint8_t* img, const uint8_t* slice) {
    return (v.ws ? slice : img) + v.off;
}

__global__ __launch_bounds__(256) void ade_pass_kernel(const uint8_t* __restrict__ img, const int64_t* __restrict__ geom,
                                                       int h, int w, AdeLimits lim, uint8_t* __restrict__ ws, int p) {
    __shared__ AdePlan P;
    __shared__ int ok;
    if (!ade_block_plan(geom, h, w, lim, P, ok) || P.pass[p].skip) return;
    uint8_t* slice = ws + (int64_t)blockIdx.y * lim.ws_stride;
    const AdePass& q = P.pass[p];
    const AdeView &in = P.view[p], &out = P.view[p + 1];
    const uint8_t* src = ade_view_base(in, img, slice);
    uint8_t* dst = slice + out.off;
    const int* tab = (const int*)(slice + q.tab_off);
    const int stride = 2 + q.ksize;
    const bool rows = p & 1;
    const int total = out.nr * out.nc;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int r = i / out.nc, c = i - r * out.nc;
        const int* t = tab + (int64_t)(rows ? r : c) * stride;
        const int xmin = t[0], n = t[1];
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
        // source pixel of tap k: along the pass's axis xmin + k, the other coordinate unchanged; clamped into
        // the input region (ade_plan made the region cover every tap: the clamp never moves an index)
        const int fr = rows ? xmin - in.r0 : out.r0 + r - in.r0;
        const int fc = rows ? out.c0 + c - in.c0 : xmin - in.c0;
        for (int k = 0; k < n; ++k) {
            const int rr = min(max(rows ? fr + k : fr, 0), in.nr - 1);
            const int cc = min(max(rows ? fc : fc + k, 0), in.nc - 1);
            const uint8_t* s = src + ((int64_t)rr * in.pitch + cc) * 3;
            const int kk = t[2 + k];
            a0 += (int)s[0] * kk;
            a1 += (int)s[1] * kk;
            a2 += (int)s[2] * kk;
        }
        uint8_t* d = dst + ((int64_t)r * out.pitch + c) * 3;
        d[0] = (uint8_t)min(max(a0 >> PRECISION_BITS, 0), 255);
        d[1] = (uint8_t)min(max(a1 >> PRECISION_BITS, 0), 255);
        d[2] = (uint8_t)min(max(a2 >> PRECISION_BITS, 0), 255);
    }
}

struct AdeNorm {
    double mean[3], stdv[3];
};

// RAW: TO = uint8_t, the crop's pixels as they are (the stage before the normalisation)
template <typename TO, bool RAW>
__global__ __launch_bounds__(256) void ade_emit_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                                       const int64_t* __restrict__ geom, int h, int w, AdeLimits lim,
                                                       const uint8_t* __restrict__ ws, AdeNorm nm, int ignore_label,
                                                       TO* __restrict__ out_img, int64_t* __restrict__ out_seg) {
#pragma clang fp contract(off)
    __shared__ AdePlan P;
    __shared__ int ok;
    if (!ade_block_plan(geom, h, w, lim, P, ok)) return;
    const uint8_t* slice = ws + (int64_t)blockIdx.y * lim.ws_stride;
    const AdeView& v = P.view[4];
    const uint8_t* src = ade_view_base(v, img, slice);
    const int* ytab = (const int*)(slice + P.ytab_off);
    const int* xtab = (const int*)(slice + P.xtab_off);
    const uint8_t* lb = lab + P.lab_off;
    const int64_t plane = (int64_t)h * w;
    TO* oi = out_img + (int64_t)blockIdx.y * 3 * plane;
    int64_t* os = out_seg + (int64_t)blockIdx.y * plane;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < h * w; i += gridDim.x * blockDim.x) {
        const int y = i / w, x = i - y * w;
        const int xs = P.flip ? w - 1 - x : x;
        const int rr = min(max(P.y0 + y - v.r0, 0), v.nr - 1), cc = min(max(P.x0 + xs - v.c0, 0), v.nc - 1);
        const uint8_t* s = src + ((int64_t)rr * v.pitch + cc) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if (RAW) {
                oi[ch * plane + i] = (TO)s[ch];
            } else {
                const float f = (float)s[ch] / 255.0f;  // the reference's float32 array / 255.0
                oi[ch * plane + i] = (TO)(float)(((double)f - nm.mean[ch]) / nm.stdv[ch]);
            }
        }
        const int l = lb[(int64_t)ytab[y] * P.W0 + xtab[xs]];
        os[i] = ignore_label < 0 ? l : (l > 0 ? l - 1 : ignore_label);
    }
}

// host: every image's plan checked against the limits; the largest slice and per-kernel work over the batch
struct AdeBatch {
    int64_t need;       // bytes of the largest workspace slice
    int plan_items;     // most items of the planning launch
    int pass_px[4];     // most pixels a pass writes (0: no image needs the pass)
};

const char* ade_check_batch(const int64_t* geom_host, int B, int h, int w, const AdeLimits& lim, AdeBatch& bt, int& bad) {
    bt = AdeBatch{0, 2, {0, 0, 0, 0}};
    for (int b = 0; b < B; ++b) {
        AdePlan P;
        const char* e = ade_plan(geom_host + (int64_t)b * GW, h, w, lim, P);
        if (e) {
            bad = b;
            return e;
        }
        bt.need = P.need > bt.need ? P.need : bt.need;
        int items = 2;
        for (int p = 0; p < 4; ++p) {
            if (P.pass[p].skip) continue;
            items += P.pass[p].cnt;
            const int px = P.view[p + 1].nr * P.view[p + 1].nc;
            bt.pass_px[p] = px > bt.pass_px[p] ? px : bt.pass_px[p];
        }
        bt.plan_items = items > bt.plan_items ? items : bt.plan_items;
    }
    return nullptr;
}

}  // namespace

extern "C" int64_t dclip_ade20k_prepare_ws_bytes(const int64_t* geom_host, int B, int h, int w) {
    if (!geom_host || B < 1 || h < 1 || w < 1 || h > ADE_MAX_SIDE || w > ADE_MAX_SIDE) {
        dclip_set_error("dclip_ade20k_prepare_ws_bytes: bad arguments B=%d crop %dx%d", B, h, w);
        return -1;
    }
    const AdeLimits lim{INT64_MAX, INT64_MAX, -1};
    AdeBatch bt;
    int bad = -1;
    const char* e = ade_check_batch(geom_host, B, h, w, lim, bt, bad);
    if (e) {
        dclip_set_error("dclip_ade20k_prepare_ws_bytes: image %d: %s", bad, e);
        return -1;
    }
    return bt.need * B;
}

extern "C" int dclip_ade20k_prepare(const uint8_t* img, int64_t img_bytes, const uint8_t* lab, int64_t lab_bytes,
                                    const int64_t* geom, const int64_t* geom_host, int B, int h, int w,
                                    const double* mean, const double* stdv, int ignore_label, void* out_img,
                                    int out_dt, int64_t* out_seg, void* ws, int64_t ws_bytes, void* stream) {
    DCLIP_HOST_CHECK(B > 0 && h > 0 && w > 0 && h <= ADE_MAX_SIDE && w <= ADE_MAX_SIDE,
                     "dclip_ade20k_prepare: bad sizes B=%d crop %dx%d", B, h, w);
    DCLIP_HOST_CHECK(img && lab && geom && geom_host && mean && stdv && out_img && out_seg && ws,
                     "dclip_ade20k_prepare: null pointer");
    DCLIP_HOST_CHECK(img_bytes > 0 && lab_bytes > 0 && ws_bytes > 0, "dclip_ade20k_prepare: empty buffer");
    DCLIP_HOST_CHECK(out_dt == DCLIP_F32 || out_dt == DCLIP_BF16 || out_dt == DCLIP_F16 || out_dt == DCLIP_U8,
                     "dclip_ade20k_prepare: out_dt must be F32, BF16, F16 or U8 (the crop before normalisation)");
    DCLIP_HOST_CHECK(ignore_label <= 255, "dclip_ade20k_prepare: ignore_label must be below 256 (negative: labels "
                     "unchanged)");
    for (int c = 0; c < 3; ++c)
        DCLIP_HOST_CHECK(stdv[c] != 0.0 && mean[c] == mean[c] && stdv[c] == stdv[c], "dclip_ade20k_prepare: bad mean / std");
    AdeLimits lim{img_bytes, lab_bytes, -1};
    AdeBatch bt;
    int bad = -1;
    const char* e = ade_check_batch(geom_host, B, h, w, lim, bt, bad);
    DCLIP_HOST_CHECK(!e, "dclip_ade20k_prepare: image %d: %s", bad, e);
    DCLIP_HOST_CHECK(bt.need * B <= ws_bytes, "dclip_ade20k_prepare: workspace of %lld bytes, %lld needed "
                     "(dclip_ade20k_prepare_ws_bytes)", (long long)ws_bytes, (long long)(bt.need * B));
    lim.ws_stride = bt.need;
    hipStream_t st = (hipStream_t)stream;
    const auto blocks = [](int64_t items) { return (unsigned)((items + 255) / 256 > 4096 ? 4096 : (items + 255) / 256); };
    ade_plan_kernel<<<dim3(blocks(bt.plan_items), B), 256, 0, st>>>(geom, h, w, lim, (uint8_t*)ws);
    for (int p = 0; p < 4; ++p)
        if (bt.pass_px[p] > 0)
            ade_pass_kernel<<<dim3(blocks(bt.pass_px[p]), B), 256, 0, st>>>(img, geom, h, w, lim, (uint8_t*)ws, p);
    AdeNorm nm;
    for (int c = 0; c < 3; ++c) nm.mean[c] = mean[c], nm.stdv[c] = stdv[c];
    const dim3 grid(blocks((int64_t)h * w), B);
#define DCLIP_ADE_EMIT(TO, RAW)                                                                                      \
    ade_emit_kernel<TO, RAW><<<grid, 256, 0, st>>>(img, lab, geom, h, w, lim, (const uint8_t*)ws, nm, ignore_label, \
                                                   (TO*)out_img, out_seg)
    if (out_dt == DCLIP_F32) DCLIP_ADE_EMIT(float, false);
    else if (out_dt == DCLIP_BF16) DCLIP_ADE_EMIT(bf16, false);
    else if (out_dt == DCLIP_F16) DCLIP_ADE_EMIT(f16, false);
    else DCLIP_ADE_EMIT(uint8_t, true);
#undef DCLIP_ADE_EMIT
    DCLIP_LAUNCH_CHECK();
    return 0;
}
