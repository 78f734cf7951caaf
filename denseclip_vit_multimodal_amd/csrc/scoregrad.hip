// Backward of the pixel-text score map (dclip_score_map / dclip_score_map_classes) for every class
// count 1 <= K <= DCLIP_CLASSES_MAX:  s[b,k,p] = <v_p / max(|v_p|, eps), t_k / max(|t_k|, eps)>.
//
//   rv = 1 / max(|v_p|, eps), vn = v rv        rt = 1 / max(|t_k|, eps), tn = t rt
//   dvn_p = sum_k ds[k,p] tn_k                 dtn_k = sum_p ds[k,p] vn_p
//   dv_p = rv (dvn_p - a_p vn_p <vn_p, dvn_p>) dt_k = rt (dtn_k - a_k tn_k <tn_k, dtn_k>)
//   a = 1 where the norm is >= eps, 0 where the clamp is active (autograd of F.normalize).
//
// Rounding points: none to 16 bits before the outputs.  v is read as 16-bit and widened exactly; the two
// products over the classes and the pixels (dvn, dtn) are f32 FMAs on the VALU over f32 tn, vn and ds; the
// norms, rv / rt and the projection dvn - a vn <vn, dvn> (a difference of two terms that nearly cancel, where
// an f32 rv would cost several ulps of the larger one) are f64, a few operations per element; dv is rounded
// once, on its store, to f32 or 16 bits.  No MFMA: an MFMA form would round tn, vn and ds to 16 bits, and at
// K = 19 the two products are 2.5 GFLOP.  (tests/score_loss_ref.py's emulation is therefore the same sequence
// evaluated in f32.)  Measured: 0.25 ms at 8 x 8192 x 512, K = 19, which is 0.54 TB/s of v + dv:
// the pass is issue- and L2-bound, not HBM-bound (tn re-read from L2 per pixel group, one v_readlane per 8
// FMAs, v read a second time by phase B); at K = 150, 1.17 ms, slower than two f32 library GEMMs.
//
// Three launches, every grid a function of (B, HW, C, K) alone, no float atomics, fixed orders:
//   1. score_bwd_text_kernel   one workgroup per (b, k): tn_k into the workspace.
//   2. score_bwd_kernel        one workgroup (4 waves) per image and span of SPAN = 256 pixels.
//        phase A (dv): a wave takes PB = 8 / NSLAB pixels at a time (NSLAB = slabs of 512 channels,
//          a lane owns one 8-channel chunk per slab), holds their dvn in registers and walks
//          the classes 64 / PB at a time: the lanes load that block of ds (scale folded in) one value
//          each, and every value is broadcast by v_readlane; tn rows come from the workspace (L2).
//          The rows themselves are loaded after the class loop, for the norms and the projection.
//          Registers: 64 f32 of dvn + 8 NSLAB of tn in the loop, + 32 of packed rows after it, whatever K is.
//        phase B (dt partials): the classes in chunks of CK = 16; the span's ds chunk is staged in LDS
//          as [pixel][16 + 4] (20 KB), a thread owns 4 channels and 16 x 4 accumulators, re-reads the span's
//          rows (L2) and writes the workgroup's partial [K][C] to the workspace.
//        LDS: 20 KB + 1 KB of rv, whatever K is.
//   3. score_bwd_fold_kernel   one workgroup per (b, k): the spans' partials in span order, the
//        projection and dt.
#include "common.h"

namespace {

constexpr int K_MAX = DCLIP_CLASSES_MAX;
constexpr int SPAN = 256;  // pixels per workgroup
constexpr int CK = 16;     // classes per phase-B chunk

__device__ __forceinline__ float lane_bcast(float x, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the 4 waves' values in wave order (red: 4 doubles of LDS), returned to every thread
__device__ __forceinline__ double block_sum4(double x, double* red) {
    x = wave_sum_d(x);
    __syncthreads();  // the previous use's readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// |t_row| in f64: every thread's channels in order, the wave's butterfly, the 4 waves in order
__device__ __forceinline__ double row_norm(const float* __restrict__ tr, int C, double* red) {
    double ss = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) ss += (double)tr[c] * (double)tr[c];
    return sqrt(block_sum4(ss, red));
}

// tn[b][k][:] = t rt
__global__ __launch_bounds__(256) void score_bwd_text_kernel(const float* __restrict__ t, float* __restrict__ tn,
                                                             int C, float eps) {
    __shared__ double red[4];
    const int64_t row = blockIdx.x;
    const float* tr = t + row * C;
    const double rt = 1.0 / fmax(row_norm(tr, C, red), (double)eps);
    for (int c = threadIdx.x; c < C; c += 256) tn[row * C + c] = (float)((double)tr[c] * rt);
}

template <typename TDV>
__device__ __forceinline__ void store8(TDV* p, const float* x);
template <>
__device__ __forceinline__ void store8<float>(float* p, const float* x) {
    *(f32x4*)p = f32x4{x[0], x[1], x[2], x[3]};
    *(f32x4*)(p + 4) = f32x4{x[4], x[5], x[6], x[7]};
}
template <>
__device__ __forceinline__ void store8<bf16>(bf16* p, const float* x) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)x[j];
    *(bf16x8*)p = o;
}
template <>
__device__ __forceinline__ void store8<f16>(f16* p, const float* x) {
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)x[j];
    *(f16x8*)p = o;
}

// tn [B][K][C]; part: [B][nspan][K][C]
template <typename TV, typename TDV, int NSLAB>
__global__ __launch_bounds__(256) void score_bwd_kernel(const TV* __restrict__ v, int64_t bstride, int64_t row_off,
                                                        int64_t ld, const float* __restrict__ tn,
                                                        const float* __restrict__ ds, float scale,
                                                        TDV* __restrict__ dv, int64_t dv_bstride, int64_t dv_row_off,
                                                        int64_t dv_ld, float* __restrict__ part, int HW, int C, int K,
                                                        float eps) {
    typedef typename Mfma<TV>::frag frag;  // 8 x 16-bit
    constexpr int PB = 8 / NSLAB;          // pixels a wave holds at a time
    constexpr int KB = 64 / PB;            // classes per ds block: one value per lane
    __shared__ __attribute__((aligned(16))) float ds_s[SPAN][CK + 4];  // pitch 20: the staging stores spread over 8 banks
    __shared__ float rv_s[SPAN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * SPAN;
    const int np = HW - p0 < SPAN ? HW - p0 : SPAN;  // >= 1
    const int nch = C >> 3;                          // 8-channel chunks of a row
    const TV* vb = v + (int64_t)b * bstride + row_off * ld;
    const float* dsb = ds + (int64_t)b * K * HW;
    const float* tnb = tn + (int64_t)b * K * C;
    TDV* dvb = dv + (int64_t)b * dv_bstride + dv_row_off * dv_ld;

    // ---------------------------------------------------------------- phase A: dv
    bool chok[NSLAB];
#pragma unroll
    for (int s = 0; s < NSLAB; ++s) chok[s] = s * 64 + lane < nch;
    // wave w takes the span's pixels [64 w, 64 w + 64), PB at a time
    for (int g = 0; g < 64; g += PB) {
        const int q0 = 64 * wave + g;  // first pixel of the group, within the span
        if (q0 >= np) break;           // uniform in the wave
        float dvn[PB][NSLAB][8];
#pragma unroll
        for (int pp = 0; pp < PB; ++pp)
#pragma unroll
            for (int s = 0; s < NSLAB; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) dvn[pp][s][j] = 0.f;
        for (int k0 = 0; k0 < K; k0 += KB) {
            // lane l holds ds[k0 + l / PB][pixel l % PB of the group], times scale; 0 outside
            const int kl = k0 + lane / PB, ql = q0 + lane % PB;
            float dl = 0.f;
            if (kl < K && ql < np) dl = dsb[(int64_t)kl * HW + p0 + ql] * scale;
            const int kn = K - k0 < KB ? K - k0 : KB;
            for (int kk = 0; kk < kn; ++kk) {
                float tr[NSLAB][8];
#pragma unroll
                for (int s = 0; s < NSLAB; ++s) {
                    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
                    if (chok[s]) {
                        const float* tp = tnb + (int64_t)(k0 + kk) * C + 8 * (s * 64 + lane);
                        lo = *(const f32x4*)tp;
                        hi = *(const f32x4*)(tp + 4);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        tr[s][j] = lo[j];
                        tr[s][4 + j] = hi[j];
                    }
                }
#pragma unroll
                for (int pp = 0; pp < PB; ++pp) {
                    // kk is not a compile-time constant: the lane index goes through an SGPR
                    const float d = lane_bcast(dl, kk * PB + pp);
#pragma unroll
                    for (int s = 0; s < NSLAB; ++s)
#pragma unroll
                        for (int j = 0; j < 8; ++j) dvn[pp][s][j] += d * tr[s][j];
                }
            }
        }
        // the group's rows only now: nothing of them is live across the class loop
        frag row[PB][NSLAB];
#pragma unroll
        for (int pp = 0; pp < PB; ++pp)
#pragma unroll
            for (int s = 0; s < NSLAB; ++s) {
                frag x;
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = (TV)0.f;
                if (q0 + pp < np && chok[s])
                    x = *(const frag*)(vb + (int64_t)(p0 + q0 + pp) * ld + 8 * (s * 64 + lane));
                row[pp][s] = x;
            }
#pragma unroll
        for (int pp = 0; pp < PB; ++pp) {
            const bool pok = q0 + pp < np;
            double ss = 0.0, dot = 0.0;  // |v|^2 and <v, dvn>
#pragma unroll
            for (int s = 0; s < NSLAB; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = (float)row[pp][s][j];
                    ss += (double)(x * x);  // a 16-bit square is exact in f32
                    dot += (double)x * (double)dvn[pp][s][j];
                }
            const double nrm = sqrt(wave_sum_d(ss));
            const double rv = 1.0 / fmax(nrm, (double)eps);
            dot = nrm >= (double)eps ? wave_sum_d(dot) * (rv * rv) : 0.0;  // a <vn, dvn> rv
            if (lane == 0 && pok) rv_s[q0 + pp] = (float)rv;
            if (pok) {
#pragma unroll
                for (int s = 0; s < NSLAB; ++s) {
                    if (!chok[s]) continue;
                    float o[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        o[j] = (float)(rv * ((double)dvn[pp][s][j] - (double)(float)row[pp][s][j] * dot));
                    store8<TDV>(dvb + (int64_t)(p0 + q0 + pp) * dv_ld + 8 * (s * 64 + lane), o);
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // one pixel's f64 temporaries at a time
        }
    }

    // ---------------------------------------------------------------- phase B: dt partials of the span
    float* pw = part + ((int64_t)b * gridDim.x + blockIdx.x) * K * C;
    const int nu = C >> 2;  // 4-channel units of a row
    for (int k0 = 0; k0 < K; k0 += CK) {
        const int kc = K - k0 < CK ? K - k0 : CK;
        __syncthreads();  // rv_s written (first chunk); the previous chunk's readers are done
        for (int e = tid; e < SPAN * CK; e += 256) {
            const int kk = e / SPAN, q = e - kk * SPAN;  // consecutive threads: consecutive pixels of a class
            float d = 0.f;
            if (kk < kc && q < np) d = dsb[(int64_t)(k0 + kk) * HW + p0 + q] * scale;
            ds_s[q][kk] = d;
        }
        __syncthreads();
        for (int u = tid; u < nu; u += 256) {
            float acc[CK][4];
#pragma unroll
            for (int kk = 0; kk < CK; ++kk)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[kk][j] = 0.f;
            typedef TV tv4 __attribute__((ext_vector_type(4)));
            const TV* vu = vb + (int64_t)p0 * ld + 4 * u;
#pragma unroll 2
            for (int q = 0; q < np; ++q) {
                const tv4 x = *(const tv4*)(vu + (int64_t)q * ld);
                const float r = rv_s[q];
                float vn[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) vn[j] = (float)x[j] * r;
#pragma unroll
                for (int k4 = 0; k4 < CK / 4; ++k4) {
                    const f32x4 d = *(const f32x4*)&ds_s[q][4 * k4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[4 * k4 + i][j] += d[i] * vn[j];
                }
            }
#pragma unroll
            for (int kk = 0; kk < CK; ++kk)
                if (kk < kc)
                    *(f32x4*)(pw + (int64_t)(k0 + kk) * C + 4 * u) =
                        f32x4{acc[kk][0], acc[kk][1], acc[kk][2], acc[kk][3]};
        }
    }
}

// dt[b][k][:] = rt (dtn - a tn <tn, dtn>), dtn = the spans' partials in span order
__global__ __launch_bounds__(256) void score_bwd_fold_kernel(const float* __restrict__ part,
                                                             const float* __restrict__ t, float* __restrict__ dt,
                                                             int nspan, int C, int K, float eps) {
    __shared__ double red[4];
    const int k = blockIdx.x, b = blockIdx.y;
    const int64_t row = (int64_t)b * K + k;
    const float* tr = t + row * C;
    const float* pr = part + ((int64_t)b * nspan * K + k) * C;
    const double nrm = row_norm(tr, C, red);
    const double rt = 1.0 / fmax(nrm, (double)eps), a = nrm >= (double)eps ? 1.0 : 0.0;
    float dtn[8];  // C <= 2048: at most 8 channels per thread
    double dot = 0.0;  // <t, dtn>; times rt^2 below
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = threadIdx.x + 256 * i;
        float s = 0.f;
        if (c < C) {
            for (int sp = 0; sp < nspan; ++sp) s += pr[(int64_t)sp * K * C + c];
            dot += (double)tr[c] * (double)s;
        }
        dtn[i] = s;
    }
    dot = block_sum4(dot, red) * (rt * rt) * a;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = threadIdx.x + 256 * i;
        if (c < C) dt[row * C + c] = (float)(rt * ((double)dtn[i] - (double)tr[c] * dot));
    }
}

int nspans(int HW) { return (HW + SPAN - 1) / SPAN; }

template <typename TV, typename TDV>
void launch(const void* v, int64_t bstride, int64_t row_off, int64_t ld, const float* tn, const float* ds, float scale,
            void* dv, int64_t dv_bstride, int64_t dv_row_off, int64_t dv_ld, float* part, int B, int HW, int C, int K,
            float eps, hipStream_t st) {
    const dim3 grid(nspans(HW), B);
#define SCORE_BWD_LAUNCH(NS)                                                                                       \
    score_bwd_kernel<TV, TDV, NS><<<grid, 256, 0, st>>>((const TV*)v, bstride, row_off, ld, tn, ds, scale, (TDV*)dv, \
                                                        dv_bstride, dv_row_off, dv_ld, part, HW, C, K, eps)
    if (C <= 512) SCORE_BWD_LAUNCH(1);
    else if (C <= 1024) SCORE_BWD_LAUNCH(2);
    else SCORE_BWD_LAUNCH(4);
#undef SCORE_BWD_LAUNCH
}

}  // namespace

extern "C" int64_t dclip_score_map_bwd_ws_floats(int B, int HW, int C, int K) {
    if (B <= 0 || HW <= 0 || C <= 0 || C > 2048 || K <= 0 || K > K_MAX) return 0;
    // tn, then the spans' dt partials (each part a multiple of 16 bytes: C % 16 == 0)
    return (int64_t)B * K * C + (int64_t)B * nspans(HW) * K * C;
}

extern "C" int dclip_score_map_bwd(const void* v, int v_dt, int64_t bstride, int64_t row_off, int64_t ld,
                                   const float* t, const float* ds, float scale, void* dv, int dv_dt,
                                   int64_t dv_bstride, int64_t dv_row_off, int64_t dv_ld, float* dt, float* ws, int B,
                                   int HW, int C, int K, float eps, void* stream) {
    DCLIP_HOST_CHECK(K >= 1 && K <= K_MAX, "dclip_score_map_bwd: K=%d (1 <= K <= %d classes)", K, K_MAX);
    DCLIP_HOST_CHECK(v_dt == DCLIP_BF16 || v_dt == DCLIP_F16, "dclip_score_map_bwd: v must be f16/bf16");
    DCLIP_HOST_CHECK(dv_dt == DCLIP_F32 || dv_dt == v_dt, "dclip_score_map_bwd: dv_dt=%d (f32 or v's dtype)", dv_dt);
    DCLIP_HOST_CHECK(C > 0 && C % 16 == 0 && C <= 2048 && ld % 8 == 0 && bstride % 8 == 0 && ((uintptr_t)v % 16) == 0,
                     "dclip_score_map_bwd: C %% 16 == 0, C <= 2048, 16-byte aligned rows");
    DCLIP_HOST_CHECK(dv_ld % 8 == 0 && dv_bstride % 8 == 0 && ((uintptr_t)dv % 16) == 0,
                     "dclip_score_map_bwd: dv needs 16-byte aligned rows (dv_ld, dv_bstride multiples of 8)");
    DCLIP_HOST_CHECK(B > 0 && HW > 0, "dclip_score_map_bwd: empty input");
    DCLIP_HOST_CHECK(B <= 65535, "dclip_score_map_bwd: B=%d (at most 65535)", B);
    DCLIP_HOST_CHECK(row_off >= 0 && dv_row_off >= 0 && ld >= C && dv_ld >= C,
                     "dclip_score_map_bwd: row offsets >= 0 and row pitches >= C");
    DCLIP_HOST_CHECK(v && t && ds && dv && dt, "dclip_score_map_bwd: v, t, ds, dv and dt required");
    DCLIP_HOST_CHECK(((uintptr_t)t % 16) == 0 && ((uintptr_t)dt % 16) == 0 && ((uintptr_t)ds % 4) == 0,
                     "dclip_score_map_bwd: t and dt 16-byte aligned");
    DCLIP_HOST_CHECK(ws != nullptr && ((uintptr_t)ws % 16) == 0,
                     "dclip_score_map_bwd: ws (dclip_score_map_bwd_ws_floats(B, HW, C, K) f32, 16-byte aligned) "
                     "required");
    hipStream_t st = (hipStream_t)stream;
    float* tn = ws;
    float* part = tn + (int64_t)B * K * C;
    score_bwd_text_kernel<<<B * K, 256, 0, st>>>(t, tn, C, eps);
    if (v_dt == DCLIP_BF16) {
        if (dv_dt == DCLIP_F32)
            launch<bf16, float>(v, bstride, row_off, ld, tn, ds, scale, dv, dv_bstride, dv_row_off, dv_ld, part, B, HW,
                                C, K, eps, st);
        else
            launch<bf16, bf16>(v, bstride, row_off, ld, tn, ds, scale, dv, dv_bstride, dv_row_off, dv_ld, part, B, HW,
                               C, K, eps, st);
    } else {
        if (dv_dt == DCLIP_F32)
            launch<f16, float>(v, bstride, row_off, ld, tn, ds, scale, dv, dv_bstride, dv_row_off, dv_ld, part, B, HW,
                               C, K, eps, st);
        else
            launch<f16, f16>(v, bstride, row_off, ld, tn, ds, scale, dv, dv_bstride, dv_row_off, dv_ld, part, B, HW, C,
                             K, eps, st);
    }
    score_bwd_fold_kernel<<<dim3(K, B), 256, 0, st>>>(part, t, dt, nspans(HW), C, K, eps);
    DCLIP_LAUNCH_CHECK();
    return 0;
}
