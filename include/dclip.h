/*
 * dclip.h — C ABI of libdclip.so, the MI355X (gfx950) DenseCLIP ViT hot path.
 *
 * Every entry point takes plain device pointers, element counts/strides and a
 * hipStream_t (passed as void*), launches asynchronously on that stream and returns
 * 0 on success or a negative DCLIP_ERR_* code; dclip_last_error() then holds a
 * message (thread-local).  No entry point synchronises or touches the host side of a
 * tensor, and workspaces are the caller's.  Two entry points allocate device memory
 * themselves, on first use per device: dclip_conv3x3* (one row of zeros, once) and
 * dclip_gemm (the scratch of its M-tail split, regrown whenever a call needs more than
 * any call before it, and shared by all calls: one stream at a time).  So run one
 * warm-up call of every shape before capturing a sequence in a hipGraph; after that a
 * caller may capture any sequence.  (DCLIP_OPT_GEMM_SCHED 1 also allocates its claim
 * counters on first use.)
 *
 * dtype codes: DCLIP_F32 / DCLIP_F16 / DCLIP_BF16.  Matrices are row-major with
 * explicit leading dimensions (in elements).
 *
 * Reference interface each entry point replaces (paths relative to
 * /root/reference/segmentation):
 *   dclip_layernorm_fwd/bwd    denseclip/models.py:243-249  LayerNorm.forward (fp32 math)
 *   dclip_gemm                 nn.Linear in models.py:275-281 (MHA in/out proj, c_fc,
 *                              c_proj), conv1 patchify models.py:407/546 as GEMM,
 *                              vis_proj / global_proj denseclip.py:198-199,605-616,
 *                              and every weight/input gradient of those
 *   dclip_attn_fwd/bwd         nn.MultiheadAttention core (SDPA) models.py:287-289
 *   dclip_conv3x3(_wgrad)      ViTFeatureFusionNeck 3x3 ConvBNReLU convs models.py:741-745
 *   dclip_upsample_ce/silog    logits/depth resize + CE / SILog losses denseclip.py:843-868,
 *                              train_denseclip.py:1265-1314, losses.py:21-78
 *   dclip_upsample_depth_stats/finish  the depth loss as a weighted sum of SILog, L1 and BerHu on the resized
 *                              depth, configs/denseclip_multitask_cityscapes.yaml:67-70,
 *                              train_denseclip.py:1276-1312
 *   dclip_upsample_eval_seg/depth  validate()'s resize + argmax / confusion matrix / CE and depth
 *                              errors, train_denseclip.py:294-684, denseclip/utils.py:109-139,
 *                              utils/depth_metrics.py:12-88
 *   dclip_slide_eval_seg/depth test_cfg mode='slide' of configs/denseclip_fpn_vit-b_640x640_80k.py:51 (the
 *                              rule is mmseg's slide_inference, restated at the entry points)
 *   dclip_slide_tta_eval_seg/depth  the same under test.py:91-96 --aug-test (mmseg's aug_test over
 *                              slide_inference: every scaled / mirrored view evaluated with windows)
 *   dclip_adamw_prepare/update torch.optim.AdamW.step + clip_grad_norm_ + the 1/grad_accum_steps loss scaling,
 *                              train_denseclip.py:1061, 1154-1155, 1314, 1356-1358
 *   dclip_im2col               conv1 (16x16, stride 16, no bias) models.py:407,546
 *   dclip_tokens_fwd/bwd       flatten/transpose + CLS + pos add, models.py:548-556
 *   dclip_pos_interp_fwd/bwd   interpolate_pos_encoding models.py:514-540
 *   dclip_transpose            per-layer read-out NLC->NCHW models.py:568-582 (and its
 *                              gradient), NCHW->NHWC for vis_proj, GEMM operand
 *                              transposes with fused bias-gradient column sums
 *   dclip_row_mean             F.adaptive_avg_pool2d(...,(1,1)) denseclip.py:596
 *   dclip_score_map            F.normalize x2 + einsum('bchw,bkc->bkhw')
 *                              denseclip.py:672-675
 *   dclip_*_classes            the score map, fused CE and fused evaluation for any class count <= 256
 *   dclip_score_concat         upsample + torch.cat of the score map onto a read-out map
 *                              denseclip.py:684-694
 *   dclip_bilinear_fwd/bwd     F.interpolate(bilinear, align_corners=False)
 *                              denseclip.py:847,860,899,909 (logits/depth upsample)
 *   dclip_cast                 dtype conversion of operands (.type()/.to() casts)
 *   dclip_cityscapes_prepare   Cityscapes label remap, disparity->depth, crop/flip/normalise
 */
#ifndef DCLIP_H
#define DCLIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCLIP_F32 0
#define DCLIP_F16 1
#define DCLIP_BF16 2
#define DCLIP_U8 3    /* dclip_cityscapes_augment (the uint8 HWC crop, before ColorJitter / Normalize) and
                         dclip_ade20k_prepare (the uint8 CHW crop, before the normalisation) only */

#define DCLIP_OK 0
#define DCLIP_ERR_ARG (-1)
#define DCLIP_ERR_HIP (-2)

/* GEMM epilogues (dclip_gemm) */
#define DCLIP_EPI_STORE 0      /* C = acc (+ bias[n])                                  */
#define DCLIP_EPI_GELU 1       /* C = z = acc + bias ; C2 = z * sigmoid(1.702 z) ; C null: C2 only */
#define DCLIP_EPI_RESIDUAL 2   /* C(f32) = aux(f32) + acc + bias (aux may alias C); C2, when set, gets the same values in ab_dt */
#define DCLIP_EPI_GELU_BWD 3   /* C = acc * quick_gelu'(aux)       (aux = z)           */
#define DCLIP_EPI_SPLITK 4     /* C(f32) = sum over K splits (+ bias): partial f32 slabs
                                  in the caller's workspace aux (splits*M*N f32), then
                                  one deterministic combine pass (weight gradients)    */
#define DCLIP_EPI_STORE_SCALED 5 /* C = (acc + bias[n]) * aux[n], aux = f32 per-column scale
                                  (the q columns of the in-projection pre-multiplied by
                                  d^-0.5 * log2(e) for dclip_attn_*)                    */

const char* dclip_last_error(void);
int dclip_abi_version(void);

/* Kernel-variant knobs for A/B tuning in one process (process-global, not thread-safe;
 * 0 restores the default).  Results do not depend on them beyond fp32 summation order.  */
#define DCLIP_OPT_ATTN_FWD_WAVES 0   /* 4 or 8 (default) waves = 128 / 256 queries per workgroup */
#define DCLIP_OPT_ATTN_DQ_WAVES 1    /* 4 or 8 (default): dQ pass queries per workgroup / 32      */
#define DCLIP_OPT_ATTN_DKDV_WAVES 2  /* 4 (default) or 8: dK/dV pass keys per workgroup / 32      */
#define DCLIP_OPT_GEMM_TILE 3        /* dclip_gemm tiles: 0 auto (default: 6, 1 below 4096 rows), 1 128x128, 2 256x256, 3 256x128, 4 256x256 k32x4, 5 256x256 ping-pong, 6 persistent 256x256, 7 the same with 4 waves of 128x128, 8 / 9 persistent with pipelined fragment reads (8 / 4 waves) */
#define DCLIP_OPT_GEMM_TN_TILE 4     /* dclip_gemm_tn tiles: 0 auto (default: 256x256 when M, N >= 256), 1 128x128, 2 256x256 with 32-row K-steps in a 4-deep ring, 3 the same 5-deep, 4 256x256 on 4 waves of 128x128, 5 the weight-gradient kernels (256x256 and 128x128) and the conv weight-gradient kernel with the LDS-DMA builtin instead of the asm form (round 6 late: the builtin made every K-step wait for the next one's staging) */
#define DCLIP_OPT_ATTN_DKDV_QS 5     /* dK/dV pass query rows per barrier: 64 (default) or 128 */
#define DCLIP_OPT_ATTN_BWD_KERNEL 7  /* 0 (default): CLS-split passes for N >= 257 (a ragged N-1 with the default pass variants only); 1: generic */
#define DCLIP_OPT_ATTN_FWD_KERNEL 6  /* 0 (default): CLS-split kernels (the pipelined attn_fwd3 when N - 1 is a multiple of 256, else attn_fwd2, ragged N-1 included); 1: generic; 2: attn_fwd3 4 waves x 64 rows; 3: attn_fwd3 8 waves; 4: attn_fwd2 always */
#define DCLIP_OPT_ATTN_BWD_BLOCK 8   /* CLS-split backward: 0 (default): the one-pass backward (attention_bwd1.hip: dK, dV and per-key-block dQ partials in one pipelined key-major sweep, an ordered dQ reduction; dclip_attn_bwd_workspace includes the partials, 3.2 GB at B=8, N=8193, H=12) with a persistent sweep (one workgroup per CU) that reduces most dQ partials at its tile seams, the reduction pass completing the rest; 10: the same with a workgroup per tile and the whole reduction in its own pass (bitwise equal); 9: the unpipelined sweep (a workgroup per tile); 6: the two-pass dQ + dK/dV passes, 64 keys per wave, AGPR dK / dV (attention_dkdv6.hip); 7: its software-pipelined schedule; 8: its ring DMA inside R4; 5: software-pipelined 32 keys per wave; 1: the unpipelined one */
#define DCLIP_OPT_GEMM_TN_COLSUM 9   /* 0 (default): the 256x256 weight-gradient kernel sums dY's columns (bias gradient) itself; 1: a separate pass */
#define DCLIP_OPT_GEMM_EPI 10      /* persistent NT GEMM epilogue: 0 (default) row-major through LDS, whole 128-B lines per store, streaming (nontemporal) stores for the wide forward outputs (N >= 2048, not RESIDUAL / GELU_BWD); 1 the accumulator-layout stores (16 rows x 64 B); 2 row-major, streaming stores for every output; 3 row-major, no streaming stores */
#define DCLIP_OPT_GEMM_TAIL 11     /* persistent NT GEMM M tail (<= 16 rows): 0 (default) one latency-shaped MFMA launch (16 columns per workgroup, every K-slice load issued up front, side inputs prefetched); 1 the 256-row split-K tile + combine pair; 2 round 4's one launch (64 columns per workgroup, 8 waves, K % 256 == 0) */
#define DCLIP_OPT_ATTN_FP8_QK 12   /* dclip_attn_fwd_fp8: 0 (default) S = QK^T on the 16-bit MFMA, P V on the fp8 one; 1 both on fp8 (the round-3 kernel) */
#define DCLIP_OPT_ATTN_DQ_ISSUE 13  /* CLS-split dQ pass LDS-DMA issue: 0 (default) a ragged-tile branch; 1 branch-free per-lane select */
#define DCLIP_OPT_ATTN_DQ_ROWS 14   /* CLS-split dQ pass query rows per wave: 32 (default; 8 waves, two per SIMD) or 64 (4 waves, one per SIMD) */
#define DCLIP_OPT_ATTN_DQ_DEFER 15  /* CLS-split dQ pass: 0 (default) a unit's dQ MFMAs right after its softmax; 1 half a step later, beside the next unit's S / dP chains */
#define DCLIP_OPT_GEMM_SCHED 16     /* persistent NT GEMM tile walk: 0 (default) static (round * G + block); 1 work-conserving (every tile claimed: round-0 ownership bitmap, XCD-local ranges, stealing) */
#define DCLIP_OPT_GEMM_KLOOP 17     /* 8-wave GEMM K-loops: 0 (default) the persistent NT kernel with its fragment reads issued one 8-MFMA group ahead except on the GELU epilogue, the TN kernel as compiled; 1 read-ahead in every NT and TN K-loop; 2 none */
#define DCLIP_OPT_ATTN_DQ_REDUCE 18 /* one-pass backward dQ reduction: 0 (default) 8 lanes per query, each lane its 8 columns over the key blocks; 1 8 queries per workgroup, their partial runs read contiguously into LDS (1 KiB per wave-instruction), then 2 columns per lane summed in the same key-block order (bitwise equal) */
#define DCLIP_OPT_ATTN_PREP_ORDER 19 /* one-pass backward prep pass: 0 (default) query blocks of one head on adjacent workgroups; 1 the heads of one query block on adjacent workgroups (same per-workgroup work, bitwise equal) */
#define DCLIP_OPT_ATTN_BWD_WGS 20 /* one-pass backward, persistent sweep (DCLIP_OPT_ATTN_BWD_BLOCK 0): its workgroup count; 0 (default) one per CU; a small value makes a small shape walk several rounds (tests). At or above the tile count (B*H*ceil((N-1)/256)) the sweep has no seams and runs a workgroup per tile */
#define DCLIP_OPT_COUNT 21
int dclip_set_option(int id, int value);

/* LayerNorm over the last dim (cols), eps, affine w/b (fp32).  y = (x-mu)*rstd*w+b.
 * mean/rstd (rows) are written when non-null.                                        */
int dclip_layernorm_fwd(const void* x, int x_dt, const float* w, const float* b,
                        void* y, int y_dt, float* mean, float* rstd,
                        int64_t rows, int64_t cols, float eps, void* stream);

/* LayerNorm backward.  dy: grad wrt y (dy_dt), x: the LN input (x_dt), mean/rstd from
 * the forward.  dx (f32) is overwritten (accumulate=0) or added to (accumulate=1).
 * dw/db (f32, cols) are ACCUMULATED (callers zero them first).                       */
int dclip_layernorm_bwd(const void* dy, int dy_dt, const void* x, int x_dt,
                        const float* w, const float* mean, const float* rstd,
                        float* dx, int accumulate, float* dw, float* db,
                        int64_t rows, int64_t cols, void* stream);
/* The same with the residual branch's gradient fused in: dx = res + LN^T(dy) (res f32, may be
 * null or alias dx) and, when lp is non-null, a 16-bit copy lp = (lp_dt) dx (lp_dt F16 or
 * BF16) — the next GEMM's operand, without a separate clone / cast pass (the
 * x + f(LN(x)) residual of models.py:292-293, backward).                              */
int dclip_layernorm_bwd_res(const void* dy, int dy_dt, const float* dy_scale, int64_t dy_ntok,
                            const void* x, int x_dt, const float* w, const float* mean, const float* rstd,
                            const float* res, float* dx, void* lp, int lp_dt, float* dw, float* db,
                            float* ws, int64_t rows, int64_t cols, void* stream);
/* dy_scale, dy_ntok (ABI 6; dclip_layernorm_bwd_res, _scaled, _scaled_add): dy is read as
 * dy * (*dy_scale) when dy_scale is non-null (an f16 dy still on its gradient scale s, dy_scale
 * pointing at 1/s: the fp16 backward's dX GEMMs write their output for the LN backward in f16 on
 * the scale their operand carries), and rows with row % dy_ntok == 0 read as 0 when dy_ntok > 0
 * (a token-buffer gradient whose CLS rows are not part of it: the ln_post read-out's).  NULL / 0:
 * dy as given.  Need cols in {512, 768, 1024}.                                               */
/* ws (ABI 5; dclip_layernorm_bwd_res, _scaled, _add, _scaled_add): the caller's scratch of
 * dclip_layernorm_bwd_ws_floats(rows, cols) floats (contents on entry irrelevant, clobbered) for
 * the per-workgroup dw / db partials, summed into dw / db in a fixed order (deterministic) by a
 * second launch on the same stream; private to the call, so concurrent calls on different
 * streams or graph replays never share it.  NULL: the workgroups add atomically into dw / db
 * (correct, summation order not fixed).  Widths without the fast kernels (cols not 512 / 768 /
 * 1024; the query returns 0 for them) always add atomically.                               */
int64_t dclip_layernorm_bwd_ws_floats(int64_t rows, int64_t cols);

/* C[m][n] = alpha * sum_k A[m][k] * B[n][k]  ("NT": both operands k-contiguous, ab_dt in
 * {F16, BF16}), m < M, n < N, k < K (K % 64 == 0, lda/ldb % 8 == 0), then the
 * epilogue.  bias: f32[N] or null.  aux: epilogue side input (see DCLIP_EPI_*).
 * alpha undoes a gradient scale carried by an operand (fp16 backward; 1 otherwise); when
 * alpha_ptr is non-null the factor is alpha * *alpha_ptr, read on the device (the 1/s entry
 * of a dclip_grad_scale pair: no host round trip).
 * splits > 1 (EPI_SPLITK only) splits K into `splits` equal 64-multiple chunks.
 * Alignment, as the kernels access memory today: a run of 8 consecutive columns of a row
 * of C, C2 or aux (RESIDUAL: f32, GELU_BWD: ab_dt) is one 16-byte access in a 16-bit matrix
 * and two in an f32 one (the persistent kernel: 4 columns, 8 or 16 bytes), and bias and
 * STORE_SCALED's scale vector are read 4 or 8 floats at a time.  Hence
 *   A, B, C, C2, aux, bias: 16-byte aligned (A and B: checked);
 *   lda, ldb % 8 == 0 (checked); ldc, ldc2, ld_aux % 8 == 0 for a 16-bit matrix, % 4 == 0
 *   for an f32 one (checked for RESIDUAL's C and aux and for SPLITK's C only).
 * N need not be a multiple of 8: a row's last, partial run is accessed element by element.
 * What is not checked is not rejected: the persistent kernel declines a call whose bias /
 * scale vector is not 16-byte aligned or whose ldc, ldc2 or ld_aux is not a multiple of 4
 * (the grid kernel runs instead), and every other kernel then issues unaligned vector
 * accesses, which no test covers.                                                      */
int dclip_gemm(int epilogue, int ab_dt,
               const void* A, int64_t lda, const void* B, int64_t ldb,
               int64_t M, int64_t N, int64_t K, int splits, float alpha, const float* alpha_ptr,
               const float* bias, const void* aux, int aux_dt, int64_t ld_aux,
               void* C, int c_dt, int64_t ldc, void* C2, int64_t ldc2, void* stream);

/* C[m][n] = alpha * sum_k A[k][m] * B[k][n] ("TN": reduction over the ROWS of both operands —
 * the weight-gradient shape dW = dY^T X without transposed copies).  A: (K, lda >= M),
 * B: (K, ldb >= N), M % 8 == N % 8 == 0.  The K range is split into `splits` chunks of
 * K_pad / splits (K_pad >= K, multiple of 64*splits; rows >= K contribute zero).
 * epilogue STORE (f32 C, splits == 1) or SPLITK (f32 slabs in ws, then a combine that adds
 * bias[n] when non-null; ws holds splits*(M*N + M) floats: the slabs, then (ABI 5) the column
 * sums' per-split partials).  colsum_a (f32, M), when non-null, receives += alpha * the column
 * sums of A over the K rows (the bias gradient of dY) — in a fixed order on every path, so the
 * result repeats bit for bit: inside the 256x256 kernel (M, N >= 256), or by a separate pass
 * over A on the small-tile path and for the tiles without fused sums (one block row per split,
 * each reducing its rows in LDS in a fixed order; no float atomics); with SPLITK the per-split
 * partials are added in split order by the combine.  alpha_ptr as in dclip_gemm.        */
/* The K-split plan dclip_gemm_tn runs best with for an M x N output over K rows
 * (splits, and K_pad = K rounded up to 64*splits); host-side only, no GPU work.      */
int dclip_gemm_tn_plan(int64_t M, int64_t N, int64_t K, int* splits, int64_t* K_pad);

int dclip_gemm_tn(int epilogue, int ab_dt, const void* A, int64_t lda, const void* B, int64_t ldb,
                  int64_t M, int64_t N, int64_t K, int64_t K_pad, int splits, float alpha,
                  const float* alpha_ptr, const float* bias,
                  void* ws, void* C, int64_t ldc, float* colsum_a, void* stream);

/* Fused multi-head attention over a packed QKV buffer.
 * qkv: (B*N, 3*H*D) row-major, [q | k | v] each (H, D) head-major (the layout of
 *      x @ in_proj_weight^T + in_proj_bias, models.py:289 / F.multi_head_attention_forward)
 *      with the q columns PRE-MULTIPLIED by c = scale * log2(e) ("log2-domain queries",
 *      produced for free by the in-projection GEMM's DCLIP_EPI_STORE_SCALED epilogue)
 * o:   (B*N, H*D) softmax(q k^T * scale) v, heads concatenated
 * lse: (B, H, N) f32, log2-domain row statistic  max*c + log2(sum), c = scale*log2(e)
 * D must be 64.                                                                      */
int dclip_attn_fwd(int dt, const void* qkv, void* o, float* lse,
                   int B, int N, int H, int D, float scale, void* stream);

/* Attention backward (flash-style recompute from lse; no N x N buffer, no atomics): for N >= 257
 * (the CLS split) by default the one-pass backward (round 6: a prep pass writing delta =
 * rowsum(dout*o) and the statistics, one key-major sweep for dK, dV and 16-bit dQ partials per
 * 256-key block, an ordered reduction of the partials); with DCLIP_OPT_ATTN_BWD_BLOCK 6, and below
 * N = 257, a query-major dQ pass (which also writes delta) and a key-major dK/dV pass.  dout:
 * (B*N, H*D) dt.  delta_ws: f32 workspace of dclip_attn_bwd_workspace(B, N, H) floats, a function
 * of (B, N, H) alone — no option changes it, so a size queried once serves a launch under any
 * option: for N >= 257 it includes the one-pass form's partials (B*H*ceil((N-1)/256)*
 * (1+64*ceil((N-1)/64))*128 bytes, 3.2 GB at B = 8, N = 8193, H = 12), the largest form; below 257
 * it is the two-pass part alone.  Its contents on entry are irrelevant.  For N >= 257 it begins with
 * the persistent sweep's seam state (B*H counters of published tiles, then B*H*ceil((N-1)/32) flags
 * of reduced 32-row dQ blocks, 32-bit words, padded to 256 bytes), which every call that uses it
 * zeroes itself with a memset node on `stream` (a captured call replays clean).  The next
 * B*H*N floats (the first, below N = 257) receive delta; the rest holds the CLS-split row-0 partials,
 * the negated lse / delta planes, key 0's dS column and the dQ partials.  The one-pass form addresses an (image,
 * head)'s partials with 32-bit offsets: when (1+64*ceil((N-1)/64))*ceil((N-1)/256)*128 >= 2^32
 * (N above about 92.7k) the call fails with DCLIP_ERR_ARG ("N too large") before any launch;
 * DCLIP_OPT_ATTN_BWD_BLOCK 6 (the two-pass backward) has no such limit.
 * qkv as for dclip_attn_fwd (q pre-multiplied by scale*log2(e)); `scale` = d^-0.5.
 * dqkv: (B*N, 3*H*D) dt output, [dq | dk | dv] in the qkv layout: gradients with
 * respect to the UNSCALED q, k, v (i.e. the in-projection output before the q scale).  */
int dclip_attn_bwd(int dt, const void* qkv, const void* o, const void* dout,
                   const float* lse, float* delta_ws, void* dqkv,
                   int B, int N, int H, int D, float scale, void* stream);

/* configs[4]'s attention backward (ABI 7): dclip_attn_bwd's contract and results within e4m3
 * rounding — on the CLS-split path (N >= 257) the dK / dV pass runs dV = P^T dO and dK = dS^T q' on
 * the block-scaled e4m3 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, MX E8M0 scales per 32 queries: the
 * Q / dO rows' from a pack pass, P's fixed at 2^-8, dS's per key from its amax), S, dP and the dQ
 * pass stay 16-bit; elsewhere it is dclip_attn_bwd.  The CLS-split path has this one form (the dQ
 * pass, the e4m3 dK / dV pass, the fold merge): DCLIP_OPT_ATTN_BWD_BLOCK selects among the 16-bit
 * dK / dV passes and is NOT read here — every value gives the result of 0, a ragged N - 1
 * included (the DCLIP_OPT_ATTN_DQ_* options still pick the dQ pass's variant).  "Elsewhere" is
 * N < 257, DCLIP_OPT_ATTN_BWD_KERNEL 1, and a ragged N - 1 (not a multiple of 256) with
 * DCLIP_OPT_ATTN_DQ_WAVES 4: those run dclip_attn_bwd's generic 16-bit passes, bit for bit its
 * result under the same options.  ws: dclip_attn_bwd_fp8_workspace(B, N, H)
 * floats, 16-B aligned (dclip_attn_bwd's two-pass workspace, then the slices' e4m3 images).  Replaces the
 * backward of models.py:287-289 under the fp8 attention of BASELINE configs[4].               */
int64_t dclip_attn_bwd_fp8_workspace(int B, int N, int H);
int dclip_attn_bwd_fp8(int dt, const void* qkv, const void* o, const void* dout, const float* lse, float* ws,
                       void* dqkv, int B, int N, int H, int D, float scale, void* stream);
int64_t dclip_attn_bwd_workspace(int B, int N, int H);

/* fp8 attention forward (BASELINE config 5; inference only — there is no fp8 backward).
 * Same qkv / o / lse contract as dclip_attn_fwd (q pre-multiplied by d^-0.5*log2(e)), computed
 * on the block-scaled e4m3 MFMA v_mfma_scale_f32_32x32x64_f8f6f4: q, k, v are quantised to
 * OCP e4m3 with one scale per (image, head, q|k|v) = 448 / amax, P to e4m3 unscaled (P <= 1).
 * ws: dclip_attn_fwd_fp8_workspace(B, N, H) bytes, 256-byte aligned (the packed q8 / k8 /
 * transposed v8 planes and the amax table).  H <= 64, D must be 64.                      */
int dclip_attn_fwd_fp8(int dt, const void* qkv, void* o, float* lse, void* ws,
                       int B, int N, int H, int D, void* stream);
int64_t dclip_attn_fwd_fp8_workspace(int B, int N, int H);

/* Non-overlapping p x p patches of img (B, Cin, Hin, Win) (img_dt) ->
 * out (B*gh*gw, ldo) (out_dt), column order (c, ky, kx) = conv weight flattening,
 * gh = Hin / p, gw = Win / p (floor, as Conv2d stride p).  Columns Cin*p*p .. ldo-1
 * are written as zeros: ldo = the patch GEMM's K padded to 64 (p = 14: 588 -> 640).
 * ldo % 4 == 0.                                                                        */
int dclip_im2col(const void* img, int img_dt, void* out, int out_dt, int64_t ldo,
                 int B, int Cin, int Hin, int Win, int p, void* stream);

/* Token assembly: x[b][0] = cls + pos[0]; x[b][1+i] = patch[b*P+i] + pos[1+i]
 * x: f32 (B*(P+1), C).  patch: (B*P, C) patch_dt.  pos: f32 (P+1, C).              */
int dclip_tokens_fwd(const void* patch, int patch_dt, const float* cls, const float* pos,
                     float* x, int B, int P, int C, void* stream);

/* Token assembly backward: dpatch[b*P+i] = dpatch_scale * dx[b][1+i] (dpatch_dt; times
 * *dpatch_scale_ptr when non-null, read on the device);
 * dcls += sum_b dx[b][0]; dpos[t] += sum_b dx[b][t]  (dcls/dpos f32, accumulated)   */
int dclip_tokens_bwd(const float* dx, void* dpatch, int dpatch_dt, float dpatch_scale,
                     const float* dpatch_scale_ptr, float* dcls, float* dpos, int B, int P, int C,
                     void* stream);

/* Bilinear (align_corners=False) resize of the g x g patch grid of pos (g*g+1, C)
 * to H x W; out (H*W+1, C), row 0 = pos row 0.                                       */
int dclip_pos_interp_fwd(const float* pos, float* out, int g, int C, int H, int W,
                         void* stream);
/* Its gradient: dpos (g*g+1, C) += interp^T(dout); dout (H*W+1, C).                 */
int dclip_pos_interp_bwd(const float* dout, float* dpos, int g, int C, int H, int W,
                         void* stream);

/* Batched transpose: out[b][c][r] (=, or += if accumulate) in[b][r0 + r][c]
 * for r < rows, c < cols; rows..rows_pad-1 of every out row are written as 0.
 * colsum (f32, cols) += sum over b, r of in[b][r0+r][c] when non-null.
 * Strides in elements.  accumulate requires out_dt == F32.                          */
int dclip_transpose(const void* in, int in_dt, int64_t in_bstride, int64_t in_ld, int64_t r0,
                    void* out, int out_dt, int64_t out_bstride, int64_t out_ld,
                    int batch, int64_t rows, int64_t rows_pad, int64_t cols,
                    int accumulate, float* colsum, void* stream);

/* Compute-dtype weight copies after an optimizer step (no reference counterpart: the reference
 * runs fp32 weights; replaces one cast and one transpose launch per weight per step).  desc:
 * n entries of 8 int64 ON THE DEVICE: [src (f32, rows x cols, contiguous, 16-B aligned),
 * plain dst (out_dt, rows x cols) or 0, transposed dst (out_dt, cols x rows) or 0, rows, cols,
 * first tile, column tiles = ceil(cols / 64), 0]; entry e covers tiles [first, first +
 * ceil(rows / 64) * column tiles), the entries in order, tiles = the total.  One launch.      */
int dclip_weight_refresh(const int64_t* desc, int n, int64_t tiles, int out_dt, void* stream);

/* Strided pixel rows: row r (< rows) of image b is X + b*bstride + (row_off + r)*ld (elements; a ViT
 * token buffer (B*N, C) has bstride N*C, row_off 1 (skips CLS), ld C).  16-bit X, 16-byte aligned rows.
 *
 * out[b][c] (f32) = mean over r < rows of row r of image b  (F.adaptive_avg_pool2d(x, (1, 1)),
 * denseclip.py:596); ws: dclip_row_mean_workspace(B, rows, C) floats (fixed-order chunk sums).
 * C % 8 == 0, C <= 2048.                                                                       */
int64_t dclip_row_mean_workspace(int B, int64_t rows, int C);
int dclip_row_mean(const void* x, int x_dt, int64_t bstride, int64_t row_off, int64_t ld, int B, int64_t rows,
                   int C, float* ws, float* out, void* stream);

/* Pixel-text score map (F.normalize x2 + einsum('bchw,bkc->bkhw'), denseclip.py:672-675) as a
 * batched MFMA product.  v: strided pixel rows as above (HW rows per image, v_dt F16/BF16),
 * t: f32 (B, K, C).  score f32 (B, K, HW) = <v/max(|v|,eps), t/max(|t|,eps)>.  K <= 32,
 * C % 16 == 0, C <= 2048.                                                                      */
int dclip_score_map(const void* v, int v_dt, int64_t bstride, int64_t row_off, int64_t ld, const float* t,
                    float* score, int B, int HW, int C, int K, float eps, void* stream);

/* The score_concat_index branch's torch.cat([x_i, F.interpolate(score, (h, w)).to(x_i.dtype)], 1)
 * (denseclip.py:684-694) in one pass: out (B*h*w, C + K) channels-last rows, 16-bit (dt) = the
 * strided pixel rows of x_i (as dclip_row_mean: image b's pixel p at b*bstride + (row_off + p)*ld)
 * followed by the bilinearly resized (align_corners=False) f32 score (B, K, hs, ws), K <= 64.      */
int dclip_score_concat(const void* rows, int dt, int64_t bstride, int64_t row_off, int64_t ld, int C,
                       const float* score, int K, int hs, int ws, void* out, int B, int h, int w, void* stream);

/* Bilinear resize, align_corners=False, of NC planes (NC, Hi, Wi) -> (NC, Ho, Wo).  Every
 * bilinear entry point (this pair, dclip_pos_interp_*, dclip_score_concat) takes its weights
 * from PyTorch's index formula in f32: scale = in / out, src = max(scale * (dst + .5) - .5, 0)
 * with the multiply-subtract FUSED (rounded once, as PyTorch's own kernels are compiled; rounding
 * the product first moves src by an ulp at a fifth of the columns of a 5 -> 1028 resize), i0 =
 * (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1; equal sizes copy exactly.   */
int dclip_bilinear_fwd(const void* in, int in_dt, void* out, int out_dt,
                       int64_t NC, int Hi, int Wi, int Ho, int Wo, void* stream);
/* Its gradient: din f32 (NC, Hi, Wi) = resize^T(dout).  ws: f32 (NC, Ho, Wi).        */
int dclip_bilinear_bwd(const void* dout, int dout_dt, float* din, float* ws,
                       int64_t NC, int Hi, int Wi, int Ho, int Wo, void* stream);

/* 3x3 / stride 1 / pad 1 convolution as an implicit GEMM on channels-last pixel rows
 * (the ViTFeatureFusionNeck's per-level convs, reference models.py:741-745 / 13-20, run on
 * the ViT token read-out without NCHW copies).  Input pixel (b, y, x) of the B x H x W image
 * is the row X + b*x_bstride + x_off + (y*W + x)*x_ld (elements, all multiples of 8); for a
 * ViT token buffer (B*N, C): x_bstride = N*C, x_off = C (skips CLS), x_ld = C.
 *   mode 0 (forward):  out[p][n] = sum_{tap, c} X[p + d(tap)][c] * Wt[n][tap*Cin + c]
 *   mode 1 (dgrad):    out[p][n] = sum_{tap, c} X[p - d(tap)][c] * Wt[n][tap*Cin + c]
 *                      (X = dOut with Cin = Cout channels, Wt[ci][tap*Cout + co] = w[co][ci][tap])
 * d(tap) = (tap/3 - 1, tap%3 - 1); out-of-image taps read zeros.  Cin % 64 == 0.
 * Output row of pixel p: p, or with out_gap > 0: p + (p / (H*W))*out_gap + out_off (e.g.
 * gap 1, off 1 writes into rows 1.. of each batch of a (B*N, C) token buffer); out_ld is
 * its row pitch.  out_dt: f32 or the operand dtype; accumulate=1 (f32 only) adds.        */
int dclip_conv3x3(int mode, int ab_dt, const void* X, int64_t x_bstride, int64_t x_off, int64_t x_ld,
                  int B, int H, int W, int Cin, const void* Wt, int Nout, void* out, int out_dt,
                  int64_t out_ld, int out_gap, int out_off, int accumulate, void* stream);

/* Weight gradient of the 3x3 conv: dW[co][tap*Cin + c] = sum_p dY[p][co] * X[p + d(tap)][c]
 * (f32, Nout x 9*Cin), pixels split into `splits` chunks summed through ws
 * (splits * Nout * 9*Cin f32) in a fixed order.  Cin % 128 == 0.  oihw = 1 writes torch's
 * weight layout instead, dW[co][c][tap] (Nout, Cin, 3, 3), times *alpha_ptr when given (the 1/s
 * entry of an fp16 gradient-scale pair; alpha_ptr needs oihw = 1).                       */
int dclip_conv3x3_wgrad(int ab_dt, const void* dY, int64_t ldy, int Nout, const void* X, int64_t x_bstride,
                        int64_t x_off, int64_t x_ld, int B, int H, int W, int Cin, float* dW, void* ws,
                        int splits, int oihw, const float* alpha_ptr, void* stream);

/* Fused bilinear upsample (align_corners=False) + loss + gradient of the heads
 * (denseclip.py:843-868 resize, train_denseclip.py:1265-1314 losses), without materialising
 * the upsampled tensors.  logits: (B, K, h, w) low_dt; labels: (B, H, W) int64 (lab_dt 0),
 * int32 (1) or uint8 (2); pixels whose label is ignore_index (or outside [0, K)) are skipped.
 *   dclip_upsample_ce:    loss_sum (f64[1]) += sum of -log softmax(up(logits))[label],
 *                         count (u32[1]) += #valid, grad (f32, B*K*h*w, accumulated)
 *                         += up^T(softmax - onehot)   (the caller scales by 1/count)
 *   dclip_upsample_silog: pred (B, 1, h, w); target f32 (B, H, W); mask u8 (B, H, W) or null.
 *                         pass 0: sums (f64[3]) += (sum d, sum d^2, T), d = log(max(up(pred),
 *                         eps)) - log(max(target, eps)) on the mask; pass 1 (sums complete):
 *                         grad (f32, B*h*w) += up^T((2d/T - 2 lambd S/T^2) / up(pred))
 *                         (zero where up(pred) < eps).  K == 19 for the CE kernel.
 *                         A mask byte counts as valid when non-zero.  Masked-out targets may hold
 *                         anything, NaN included: they are not used.  A NaN among the in-mask
 *                         resized predictions or targets makes sums[0..1] NaN (max() here keeps a
 *                         NaN, as torch.clamp does); T counts the pixel all the same.
 * ws (ABI 7): the caller's scratch of dclip_upsample_ws_floats(B, K, h, w) floats (K = 1 for
 * SILog), 8-byte aligned, contents undefined on entry: every workgroup writes its loss partials
 * and its low-res gradient tile there and two short launches add them in a fixed order, so the
 * loss and the gradient are bitwise reproducible (ABI 6 used float atomics).  Stream-ordered:
 * one ws per call in flight.                                                            */
int64_t dclip_upsample_ws_floats(int B, int K, int h, int w);
int dclip_upsample_ce(int low_dt, const void* logits, int B, int K, int h, int w, const void* labels, int lab_dt,
                      int H, int W, int ignore_index, double* loss_sum, unsigned* count, float* grad, float* ws,
                      void* stream);
int dclip_upsample_silog(int pass, int low_dt, const void* pred, int B, int h, int w, const float* target,
                         const uint8_t* mask, int H, int W, float eps, float lambd, double* sums, float* grad,
                         float* ws, void* stream);

/* The depth loss as any weighted sum of SILog, L1 and BerHu (the reference's LOSS_TYPE 'silog', 'berhu' or
 * 'l1', configs/denseclip_multitask_cityscapes.yaml:67-70, and "the sum of depth components",
 * train_denseclip.py:1276-1312) on the resized prediction, which is never materialised
 * (csrc/depthlossopt.hip).  Additive to ABI 7; dclip_upsample_silog is untouched.
 * pred (B, 1, h, w) low_dt; target f32 (B, H, W); mask u8 (B, H, W) or null; B*H*W < 2^31.  On the mask M
 * (a non-zero byte; every pixel without a mask), p = up(pred) with dclip_upsample_silog's arithmetic,
 * r = p - target, e = |r|, T = #M, T' = max(T, 1), d as in dclip_upsample_silog:
 *     silog = sum d^2 / T' - lambd (sum d)^2 / T'^2
 *     l1    = sum e / T'
 *     berhu = sum b(e) / T',  b(e) = e if e <= c, else (e^2 + c^2) / (2 c),  c = threshold * max_M e
 *             (c = 0 without a pixel).  c is a constant of the CALL (Laina et al.): no gradient flows through
 *             the maximum, and the maximum is over this call's pixels only, hence per rank and per
 *             micro-batch when the caller splits a batch.
 *   dclip_upsample_depth_stats: terms is a bit set of DCLIP_DEPTH_*.  stats (f64[6]) = (sum d, sum d^2, T,
 *       sum e, max e, unused): the sums are accumulated (+=), the maximum is max(start, .), T always, sum d
 *       and sum d^2 with SILOG, sum e with L1 or BERHU, max e with BERHU; every other slot comes back as it
 *       went in.  max e is an f32 value held exactly.
 *   dclip_upsample_depth_finish: terms is the set `stats` was built for; a non-zero weight needs its bit.
 *       Weights finite and >= 0, at least one > 0; 0 < threshold <= 1 with a BerHu weight.  stats is read
 *       only.  berhu_sum (f64[1]) += sum b(e): required with w_berhu > 0, null otherwise.  grad (f32,
 *       B*h*w, accumulated, or null for the forward-only form) += up^T of
 *           w_silog * dclip_upsample_silog's pass-1 expression + w_l1 * sign(r) / T'
 *           + w_berhu * (sign(r) / T' if e <= c else r / (c T'))        on M, sign(0) = 0,
 *       so c = 0 never divides, and with T = 0 every element comes back bitwise as it went in.
 * NaN follows dclip_upsample_silog's rule: one NaN among the in-mask resized predictions or targets makes
 * sum e, max e (the maximum is a select that keeps a NaN) and sum b(e) NaN; T counts the pixel all the same;
 * masked-out targets may hold anything.
 * ws: the caller's scratch of dclip_upsample_depth_loss_ws_floats(B, h, w) floats, 8-byte aligned, contents
 * undefined on entry.  Per-workgroup records and gradient tiles, folded in a fixed order by short launches:
 * no float atomics, two runs are bitwise equal.  Stream-ordered: one ws per call in flight.          */
#define DCLIP_DEPTH_SILOG 1
#define DCLIP_DEPTH_L1 2
#define DCLIP_DEPTH_BERHU 4
int64_t dclip_upsample_depth_loss_ws_floats(int B, int h, int w);
int dclip_upsample_depth_stats(int low_dt, const void* pred, int B, int h, int w, const float* target,
                               const uint8_t* mask, int H, int W, float eps, int terms, double* stats, float* ws,
                               void* stream);
int dclip_upsample_depth_finish(int low_dt, const void* pred, int B, int h, int w, const float* target,
                                const uint8_t* mask, int H, int W, float eps, float lambd, int terms, float w_silog,
                                float w_l1, float w_berhu, float threshold, const double* stats, double* berhu_sum,
                                float* grad, float* ws, void* stream);

/* Fused bilinear upsample (align_corners=False) + evaluation of the heads, forward only: the
 * reference's validate() (train_denseclip.py:294-684: resize :461-467, CE :497, argmax :582, masked
 * RMSE :589-593) with compute_segmentation_metrics (denseclip/utils.py:109-139) and
 * compute_depth_errors (utils/depth_metrics.py:12-88), without materialising the resized tensors.
 * H >= h, W >= w, B*H*W < 2^31.  Additive to ABI 7.
 *   dclip_upsample_eval_seg:  logits (B, K, h, w) low_dt, K == 19.  pred (nullable): u8 (B, H, W)
 *       argmax class ids, the lowest index among equal maxima.  labels (nullable): (B, H, W)
 *       int64 / int32 / uint8 (lab_dt 0 / 1 / 2); pixels whose label is ignore_index or outside
 *       [0, K) are skipped.  With labels: cm (i64, K x K, row = target, column = prediction)
 *       += the pixel counts, loss_sum (f64[1]) += sum of -log softmax(up(logits))[label],
 *       count (u64[1]) += #valid.  Without labels cm, loss_sum and count must be null (pred only;
 *       ws unused).
 *   dclip_upsample_eval_depth: pred (B, 1, h, w) low_dt; target f32 (B, H, W); mask u8 (B, H, W) or
 *       null (all valid).  up (nullable): f32 (B, H, W) resized prediction.  sums (f64[12]) +=
 *       on mask && min_depth <= target <= max_depth, with p = clamp_pred ? clamp(up, min_depth,
 *       max_depth) : up, gt = target:
 *         [0] n  [1] sum (gt-p)^2  [2] sum (log gt - log p)^2  [3] sum |gt-p|/gt  [4] sum (gt-p)^2/gt
 *         [5..7] #(max(gt/p, p/gt) < 1.25, 1.25^2, 1.25^3)
 *       on mask alone, with the unclamped up:
 *         [8] n_mask  [9] sum (gt-up)^2  [10] sum d  [11] sum d^2,  d as in dclip_upsample_silog.
 * ws: the caller's scratch of dclip_upsample_eval_ws_bytes(B, K, h, w) bytes (K = 1 for depth; a
 * function of its arguments alone), 8-byte aligned, contents undefined on entry.  Integer counts
 * are exact; every floating sum has f32 per-pixel terms summed in f64 in a fixed order
 * (per-workgroup partials in ws, folded in workgroup order by a second launch): two runs are
 * bitwise equal.  No atomics on global memory.  Stream-ordered: one ws per call in flight.  */
int64_t dclip_upsample_eval_ws_bytes(int B, int K, int h, int w);
int dclip_upsample_eval_seg(int low_dt, const void* logits, int B, int K, int h, int w, const void* labels,
                            int lab_dt, int H, int W, int ignore_index, uint8_t* pred, int64_t* cm,
                            double* loss_sum, unsigned long long* count, void* ws, void* stream);
int dclip_upsample_eval_depth(int low_dt, const void* pred, int B, int h, int w, const float* target,
                              const uint8_t* mask, int H, int W, float min_depth, float max_depth, int clamp_pred,
                              float eps, float* up, double* sums, void* ws, void* stream);

/* The three fused paths above for any class count 1 <= K <= DCLIP_CLASSES_MAX = 256 (csrc/classes.hip; additive to ABI 7).
 * The 19-class entry points keep a pixel's K values in registers and the K-channel patch in LDS; these
 * walk the classes in chunks of 16, so neither grows with K.  Arguments and semantics are those of the
 * counterpart unless noted; any other K is rejected before a launch.
 *   dclip_score_map_classes:  dclip_score_map with the class embeddings in 32-row tiles: the same
 *       normalisation, eps rule (an all-zero pixel row scores 0), strided rows and fixed-order norms.
 *   dclip_upsample_ce_classes:  dclip_upsample_ce.  ignore_index is tested before the range [0, K), so
 *       K = 256 with ignore 255 skips the label 255.  An int64 label that no int32 holds is out of range.
 *       ws: dclip_upsample_ce_classes_ws_floats(B, K, h, w) floats, 8-byte aligned, contents undefined
 *       on entry; at most 3x the gradient's bytes + 1 MiB wherever K * w >= 4 (below that the 16
 *       bytes of loss partials per low-res row and 32-column chunk weigh more than the gradient
 *       itself: 6x at K = w = 1).  No atomics; bitwise reproducible.
 *   dclip_upsample_eval_seg_classes:  dclip_upsample_eval_seg (pred u8, so a class id is at most 255).
 *       ws: dclip_upsample_eval_seg_classes_ws_bytes(B, K, h, w) bytes (<= 80 MiB), 8-byte aligned,
 *       contents undefined on entry.  The confusion counts are added to u32 histograms in ws with integer
 *       atomics (exact in any order); the CE sum has f32 terms summed in f64 in a fixed order: two runs
 *       are bitwise equal.                                                                            */
#define DCLIP_CLASSES_MAX 256
int dclip_score_map_classes(const void* v, int v_dt, int64_t bstride, int64_t row_off, int64_t ld, const float* t,
                            float* score, int B, int HW, int C, int K, float eps, void* stream);
int64_t dclip_upsample_ce_classes_ws_floats(int B, int K, int h, int w);
int dclip_upsample_ce_classes(int low_dt, const void* logits, int B, int K, int h, int w, const void* labels,
                              int lab_dt, int H, int W, int ignore_index, double* loss_sum, unsigned* count,
                              float* grad, float* ws, void* stream);
int64_t dclip_upsample_eval_seg_classes_ws_bytes(int B, int K, int h, int w);
int dclip_upsample_eval_seg_classes(int low_dt, const void* logits, int B, int K, int h, int w, const void* labels,
                                    int lab_dt, int H, int W, int ignore_index, uint8_t* pred, int64_t* cm,
                                    double* loss_sum, unsigned long long* count, void* ws, void* stream);

/* Backward of the score map (csrc/scoregrad.hip; additive to ABI 7), one kernel family for every
 * 1 <= K <= DCLIP_CLASSES_MAX.  With s[b,k,p] = <v_p / max(|v_p|, eps), t_k / max(|t_k|, eps)> and the upstream
 * ds (B, K, HW) f32, every element multiplied by `scale` on load (a trainer passes 1 / tau):
 *     rv = 1 / max(|v_p|, eps), vn = v rv          rt = 1 / max(|t_k|, eps), tn = t rt
 *     dvn_p = sum_k ds[k,p] tn_k                   dtn_k = sum_p ds[k,p] vn_p
 *     dv_p = rv (dvn_p - a_p vn_p <vn_p, dvn_p>)   dt_k = rt (dtn_k - a_k tn_k <tn_k, dtn_k>)
 * a = 1 where the norm is >= eps and 0 where the clamp is active: autograd of F.normalize; an all-zero row
 * gets dvn / eps (dtn / eps), finite in f32 for eps = 1e-12 and gradients of ordinary size.
 * v: the forward's strided 16-bit pixel rows, read in place.  dv: image b's pixel p at dv + b*dv_bstride +
 * (dv_row_off + p)*dv_ld, dv_dt F32 or v_dt; only the B*HW pixel rows are written (CLS rows of a token
 * buffer and anything past HW keep their contents).  dt (B, K, C) f32 is overwritten, never accumulated into.
 * No 16-bit rounding before the stores: the sums over classes and pixels are f32 FMAs, the norms, rv / rt and
 * the two projections (differences of nearly equal terms) f64.  dt's sum over pixels goes through
 * per-workgroup partials in ws (dclip_score_map_bwd_ws_floats(B, HW, C, K) floats, 16-byte aligned, contents
 * undefined on entry) folded in a fixed order: no float atomics, the grid depends on the shapes alone, two
 * runs are bitwise equal.  C % 16 == 0, C <= 2048, 16-byte aligned rows of v and dv, t and dt 16-byte
 * aligned, B <= 65535.  Stream-ordered: one ws per call in flight.                                      */
int64_t dclip_score_map_bwd_ws_floats(int B, int HW, int C, int K);
int dclip_score_map_bwd(const void* v, int v_dt, int64_t bstride, int64_t row_off, int64_t ld, const float* t,
                        const float* ds, float scale, void* dv, int dv_dt, int64_t dv_bstride, int64_t dv_row_off,
                        int64_t dv_ld, float* dt, float* ws, int B, int HW, int C, int K, float eps, void* stream);

/* dclip_upsample_ce / dclip_upsample_ce_classes with F.cross_entropy's other arguments (csrc/celossopt.hip;
 * additive to ABI 7), for every 1 <= K <= DCLIP_CLASSES_MAX: K = 19 keeps a pixel's values in registers, any
 * other K walks the classes in chunks of 16.  For a valid pixel p (label t != ignore_index, tested first, and
 * in [0, K)), u = up(logits)_p, P = softmax(u), w = class_weight (all 1 when null), Wsum = sum_k w_k,
 * e = label_smoothing, q_p = pixel_weight[p] (1 when null; any finite float):
 *     l_p      = (1 - e) w_t (-log P_t) + (e / K) sum_k w_k (-log P_k)
 *     dl_p/du  = (1 - e) w_t (P - onehot_t) + (e / K) (P Wsum - w)
 *     sums[0] += sum_p q_p l_p    sums[1] += sum_p q_p w_t    count += #valid (q plays no part)
 *     pixel_loss[p] = l_p (without q_p); 0 at a pixel that is not valid (every element is written)
 *     grad    += up^T(q_p dl_p/du)   (un-normalised and accumulated, as dclip_upsample_ce)
 * sums[0] / sums[1] is F.cross_entropy(weight=w, label_smoothing=e, reduction="mean"); pixel_loss is
 * reduction="none".  grad == null: forward only (no gradient pass, no tiles, no merge).  pixel_loss, and
 * sums with count (both or neither), may be null; at least one output is required.  0 <= e < 1;
 * B*H*W < 2^31.  With all-one weights, e = 0 and no pixel_weight, sums[0], count and grad are bitwise those
 * of dclip_upsample_ce (K = 19) / dclip_upsample_ce_classes.
 * ws: dclip_upsample_ce_opt_ws_floats(B, K, h, w) floats, 8-byte aligned, contents undefined on entry.  The
 * same fixed summation orders, per-workgroup tiles and partials, merge and sums launches: no atomics, and
 * sums, count, grad and pixel_loss repeat bit for bit.  Stream-ordered: one ws per call in flight.       */
int64_t dclip_upsample_ce_opt_ws_floats(int B, int K, int h, int w);
int dclip_upsample_ce_opt(int low_dt, const void* logits, int B, int K, int h, int w, const void* labels,
                          int lab_dt, int H, int W, int ignore_index, const float* class_weight,
                          float label_smoothing, const float* pixel_weight, float* pixel_loss, double* sums,
                          unsigned* count, float* grad, float* ws, void* stream);

/* Multi-scale + flip test-time ensembling fused into the evaluation above (the reference's aug_test,
 * denseclip.py:1005-1041 with test.py:91-96, without materialising one resized tensor per view).
 * A view is a low-res map (B, K, h, w) of low_dt (one dtype, B and K for all views) and a flip flag;
 * `views` is a HOST array of nviews (1 .. DCLIP_ENSEMBLE_MAX_VIEWS) entries, copied into the kernel
 * arguments by the call (no device-side table, no copy: capturable).  Per output pixel (y, x), for
 * every view in the order given, u_v = the bilinear resize (align_corners=False, the arithmetic of
 * dclip_upsample_eval_*) of view v at (y, x_v), x_v = x for a plain view and W-1-x for a flipped one
 * (the view's resized map mirrored back, F.interpolate(...).flip(-1)); the u_v are accumulated in f32
 * in view order and scaled by 1/nviews.  h_v <= H, w_v <= W, B*H*W < 2^31.  Additive to ABI 7.
 *   dclip_ensemble_eval_seg: K == 19.  average 0 ("logits", the reference's rule): the mean of the
 *       u_v; CE = -log softmax(mean)[label].  average 1 ("probs", mmseg's rule): the mean of
 *       softmax_K(u_v); CE = -log(mean[label]).  pred / labels / cm / loss_sum / count as
 *       dclip_upsample_eval_seg, taken from the mean (argmax: the lowest index among equal maxima).
 *   dclip_ensemble_eval_depth: views (B, 1, h, w).  up (nullable): f32 (B, H, W), the mean of the
 *       resized, mirrored-back predictions; sums (f64[12]) += the sums of dclip_upsample_eval_depth
 *       evaluated on that mean.  target null: prediction only (up required; mask, sums and ws unused).
 * ws: dclip_ensemble_eval_ws_bytes(B, K, nviews) bytes (K = 1 for depth; a function of its arguments
 * alone), 8-byte aligned, contents undefined on entry.  Reductions as dclip_upsample_eval_*: exact
 * counts, f64 sums in a fixed order, two runs bitwise equal, no atomics on global memory.  The fused
 * multiply-adds of the interpolation are spelled out so that a source column always goes through
 * the same roundings: a flipped view gives exactly the column mirror of the same map unflipped.
 * One plain view with average 0 gives the class map, confusion matrix and count of
 * dclip_upsample_eval_seg and, bitwise, the up and sums of dclip_upsample_eval_depth (its CE sum
 * is not bitwise dclip_upsample_eval_seg's: the resized logits may differ in their last bits).  */
#define DCLIP_ENSEMBLE_MAX_VIEWS 16
typedef struct {
    const void* low;
    int h, w, flip;
} dclip_view;
int64_t dclip_ensemble_eval_ws_bytes(int B, int K, int nviews);
int dclip_ensemble_eval_seg(int low_dt, const dclip_view* views, int nviews, int B, int K, int average,
                            const void* labels, int lab_dt, int H, int W, int ignore_index, uint8_t* pred,
                            int64_t* cm, double* loss_sum, unsigned long long* count, void* ws, void* stream);
int dclip_ensemble_eval_depth(int low_dt, const dclip_view* views, int nviews, int B, const float* target,
                              const uint8_t* mask, int H, int W, float min_depth, float max_depth, int clamp_pred,
                              float eps, float* up, double* sums, void* ws, void* stream);

/* Sliding-window inference fused into the evaluation above (test_cfg mode='slide' of the reference's
 * ViT configs; the rule is mmseg's slide_inference, which the reference tree only names), without
 * the image-sized (B, K, H, W) accumulator and count map.  The caller runs the model on crops
 * img[:, :, y0:y0+wh, x0:x0+ww] of one size wh x ww; a window is the crop's low-res map (B, K, h, w)
 * of low_dt (one dtype, B, K, h and w for all windows) and its origin (y0, x0) in the H x W image.
 * mmseg places them, for crop_size (ch, cw) and stride (sh, sw), at
 *     h_grids = max(H - ch + sh - 1, 0) / sh + 1        (w_grids likewise)
 *     window (i, j), i-major:  y2 = min(i sh + ch, H), y0 = max(y2 - ch, 0)   (x0 likewise)
 * so wh x ww = min(ch, H) x min(cw, W) and the last window of a row or column is shifted back, not
 * shrunk; any table that covers every pixel is accepted.  `wins` is a HOST array of nwin
 * (1 .. DCLIP_SLIDE_MAX_WINDOWS) entries, copied into the kernel arguments by the call (no
 * device-side table, no copy: capturable).  Per output pixel (y, x), for every window that covers it,
 * in the order given, u = the bilinear resize (align_corners=False, the arithmetic of
 * dclip_ensemble_eval_*) of the window's map to wh x ww at (y - y0, x - x0); the u are accumulated in
 * f32 in table order and the result is sum / count, one correctly rounded division: a pixel that one
 * window covers holds exactly that window's resized value.
 * h <= wh <= H, w <= ww <= W, 0 <= y0 <= H - wh, 0 <= x0 <= W - ww, B*H*W < 2^31, and every pixel
 * covered by at least one window (checked on the host; the message names the first uncovered pixel).
 * Additive to ABI 7.
 *   dclip_slide_eval_seg: K == 19.  CE = -log softmax(result)[label].  pred / labels / cm / loss_sum /
 *       count as dclip_upsample_eval_seg, taken from the result (argmax: the lowest index among equal
 *       maxima).  Without labels cm, loss_sum and count must be null (pred only; ws unused).
 *   dclip_slide_eval_depth: windows (B, 1, h, w).  up (nullable): f32 (B, H, W), the mean of the
 *       covering windows' resized predictions; sums (f64[12]) += the sums of
 *       dclip_upsample_eval_depth evaluated on that mean.  target null: prediction only (up required;
 *       mask, sums and ws unused).
 * ws: dclip_slide_eval_ws_bytes(B, K, nwin) bytes (K = 1 for depth; a function of its arguments
 * alone), 8-byte aligned, contents undefined on entry.  Reductions as dclip_upsample_eval_*: exact
 * counts, f64 sums in a fixed order, two runs bitwise equal, no atomics on global memory.  One window
 * covering the image gives, bitwise, what dclip_ensemble_eval_* gives for one plain view of the same
 * map; a window's depth values are those of dclip_upsample_eval_depth on its map at the window's
 * size, wherever the window lies (the roundings follow the window-local column).  */
#define DCLIP_SLIDE_MAX_WINDOWS 64
typedef struct {
    const void* low;
    int y0, x0;
} dclip_window;
int64_t dclip_slide_eval_ws_bytes(int B, int K, int nwin);
int dclip_slide_eval_seg(int low_dt, const dclip_window* wins, int nwin, int B, int K, int h, int w, int wh, int ww,
                         const void* labels, int lab_dt, int H, int W, int ignore_index, uint8_t* pred, int64_t* cm,
                         double* loss_sum, unsigned long long* count, void* ws, void* stream);
int dclip_slide_eval_depth(int low_dt, const dclip_window* wins, int nwin, int B, int h, int w, int wh, int ww,
                           const float* target, const uint8_t* mask, int H, int W, float min_depth, float max_depth,
                           int clamp_pred, float eps, float* up, double* sums, void* ws, void* stream);

/* Sliding windows inside multi-scale + flip ensembling: mmseg's aug_test -> inference ->
 * slide_inference, what the reference's ViT configs (test_cfg mode='slide') run under test.py
 * --aug-test, without any per-view tensor (no (B, K, Hv, Wv) accumulator, count map, resized or
 * softmax copy).  View v is the image resized to Hv x Wv (Hv > H allowed) and mirrored when flip; it
 * is evaluated with the windows wins[first .. first + nwin) of one size wh x ww in the VIEW's
 * coordinates, each a low-res map (B, K, h, w) of low_dt (one h x w per view; one dtype, B and K for
 * the call) at origin (y0, x0) of the view.  Per output pixel (y, x), for every view in the order given:
 *   S_v, the view's slide result, is per view pixel what dclip_slide_eval_* computes on an Hv x Wv
 *       image: the resizes of the covering windows' maps to wh x ww, accumulated in f32 in table
 *       order, and one correctly rounded division by their number;
 *   U_v = the bilinear resize (align_corners=False, plain 4 taps, no antialiasing; the fused
 *       multiply-adds of dclip_ensemble_eval_seg) of S_v to H x W at (y, x_v), x_v = x for a plain
 *       view and W-1-x for a flipped one; (Hv, Wv) == (H, W): U_v = S_v(y, x_v), no arithmetic;
 *   the U_v (average 0, "logits") or softmax_K(U_v) (average 1, "probs", mmseg's rule here) are
 *       accumulated in f32 in view order and scaled by 1/nviews, CE as dclip_ensemble_eval_seg; the
 *       depth is always the mean of the U_v.
 * pred / labels / cm / loss_sum / count / up / sums / target / mask are dclip_slide_eval_*'s, taken
 * from that mean; without labels cm, loss_sum and count must be null (pred required); without a
 * target up is required.  Both tables are HOST arrays: nviews in 1 .. DCLIP_ENSEMBLE_MAX_VIEWS,
 * nwin_total in 1 .. DCLIP_SLIDE_TTA_MAX_WINDOWS.  The window table does not fit kernel arguments:
 * the call writes it into ws with small launches of its own (no copy, no pinned memory), so it
 * stays stream-ordered and capturable, and ws is ALWAYS required: dclip_slide_tta_eval_ws_bytes(B, K,
 * nviews, nwin_total) bytes (K = 1 for depth; a function of its arguments alone), 8-byte aligned,
 * contents undefined on entry.  Checked on the host before any launch: K == 19; h <= wh <= Hv,
 * w <= ww <= Wv, 0 <= y0 <= Hv - wh, 0 <= x0 <= Wv - ww; every view pixel covered (the message names
 * the view and its first uncovered pixel); B*H*W and B*Hv*Wv < 2^31; a window's patch under one
 * output tile within the kernel's LDS (views up to a few times the image).  Reductions as
 * dclip_upsample_eval_*: exact counts, f64 sums in a fixed order, two runs bitwise equal, no atomics on
 * global memory.  Additive to ABI 7.  Degenerate cases, bitwise:
 *   one plain view at the image's size = dclip_slide_eval_* on the same windows (pred, cm, count;
 *       up and the 12 depth sums; the CE sum only to rounding, its summation order differs);
 *   views at the image's size with one window over the whole view each = dclip_ensemble_eval_* on
 *       the same maps (likewise);
 *   a flipped view = the column mirror of the same view unflipped.  */
#define DCLIP_SLIDE_TTA_MAX_WINDOWS 1024 /* total over the views; views <= DCLIP_ENSEMBLE_MAX_VIEWS */
typedef struct {
    int Hv, Wv, flip, wh, ww, h, w, first, nwin; /* wins[first .. first+nwin) */
} dclip_slide_view;
int64_t dclip_slide_tta_eval_ws_bytes(int B, int K, int nviews, int nwin_total);
int dclip_slide_tta_eval_seg(int low_dt, const dclip_slide_view* views, int nviews, const dclip_window* wins,
                             int nwin_total, int B, int K, int average, const void* labels, int lab_dt, int H, int W,
                             int ignore_index, uint8_t* pred, int64_t* cm, double* loss_sum,
                             unsigned long long* count, void* ws, void* stream);
int dclip_slide_tta_eval_depth(int low_dt, const dclip_slide_view* views, int nviews, const dclip_window* wins,
                               int nwin_total, int B, const float* target, const uint8_t* mask, int H, int W,
                               float min_depth, float max_depth, int clamp_pred, float eps, float* up, double* sums,
                               void* ws, void* stream);

/* Cityscapes depth + segmentation batch preparation (datasets/cityscapes_depth_seg.py:129-170,
 * 218 and the trainer's RandomCrop / HorizontalFlip / Normalize / ToTensorV2,
 * train_denseclip.py:143-149).  Inputs: decoded planes of B images of H x W — img uint8
 * (B, H, W, 3) RGB, ids uint8 (B, H, W) Cityscapes label ids, disp uint16 (B, H, W) disparity;
 * crop int32 (B, 3) = (y0, x0, flip) per image, window [y0, y0 + h) x [x0, x0 + w) inside the
 * image (mirrored when flip != 0).  Outputs for the h x w crops: out_img (B, 3, h, w) out_dt
 * = (x - 255 mean) * (1 / (255 std)); out_seg int64 (B, h, w) train ids (ids >= 34 -> 255);
 * out_depth f32 (B, h, w) = bf / ((d - 1) / 256 + 1e-6) where d > 0, (d - 1) / 256 > 1e-3 and
 * the depth <= depth_max, else 0; out_mask uint8 (B, h, w) = depth > 0.  All device pointers
 * (mean, stdv: 3 host floats).                                                          */
int dclip_cityscapes_prepare(const uint8_t* img, const uint8_t* ids, const uint16_t* disp, int B, int H, int W,
                             const int* crop, int h, int w, const float* mean, const float* stdv, float bf,
                             float depth_max, void* out_img, int out_dt, int64_t* out_seg, float* out_depth,
                             uint8_t* out_mask, void* stream);

/* dclip_cityscapes_prepare with the trainer's whole spatial pipeline in front of the crop
 * (train_denseclip.py:138-149): RandomScale -> PadIfNeeded -> RandomCrop -> HorizontalFlip.
 * params int32 (B, 7) on the device = (Hs, Ws, pad_top, pad_left, y0, x0, flip) per image: the
 * image is resized to Hs x Ws (cv2 INTER_CUBIC on uint8, the flag the reference's
 * interpolation=Image.BILINEAR (= 2) selects; label ids and disparity INTER_NEAREST), padded by
 * pad_top / pad_left (image 0, seg 255, depth 255 -> mask 1, as PadIfNeeded(value=0,
 * mask_value=255) followed by the reference's depth > 0 validity), and the h x w window at
 * (y0, x0) of the padded image is taken (mirrored when flip).  Same outputs as
 * dclip_cityscapes_prepare; identity params (H, W, 0, 0, y0, x0, flip) give its result.   */
int dclip_cityscapes_augment(const uint8_t* img, const uint8_t* ids, const uint16_t* disp, int B, int H, int W,
                             const int* params, int h, int w, const float* mean, const float* stdv, float bf,
                             float depth_max, void* out_img, int out_dt, int64_t* out_seg, float* out_depth,
                             uint8_t* out_mask, void* stream);

/* ADE20K batch preparation (the reference's datasets/ade20k.py:57-185 per sample; csrc/dataade.hip).
 * img: the decoded uint8 RGB (H, W, 3) images of B samples of any sizes, packed into one device buffer of
 * img_bytes; lab: their uint8 (H, W) raw label planes (0 .. 150), packed likewise, lab_bytes.  geom: int64
 * (B, DCLIP_ADE_GEOM_WORDS) on the device, geom_host the same table on the host; per image
 *   0 img_off, 1 lab_off   byte offsets of its planes in img / lab
 *   2 H0, 3 W0             the decoded size
 *   4 H1, 5 W1             after the first resize (int(H s), int(W s) of the random scale s)
 *   6 H2, 7 W2             after the second resize (ade20k.py:97-118; = H1, W1 without one)
 *   8 y0, 9 x0             the crop's origin in the H2 x W2 image, window [y0, y0 + h) x [x0, x0 + w) inside it
 *   10 flip                != 0: the crop mirrored horizontally (an extension; the reference never flips)
 *   11                     reserved, 0
 * Each resize is PIL's on 8-bit planes: BILINEAR for the image (separable, horizontal pass first, each pass
 * rounded to uint8: out = clip(((1 << 21) + sum px k) >> 22) with k = int(0.5 + weight 2^22) from f64 triangle
 * weights over [xmin, xmax) = int(center -+ support + 0.5), support = max(in / out, 1); a pass between equal
 * sizes is skipped) and NEAREST for the labels (source index int(xo), xo = a / 2 then one `xo += a` per
 * output coordinate, a = in / out).  Outputs: out_img (B, 3, h, w) out_dt = (float32(u8) / 255 - mean) / std
 * evaluated in f64 (mean, stdv: 3 host doubles), or with out_dt DCLIP_U8 the uint8 crop itself in the same
 * layout; out_seg int64 (B, h, w) = v - 1 for v > 0, ignore_label for 0 (ignore_label < 0: v unchanged).
 * ws: dclip_ade20k_prepare_ws_bytes(geom_host, B, h, w) bytes (ws_bytes: what the caller holds), 16-byte
 * aligned; -1 from the query: bad geometry (dclip_last_error).  Every geometry entry is validated on the host
 * before any launch (sizes >= 1, window inside the image, planes inside the packed buffers, workspace size);
 * the kernels repeat the checks on the device copy and skip an image whose row fails them.  No host
 * synchronisation, no atomics: capturable, and two runs are bitwise equal.  Launch sizes follow geom_host: a
 * captured call replays for device tables of the same geometry.                                          */
#define DCLIP_ADE_GEOM_WORDS 12
int64_t dclip_ade20k_prepare_ws_bytes(const int64_t* geom_host, int B, int h, int w);
int dclip_ade20k_prepare(const uint8_t* img, int64_t img_bytes, const uint8_t* lab, int64_t lab_bytes,
                         const int64_t* geom, const int64_t* geom_host, int B, int h, int w, const double* mean,
                         const double* stdv, int ignore_label, void* out_img, int out_dt, int64_t* out_seg, void* ws,
                         int64_t ws_bytes, void* stream);

/* ColorJitter (albumentations, train_denseclip.py:152-155; `color_jitter: true`) in place on a
 * uint8 HWC batch img (B, h, w, 3) RGB: params (B, 8) f64 on the device = brightness, contrast,
 * saturation, hue factors and the order of the four (0 brightness, 1 contrast, 2 saturation,
 * 3 hue) per image; identity factors (1, 1, 1, 0) leave an image untouched.  uint8 arithmetic of
 * albumentations' *_torchvision functions and OpenCV's 8-bit RGB<->GRAY / HSV conversions.
 * ws: B uint64 (per-image gray sums for the contrast mean).                             */
int dclip_color_jitter(uint8_t* img, int B, int h, int w, const double* params, unsigned long long* ws,
                       void* stream);

/* Normalize + ToTensorV2 of a uint8 HWC batch (B, h, w, 3): out (B, 3, h, w) out_dt =
 * (x - 255 mean) * (1 / (255 std)) (mean, stdv: 3 host floats).                           */
int dclip_normalize_u8(const uint8_t* img, int B, int h, int w, const float* mean, const float* stdv, void* out,
                       int out_dt, void* stream);

/* Element-wise dtype conversion of n elements: out = (out_dt)(in * scale), times *scale_ptr
 * when non-null (read on the device).  A power-of-two scale keeps fp16 gradients out of the
 * subnormal range (see dclip_grad_scale and dclip_gemm's alpha).                      */
int dclip_cast(const void* in, int in_dt, void* out, int out_dt, int64_t n, float scale,
               const float* scale_ptr, void* stream);

/* Eval-mode BatchNorm2d (+ ReLU when relu != 0) from the running statistics, on the same rows
 * as dclip_bn_fwd: y = x * w / sqrt(running_var + eps) + (b - running_mean * that scale), f32
 * arithmetic, 16-bit I/O.  ws: dclip_bn_workspace(rows, C) floats.  (nn.BatchNorm2d.eval() of
 * the neck's ConvModules and the FCN heads, models.py:13-20.)                            */
int dclip_bn_eval(int dt, const void* x, int64_t rows, int C, int64_t ld, const float* w, const float* b, float eps,
                  const float* running_mean, const float* running_var, float* ws, void* y, int relu, void* stream);

/* Stochastic depth (drop_path, reference models.py:257-268, 291-294 on the LND layout: one keep
 * value per token position): out[r][c] = (x ? x[r][c] : 0) + s[r % ntok] * y[r][c], f32
 * (rows, cols) row-major, rows a multiple of ntok, cols % 4 == 0; out may alias x or y. */
int dclip_row_scale_add(const float* x, const float* y, const float* s, int ntok, float* out, int64_t rows,
                        int cols, void* stream);

/* Power-of-two scale for the fp16 cast of an f32 gradient g (n elements, 16-byte aligned),
 * computed on the device: ws[0] = s = 2^clamp(floor(log2(target / max|g|)), -60, 60),
 * ws[1] = 1/s (s = 1 when max|g| is 0 or not finite).  ws: 4 floats, ws[2..3] zero on entry
 * (left zero on exit, so one buffer serves successive calls on a stream).  Pass ws to
 * dclip_cast / dclip_tokens_bwd as scale_ptr and ws + 1 to dclip_gemm / dclip_gemm_tn as
 * alpha_ptr.  (No reference counterpart: the reference trains in fp32.)              */
int dclip_grad_scale(const float* g, int64_t n, float target, float* ws, void* stream);
/* Read-out gradient folded into a block's incoming gradient (replaces the autograd sum of the
 * two uses of a block output, models.py:565 -> 577-597, plus the backward's cast): sum = a + b
 * with b's CLS rows (row % ntok == 0) read as 0, lp = (lp_dt)(sum * scale).  a, sum: f32
 * (rows, cols); b: (rows, cols) token buffer, f32/bf16/f16; cols % 8 == 0; sum may alias a. */
int dclip_add_readout_cast(const float* a, const void* b, int b_dt, float* sum, void* lp, int lp_dt,
                           int64_t rows, int cols, int ntok, float scale, void* stream);

/* The fp16 backward's form of the same fold: sum = a + b * (*b_scale_ptr, or 1 when null) with
 * b's CLS rows read as 0, and in the same pass ws = the dclip_grad_scale pair (s, 1/s, 0, 0) of
 * sum for its fp16 cast (ws zeroed before first use, left reusable).  b_scale_ptr: the 1/s entry
 * of the fp16 heads' gradient scale (the map gradient arrives scaled).  cols % 8 == 0.      */
int dclip_add_readout_amax(const float* a, const void* b, int b_dt, const float* b_scale_ptr, float* sum,
                           int64_t rows, int cols, int ntok, float target, float* ws, void* stream);

/* DELAYED-scale fp16 casts of the backward's block gradients (the fp16 line; replaces a
 * dclip_grad_scale + dclip_cast pair, or dclip_add_readout_amax + dclip_cast, per block branch).
 * st: the state of one gradient site, DCLIP_DS_STATE_FLOATS floats that persist across training
 * steps (3 x 64 shards of |x|-maximum bits, then 3 used scales); `use` counts the site's calls
 * from 1.  Call k casts with s = 2^clamp(floor(log2(target / max_{k-1})), -60, 60), the scale of
 * call k-1's own maximum (call k-1's scale again when that maximum was 0 or not finite), writes
 * (s, 1/s) to spair (2 floats: what the consumers of lp unscale by) and records its maximum in st
 * for call k+1 — no fences, no arrival counter.  Seeding for call 1 (after an exact two-pass cast
 * with scale s0): st all zero except st[0] = target / s0 and st[192] = s0.  A gradient that grew
 * by more than 65504 / target between two calls overflows to inf in lp (the fp16 train step
 * then checks its gradients and skips, train.step_unless_nonfinite).  (No reference
 * counterpart: the reference trains in fp32.)
 *   dclip_add_readout_cast_scaled: sum = a (+ b * (*b_scale_ptr), b's CLS rows read as 0; b may be
 *     null, then sum is not written), lp = (f16)(sum * s).  models.py:565 -> 577-597 as
 *     dclip_add_readout_cast.  cols % 8 == 0.
 *   dclip_layernorm_bwd_scaled: dclip_layernorm_bwd_res with an f32 x, dy f32 or (ABI 6) f16 on
 *     dy_scale, and lp = (f16)(dx * s) (models.py:243-249 backward).  cols in {512, 768, 1024}. */
#define DCLIP_DS_STATE_FLOATS 196
int dclip_add_readout_cast_scaled(const float* a, const void* b, int b_dt, const float* b_scale_ptr, float* sum,
                                  void* lp, int64_t rows, int cols, int ntok, float target, float* st, int use,
                                  float* spair, void* stream);
int dclip_layernorm_bwd_scaled(const void* dy, int dy_dt, const float* dy_scale, const void* x, int x_dt,
                               const float* w, const float* mean, const float* rstd, const float* res, float* dx,
                               void* lp, float* dw, float* db, float* ws, int64_t rows, int64_t cols, float target,
                               float* st, int use, float* spair, void* stream);

/* LayerNorm backward of a block's ln_1 with the PREVIOUS block's read-out map gradient folded in
 * (models.py:243-249 backward + the models.py:565 -> 577-597 read-out's gradient):
 *   dx = (res + LN^T(dy)) + add,  lp = (lp_dt) dx
 * add: a bf16 (rows, cols) token buffer whose rows with row % ntok == 0 (CLS) read as 0.  One pass
 * in place of dclip_layernorm_bwd_res + dclip_add_readout_cast (bitwise their result: the same
 * fp32 additions in the same order).  dy f32 or bf16, x f32, cols in {512, 768, 1024}; lp required.
 * dw / db accumulate as in dclip_layernorm_bwd_res (may be NULL). */
int dclip_layernorm_bwd_add(const void* dy, int dy_dt, const float* x, const float* w, const float* mean,
                            const float* rstd, const float* res, const void* add, int ntok, float* dx, void* lp,
                            int lp_dt, float* dw, float* db, float* ws, int64_t rows, int64_t cols, void* stream);
/* The fp16 backward's form: dclip_layernorm_bwd_scaled (dy f32 or f16 on dy_scale, f32 x, lp = (f16)(dx * s) on the
 * delayed scale of st's use `use`, (s, 1/s) to spair) with dx = (res + LN^T(dy)) + add * (*add_scale)
 * (add: f16 or bf16 (add_dt), CLS rows read as 0; add_scale may be NULL = 1) — in place of
 * dclip_layernorm_bwd_res + dclip_add_readout_cast_scaled on the same site state.  cols in
 * {512, 768, 1024}. */
int dclip_layernorm_bwd_scaled_add(const void* dy, int dy_dt, const float* dy_scale, const float* x,
                                   const float* w, const float* mean, const float* rstd, const float* res,
                                   const void* add, int add_dt, const float* add_scale, int ntok, float* dx,
                                   void* lp, float* dw, float* db, float* ws, int64_t rows, int64_t cols,
                                   float target, float* st, int use, float* spair, void* stream);

/* Train-mode BatchNorm2d (+ optionally the ReLU after it) on a channels-last 16-bit map viewed as
 * rows (B*H*W) of C channels at a row pitch of ld elements (ld = C for a whole map; larger for a
 * channel slice of a wider buffer, e.g. one level of the neck's concatenation).  Replaces
 * nn.BatchNorm2d + nn.ReLU in the neck's ConvModules (models.py:13-20) and the FCN heads;
 * torch.nn.functional.batch_norm semantics: biased batch variance for the normalisation,
 * unbiased for running_var, running = (1 - momentum) running + momentum batch.  C % 8 == 0,
 * C <= 2048, ld % 8 == 0.  w, b, running_mean / running_var may be NULL.  ws:
 * dclip_bn_workspace(rows, C) floats.  Forward: y = [relu](bn(x)) (same pitch as x), mean /
 * rstd (f32, C) for the backward.  Backward (relu: dy masked where bn(x) <= 0, recomputed from x):
 * dx (dt, same pitch) and, when non-null, dw / db (f32, C). */
int64_t dclip_bn_workspace(int64_t rows, int C);
int dclip_bn_fwd(int dt, const void* x, int64_t rows, int C, int64_t ld, const float* w, const float* b,
                 float eps, float momentum, float* running_mean, float* running_var, float* ws, float* mean,
                 float* rstd, void* y, int relu, void* stream);
/* gscale (nullable): dw and db are multiplied by *gscale (the 1/s entry of the fp16 heads'
 * gradient-scale pair; dx keeps the scale of dy).                                         */
int dclip_bn_bwd(int dt, const void* dy, const void* x, int64_t rows, int C, int64_t ld, const float* w,
                 const float* b, const float* mean, const float* rstd, float* ws, void* dx, float* dw,
                 float* db, int relu, const float* gscale, void* stream);

/* Multi-tensor AdamW step with global-norm clipping, gradient-accumulation scaling and a learning
 * rate read from device memory (optim.hip; train.FusedAdamW).  torch.optim.AdamW (decoupled weight
 * decay) + torch.nn.utils.clip_grad_norm_ + the non-finite check + dclip_weight_refresh, in two
 * passes over HBM; no atomics, bitwise reproducible.  An additive part of ABI 7.
 *
 * Descriptor: n entries of DCLIP_ADAMW_DESC_WORDS int64, on the device (desc, read by the kernels)
 * and, identical, on the host (desc_host, read by the entry points: launch geometry and checks):
 *   [0] p  [1] exp_avg m  [2] exp_avg_sq v   (f32, contiguous, numel = rows * cols)
 *   [3] plain 16-bit copy (rows, cols) or 0   [4] transposed 16-bit copy (cols, rows) or 0
 *   [5] rows  [6] cols  [7] first tile  [8] column tiles ceil(cols / 64), or 0: walked as flat
 *   chunks of 4096 elements (required to be non-zero with a transposed copy)
 *   [9] hyper-parameter row  [10] the copies' dtype (DCLIP_BF16 / DCLIP_F16)  [11] unused
 * Entry e covers tiles [first, first + (tiles of its walk)); `tiles` is their total.  Copies must
 * be 16-byte aligned; p, g, m, v take 16-byte accesses when all four are 16-byte aligned.
 * grads: n HOST pointers to the f32 gradients in entry order (NULL: the entry is skipped this step).
 * They are passed to the kernels as launch arguments, DCLIP_ADAMW_CHUNK entries per launch, so no
 * buffer of the caller's has to outlive the call.
 *
 * hp: n_rows device rows of DCLIP_ADAMW_HP_FLOATS f32, one per param group:
 *   lr, 1 - beta1, 1 - beta2, eps, weight_decay, max_norm (<= 0: no clipping), inv_accum, unused
 * (the complements of the betas: 1 - 0.999 keeps in fp32 the digits that 0.999 would lose).
 * The global norm and clip coefficient take max_norm and inv_accum from row 0.
 *
 * state: DCLIP_ADAMW_STATE_HEAD + n_rows * DCLIP_ADAMW_STATE_ROW_FLOATS device f32 the optimizer
 * owns (zeroed once; [3] persists):
 *   [0] total_norm  [1] clip coefficient  [2] found_inf (0 / 1)  [3] step count: the steps APPLIED
 *   [4] the count of the prepared step (prepare writes it, update commits it to [3]), then per row
 *   lr, lr*wd, lr/(1 - beta1^t), 1/sqrt(1 - beta2^t), 1 - beta1, beta2, 1 - beta2, eps, c, 3 unused.
 *
 * dclip_adamw_prepare: with_norm launches the partial sums (per element the exact fp64 square of
 * the fp32 gradient; per thread in element order, a fixed 64-lane butterfly, the 4 waves in order:
 * ONE fp64 partial per tile in ws, dclip_adamw_ws_bytes(tiles) bytes — a function of `tiles`
 * alone).  Always launches the one-workgroup fold: sum = the partials added in a fixed order (0
 * without the norm pass);
 *   found_inf  = 1 when sum is not finite or *found_inf (optional device f32) is non-zero
 *   total_norm = sqrt(sum) * inv_accum
 *   coef       = min(1, max_norm / (total_norm + 1e-6)) when max_norm > 0, else 1  (clip_grad_norm_)
 *   t          = [3] + 1 unless found_inf, to [4];  the bias corrections in fp64, stored as f32
 *                (preparing twice, or without an update, counts nothing)
 *   c          = coef * inv_accum (per row)
 * dclip_adamw_update: one workgroup per tile; writes NOTHING when found_inf is 1.  Otherwise tile
 * 0's workgroup commits the step count ([3] = [4]; nothing else reads [3] in this launch) and, fp32
 * per element in torch's AdamW order, the gradient never rewritten:
 *   g' = g c
 *   p  = p (1 - lr wd)                      [as p - (lr wd) p, one rounding]
 *   m  = m + (1 - beta1)(g' - m)
 *   v  = beta2 v + (1 - beta2) g'^2
 *   p  = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
 * and the copies are the cast of the new p, as dclip_weight_refresh writes them. */
#define DCLIP_ADAMW_DESC_WORDS 12
#define DCLIP_ADAMW_CHUNK 256
#define DCLIP_ADAMW_HP_FLOATS 8
#define DCLIP_ADAMW_STATE_HEAD 8
#define DCLIP_ADAMW_STATE_ROW_FLOATS 12
int64_t dclip_adamw_ws_bytes(int64_t tiles);
int dclip_adamw_prepare(const int64_t* desc, const int64_t* desc_host, const void* const* grads, int n,
                        int64_t tiles, const float* hp, int n_rows, const float* found_inf, float* state,
                        void* ws, int with_norm, void* stream);
int dclip_adamw_update(const int64_t* desc, const int64_t* desc_host, const void* const* grads, int n,
                       int64_t tiles, float* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCLIP_H */
