/*
 * vit_hip.h — C-ABI of libvit_hip.so, the MI355X (gfx950 / CDNA4) compute library behind the drop-in
 * `VisionTransformer` package (vision-transformer_amd/VisionTransformer).
 *
 * The reference (SiddhantSKarki/Vision-Transformer) has no FFI: its boundary is the torch.nn.Module API and every op
 * below replaces an ATen call site on the training hot path (SURVEY.md §2 table "ATen op call sites").  Each entry
 * point cites the reference line(s) whose arithmetic it replaces.
 *
 * Conventions (all entry points):
 *   - plain device pointers + int64 sizes; no torch types; dtype enums below;
 *   - `stream` is a hipStream_t passed as void*; every launch is asynchronous on it; no device sync, no allocation
 *     (callers own all buffers and workspaces — the PyTorch caching allocator in the host package);
 *   - return 0 on success, a nonzero vit_status on failure with a thread-local message in vit_last_error();
 *   - re-entrant; the only process-wide state is the option table of vit_set_option (below), whose defaults are the
 *     shipped configuration.  The library never reads the environment.
 */
#ifndef VIT_HIP_H
#define VIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIT_ABI_VERSION 18

typedef enum { VIT_OK = 0, VIT_ERR_INVALID = 1, VIT_ERR_LAUNCH = 2 } vit_status;
typedef enum { VIT_F32 = 0, VIT_BF16 = 1, VIT_MASK4 = 2 } vit_dtype;

/* VIT_MASK4: a bit mask of an [m][n] tensor (ReLU / dropout masks saved by the forward for the backward): byte
 * ((i/4)*ceil(n/4) + j/4)*4 + i%4, bit j%4; 4*ceil(m/4)*ceil(n/4) bytes.  One byte = 4 columns of a row; one dword =
 * a 4 x 4 block (byte = row).  8x smaller than the bf16 tensor it replaces as a mask source. */
typedef enum { VIT_ACT_NONE = 0, VIT_ACT_RELU = 1, VIT_ACT_GELU = 2 } vit_act;

/* Launch flags (vit_gemm_desc.flags, vit_attn_bwd `flags`).
 * VIT_FLAG_SHARED_CUS: other kernels may hold compute units while this launch runs — RCCL all-reduce kernels of the
 *   data-parallel backward overlap it.  Kernels that otherwise run a persistent one-workgroup-per-CU grid with a
 *   static item assignment (the bf16 GEMM's wide-epilogue kinds, the fused attention backward) then launch one
 *   workgroup per item, so the hardware places work on whichever CUs are free instead of a workgroup waiting for a
 *   CU a collective holds.  Same arithmetic, bitwise-identical results. */
#define VIT_FLAG_SHARED_CUS 1

int vit_abi_version(void);
const char* vit_last_error(void);

/* Launch options (process-wide; every name's default is the shipped configuration).  They choose between kernel
 * variants that compute the same function — A/B runs and the per-variant tests use them — and are the only switches
 * the library has: nothing is read from the environment, so a user's environment cannot change which kernels run.
 *   "gemm_impl"          0 automatic (default); 1 / 2 / 4 force the bf16 GEMM kernel generation (register-staged
 *                        128x128 / LDS-DMA 128x128 / LDS-DMA 256x256 ping-pong)
 *   "gemm_tail"          0 (default since round 5): 1 = split-K tail for a last round of 256x256 tiles that fills at
 *                        most half the CUs.  With the package's two-stream forward and backward the other stream
 *                        fills those CUs instead: the tails measured 0.18 ms/step slower at C2
 *   "gemm_tail_min_kt"   40: minimum k-tiles (K / 64) for that tail (with the tail on and the weight gradients on their
 *                        own stream, the QKV input gradient's tail at K = 2304 (36) measured 0.35 ms/step slower)
 *   "splitk_min_kt"      0 (automatic): minimum k-tiles per K-slice in vit_gemm_split_k_hint
 *   "gemm_group_m"       0 (automatic): tile-row group size of the 256x256 tile order
 *   "gemm_epi_general"   0: 1 forces the general (unspecialised) GEMM epilogue
 *   "gemm_persist"       1: persistent one-workgroup-per-CU grid for the wide-epilogue GEMM kinds (0: one per tile)
 *   "attn_fwd_split"     0: 1 forces the tiled attention forward for T <= 256 (default there: the persistent ring)
 *   "attn_bwd_split"     0: 1 forces the tiled attention backward for T <= 256
 *   "attn_bwd_grid"      0 (automatic): workgroups of the persistent attention backward
 *   "ln16"               1: the 16-B-per-lane LayerNorm forward where the layout allows it
 *   "ln_al"              1: LayerNorm backward accumulators in LDS (0: registers)
 *   "splitk_rounds"      1: rounds of 256 workgroups the weight-gradient K split aims at (vit_gemm_split_k_hint)
 *   "attn_fwd_grid"      0 (automatic: one workgroup per CU): workgroups of the persistent ring attention forward
 *                        when the call's own max_wgs is 0
 *   "augment_path"       0 (automatic): 1 forces the direct form of vit_augment_to_tensor, 2 its tiled two-pass form
 *                        wherever a tile's row span fits (see "Training augmentation" below)
 * ABI 15 removed the one-workgroup-per-head attention forward, which lost its A/B runs, together with the option name
 * that selected it: vit_set_option refuses that name.
 * ABI 16 removed the 128x128-tile second launch for a last partial round of 256x256 tiles, which measured slower (33.0
 * vs 31.6 ms/step), and its option name "gemm_tail_v2": refused likewise.
 * ABI 17 adds the gradient-clipping entry points (vit_grad_sumsq, vit_grad_clip_finish, vit_adamw_clipped) and no
 * option name: clipping is an argument of the optimizer, not a kernel variant.
 * ABI 18 adds the weight-EMA entry points (vit_adamw_ema, vit_ema_swap), likewise with no option name.
 * Since ABI 18, entry points that are purely added do not change the version: a host that needs one checks for the
 * symbol (dlsym, or a link error).  The version changes only when an existing signature or meaning does.  Added under
 * 18 this way: vit_softmax_xent_mixed and vit_mix_batch (label smoothing, mixup and CutMix), with no option name;
 * vit_augment_workspace_bytes and vit_augment_to_tensor (crop, flip, normalize, erase), with "augment_path";
 * vit_drop_path_rows, vit_gemm_rowscale and vit_gemm_kernel_choice (stochastic depth), with no option name;
 * vit_adamw_groups and vit_lamb_{moments,trust,update}_groups (every param group in one launch), with no option name;
 * vit_augment_to_u8, vit_randaug_workspace_bytes and vit_randaug_to_tensor (RandAugment), with no option name of their
 * own ("augment_path" chooses the form of vit_augment_to_u8 as it does for vit_augment_to_tensor);
 * vit_attn_rollout_workspace_bytes, vit_attn_rollout_step and vit_attn_rollout_step_form (attention rollout), with no
 * option name: the form is an argument of the third;
 * vit_patch_keep, vit_im2col_gather, vit_gather_pos, vit_pos_grad_gather and vit_col2im_scatter (patch dropout), with
 * no option name;
 * vit_softmax_xent_distill (knowledge distillation against a frozen teacher's logits), with no option name.
 * vit_set_option returns VIT_ERR_INVALID for an unknown name; vit_get_option returns INT64_MIN for one. */
int vit_set_option(const char* name, int64_t value);
int64_t vit_get_option(const char* name);

/* ------------------------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:  C[i][j] = epi( alpha * sum_r A(i,r) * B(j,r) )
 *   A(i,r) at a[i*lda + r] when a_kcontig, else a[r*lda + i]   (same for B with ldb / b_kcontig)
 *   epi(v): v += beta*C_old (f32 out only); v += bias[j]; act; v *= (aux(i,j) > 0) when aux (aux_dtype VIT_MASK4:
 *           v *= aux bit);
 *           dropout(p, seed, index i*n + j) with 1/(1-p) scale; v += res(row(i), j) where row(i) = i % res_rowmod
 *           (res_rowmod == 0: i); stored at C[orow(i)*ldc + j], orow(i) = (i/G)*Gs + i%G when out_group_rows = G > 0.
 * Replaces: nn.Linear (transformer.py:12-18,38,56,58; vit.py:70,73), the conv-as-GEMM (vit.py:21-28), and all their
 * autograd dgrad/wgrad GEMMs; dropout (transformer.py:47,59); residual adds (transformer.py:77-78); ReLU (:57).
 * bf16 inputs run on v_mfma_f32_16x16x32_bf16 (fp32 accumulate); f32 inputs on v_mfma_f32_32x32x2_f32 (exact fp32).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct vit_gemm_desc {
  const void* a;
  const void* b;
  void* c;
  int64_t lda, ldb, ldc;
  int64_t m, n, k;
  int32_t a_kcontig, b_kcontig;
  int32_t in_dtype;   /* vit_dtype of A and B */
  int32_t out_dtype;  /* vit_dtype of C */
  float alpha, beta;
  const float* bias;  /* [n] or NULL */
  int32_t act;        /* vit_act */
  int32_t aux_dtype;
  const void* aux;    /* relu-backward mask source (keep where aux > 0) or NULL */
  int64_t ldaux;
  const void* res;    /* residual added last, or NULL */
  int64_t ldres;
  int64_t res_rowmod;
  int32_t res_dtype;
  float dropout_p;    /* 0 disables */
  uint32_t dropout_seed;
  int32_t split_k;    /* >1: K split over workgroups, fp32 slabs in workspace, deterministic reduce */
  int64_t out_group_rows, out_group_stride;
  void* workspace;
  int64_t workspace_bytes;
  /* NULL, or [ceil(m/256)][n] f32: per-256-row-block column sums of C as stored (after the epilogue and the
   * out_dtype rounding) — the bias gradient of the layer whose input gradient C is (transformer.py Linear backward),
   * finished by vit_colsum_finish.  Requires out_group_rows == 0. */
  float* colsum_part;
  /* NULL, or a VIT_MASK4 buffer for C: the dropout keep bits when the epilogue applies dropout (transformer.py:47,59),
   * else (C as stored > 0) — the ReLU-backward mask (transformer.py:57).  Requires out_group_rows == 0. */
  void* mask_out;
  /* 0/1, or S: the dropout index of output row i is (i * S) * n + j — C computes rows i*S of a larger [m*S][n] tensor
   * (the last block's token-0 rows, ldA = S*K), and its dropout draws the same bits as the full tensor's rows. */
  int64_t dropout_row_stride;
  int32_t flags;      /* VIT_FLAG_* */
  /* 0, or R0: C's row i is row i + R0 of the tensor its dropout indices refer to ((i + R0) * S * n + j with S the
   * row stride above): a GEMM over a row range of a larger tensor (one half-batch chain of the forward) draws the
   * same bits as the whole tensor's rows (ABI 13). */
  int64_t dropout_row0;
} vit_gemm_desc;

/* Workspace vit_gemm can use: split_k > 1: the K-split fp32 slabs (required).  split_k <= 1: the slabs of the split-K
 * tail (when the 256x256 tiles leave the last round of the 256 CUs at most half full, those tile rows run split-K
 * over the idle CUs; option "gemm_tail" 0 disables it), or 0.  Without it (NULL / too small) the GEMM runs unsplit. */
int64_t vit_gemm_workspace_bytes(const vit_gemm_desc* d);
/* Recommended split_k for C[m][n] with reduction depth k and input dtype (VIT_BF16 / VIT_F32) on the kernel vit_gemm
 * will pick: fills one round of the 256 CUs with output tiles x K-slices, each slice >= 4 (bf16) / 8 (f32)
 * k-tiles deep.  Used for the weight-gradient GEMMs (reduction over B*T rows; transformer.py Linear backward). */
int vit_gemm_split_k_hint(int64_t m, int64_t n, int64_t k, int in_dtype);
int vit_gemm(const vit_gemm_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Stochastic depth (drop path; timm's drop_path with scale_by_keep=True — the reference has none): in training a
 * whole residual branch is dropped per image, x = x + keep[b] / (1 - p_l) * dropout(branch(x)), keep ~ Bernoulli(1 -
 * p_l) drawn per block l, site (0 = attention, 1 = FFN) and image b.  Two purely added entry points (ABI 18):
 *
 * vit_drop_path_rows: one launch fills the factor table of a whole forward, one float per token row,
 *     out[(l*2 + site) * B*T + b*T + t] = keep ? 1.0f / (1.0f - rates[l]) : 0.0f      (L * 2 * B * T floats)
 *     keep = vit_hash_u32(site_seed(seed, L + l, site), b) >= threshold(rates[l]),
 *   with the counter hash, per-site seed and threshold of the element dropout (site_seed: the host package's and the
 *   oracle's; layers L .. 2L-1 keep these streams apart from the element dropout's, which use 0 .. L-1).  `rates` is a
 *   HOST float[L], copied into the kernel arguments: no table upload, no host sync, no allocation.  A rate of 0 gives
 *   1.0f everywhere.  Refused: a NULL out / rates, L, B or T <= 0, L > VIT_DROP_PATH_MAX_LAYERS, B * T >= 2^31, a
 *   rate outside [0, 1) or NaN.
 *
 * vit_gemm_rowscale: vit_gemm with one more epilogue step, after the dropout and before the residual add:
 *     s = row_scale[(i + dropout_row0) * max(dropout_row_stride, 1)];   v = (s != 0) ? v * s : 0;
 *   The row index is the dropout index's row, so a GEMM over a row range (dropout_row0) or over the token-0 rows
 *   (dropout_row_stride = T) of a larger tensor addresses that tensor's table, which must reach that index for every
 *   i < m.  The zero is a select, not a product: a dropped row passes on no inf or NaN of its branch.  mask_out is
 *   vit_gemm's mask with the bits of every row whose s == 0 cleared, so the saved keep bits already combine both
 *   masks and the backward needs the mask and the scalar 1 / ((1 - dropout_p)(1 - p_l)) alone.  Every kernel and
 *   epilogue vit_gemm chooses between applies the factor (the 256x256 kernel through an epilogue kind of its own
 *   beside the dropout + residual one, which is left as it was).  row_scale == NULL is vit_gemm itself; a table of
 *   1.0f gives vit_gemm's bits.  row_scale is DEVICE memory, 4-B aligned.
 * ------------------------------------------------------------------------------------------------------------ */
#define VIT_DROP_PATH_MAX_LAYERS 64
int vit_drop_path_rows(float* out, uint32_t seed, int64_t L, int64_t B, int64_t T, const float* rates /* host, [L] */,
                       void* stream);
int vit_gemm_rowscale(const vit_gemm_desc* d, const float* row_scale /* device; NULL: vit_gemm */, void* stream);

/* Which kernel vit_gemm (row_scale == NULL) or vit_gemm_rowscale would launch for this descriptor under the current
 * options; nothing is launched and no pointer is read (added under ABI 18).  It is the launcher's own plan, so a test
 * can tell that a case reaches the kernel it means to test.
 *   *impl: 0 the fp32 kernel; 1 / 2 / 4 the bf16 kernel generation (option "gemm_impl")
 *   *kind: the 256x256 kernel's epilogue kind (impl 4; VIT_EPI_GENERAL otherwise: the other kernels have the general
 *          epilogue alone).  Named here: the kinds a dropout / residual epilogue can take.  Other values are further
 *          fast kinds (bias + activation, ReLU masks, the patch embedding).
 * Where a split-K tail follows the whole rounds of tiles, the whole-round launch is reported.  Refused: what vit_gemm
 * refuses, and a NULL impl / kind. */
#define VIT_EPI_BDR 3     /* dropout(alpha * acc [+ bias]) [+ residual], wide bf16 rows */
#define VIT_EPI_SLAB 4    /* split-K fp32 slabs; the reduce then runs the general epilogue */
#define VIT_EPI_GENERAL 5 /* the general epilogue */
#define VIT_EPI_BDRS 8    /* VIT_EPI_BDR with the row factor of vit_gemm_rowscale */
int vit_gemm_kernel_choice(const vit_gemm_desc* d, const float* row_scale, int32_t* impl, int32_t* kind);

/* ------------------------------------------------------------------------------------------------------------
 * Patch embedding (vit.py:21-29,39-42).
 *   vit_im2col: x[B][C][H][W] (x_dtype) -> cols[B*N][C*P*P] (dtype), column order (c, kh, kw) = conv weight order,
 *               patch order row-major over (H/P, W/P).  The GEMM epilogue then adds conv bias + pos (res_rowmod = N)
 *               and writes rows (b, n) to x0[b*T + n] (out_group_rows = N, out_group_stride = T).
 *   vit_embed_cls: x0[b*T + N][:] = cls[b][:] + pos[N][:]   (CLS appended LAST, vit.py:41)
 * ------------------------------------------------------------------------------------------------------------ */
int vit_im2col(const void* x, int32_t x_dtype, void* cols, int32_t dtype, int64_t B, int64_t C, int64_t H,
               int64_t W, int64_t P, void* stream);
/* vit_col2im: the inverse permutation of vit_im2col (k = s = P): x[B][C][H][W] (x_dtype) <- cols[B*N][C*P*P] (dtype).
 * Used for the input-image gradient (conv dgrad, vit.py:21-28 backward) when the caller's input requires grad. */
int vit_col2im(const void* cols, int32_t dtype, void* x, int32_t x_dtype, int64_t B, int64_t C, int64_t H, int64_t W,
               int64_t P, void* stream);
int vit_embed_cls(const float* cls, const float* pos, void* x0, int32_t dtype, int64_t B, int64_t T, int64_t D,
                  void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * LayerNorm (nn.LayerNorm, transformer.py:71-72,77-78; vit.py:72), fp32 statistics.
 *   fwd: y = (x - mean) * rstd * gamma + beta; saves mean/rstd [rows].
 *   bwd: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma;
 *        dx_out = dx (+ dres when dres != NULL)                    — fused residual-gradient add (transformer.py:77-78)
 *        drop_out = dx_out * keep(drop_seed, i*cols + j)            — fused dropout backward of the producer branch,
 *                   WITHOUT the 1/(1-p) scale (exact in bf16: the consumers apply it, e.g. as GEMM alpha); with
 *                   drop_mask (VIT_MASK4 [rows][cols], the producing GEMM's mask_out) the keep bits are read from it
 *                   instead of re-hashed
 *        dgamma/dbeta: per-workgroup partials in `partial` [2][nparts][cols], reduced by vit_colsum_finish
 *        (deterministic); with `osum` != 0 also partial [2] = column sums of the stored gradient output (drop_out
 *        / (1-p) when drop_out is given, else dx_out) — the bias gradient of the Linear that consumes it, so
 *        [3][nparts][cols].
 * ------------------------------------------------------------------------------------------------------------ */
int vit_layernorm_fwd(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy,
                      float* mean, float* rstd, int64_t rows, int64_t cols, float eps, int32_t dtype, void* stream);
int64_t vit_layernorm_bwd_parts(int64_t rows, int64_t cols);
int vit_layernorm_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* gamma,
                      const float* mean, const float* rstd, const void* dres, void* dx_out, void* drop_out,
                      float drop_p, uint32_t drop_seed, const void* drop_mask, float* partial, int32_t osum,
                      int64_t rows, int64_t cols, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Multi-head self-attention (transformer.py:9-31 per head, :44-45 concat): qkv[B*T][3*D] with Q at columns
 * h*hd, K at D + h*hd, V at 2D + h*hd; o[B*T][D] (heads concatenated, same column order as torch.cat).
 *   o = softmax(scale * Q K^T) V with scale = sqrt(hd) in the reference (multiplied, transformer.py:24);
 *   lse[B][H][T] (natural log of the row softmax denominator, scaled-logit domain) saved for backward;
 *   probs [B][H][T][T] f32 optional (the `.attention_probs` side attribute, transformer.py:48).
 * bf16 & hd == 64: flash-style MFMA kernels (K/V tiles in LDS, online softmax); otherwise a generic VALU kernel.
 * Under the reference's x sqrt(hd) logit scale most softmax rows saturate and dS = P (dP - delta) becomes a small
 *   difference, so delta = rowsum(dO * O) must be exact to fp32 rounding:
 *   - the fused backward (bf16, hd == 64, T <= 256: every ViT-B/L 224^2 config) forms delta = rowsum(P * dP) itself
 *     from the fp32 P and dP it computes anyway; it reads neither `o` nor `o32`;
 *   - the tiled backward (T > 256) takes delta from o32 when given: the forward then also stores O unrounded,
 *     [B*T][D] f32 (o32 == NULL: the bf16 O, standard flash-attention practice, cheaper but inexact).
 *   vit_attn_bwd_uses_o32() says which one a shape runs (1: pass o32 to the forward and the backward).
 * fwd max_wgs (ABI 14): 0 = automatic (one workgroup per CU, or option "attn_fwd_grid"); > 0 = the persistent ring
 *   forward (T <= 256) runs at most max_wgs workgroups — per call, so two callers on two threads or streams never
 *   share the choice (the package's two-stream forward gives one chain 3/4 of the CUs this way).  Other forms ignore it.
 * bwd: dqkv[B*T][3*D]; workspace = vit_attn_bwd_workspace_bytes.
 * ------------------------------------------------------------------------------------------------------------ */
int vit_attn_fwd(const void* qkv, void* o, float* o32, float* lse, float* probs, int64_t B, int64_t T, int64_t H,
                 int64_t hd, float scale, int32_t dtype, int64_t max_wgs, void* stream);
int vit_attn_bwd_uses_o32(int64_t B, int64_t T, int64_t H, int64_t hd, int32_t dtype);
int64_t vit_attn_bwd_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t hd, int32_t dtype);
int vit_attn_bwd(const void* qkv, const void* o, const float* o32, const void* d_o, const float* lse, void* dqkv,
                 int64_t B, int64_t T, int64_t H, int64_t hd, float scale, int32_t dtype, void* workspace,
                 int32_t flags, void* stream);

/* Query 0 only (round 5): the last encoder block, whose output the classifier reads at token 0 only (vit.py:80), needs
 * attention output row 0 of every image (queries 1..T-1 feed rows nothing reads) and, in the backward, has a nonzero
 * output gradient on row 0 only; every softmax row is independent, so row 0 alone is the same function, in O(T hd) per
 * (image, head) instead of O(T^2 hd).
 *   fwd: o[b*T][D] (row 0 of every image; other rows untouched), lse[b][h][0].
 *   bwd: from d_o0[b][D] (image b's row-0 output gradient, row stride ldo): dQ row 0, every row of dK and dV into
 *        dqkv[B*T][3*D] (dQ rows 1..T-1 untouched).  P is recomputed as the forward forms it (row max, exp2, 1/sum;
 *        no log-sum-exp round trip: a one-key row has P = 1, dS = 0 exactly); delta = sum_k P dP from fp32 P and dP.
 *   fp32 arithmetic, outputs rounded once; hd <= 128, hd % 4 == 0, T <= 4096. */
int vit_attn_fwd_row0(const void* qkv, void* o, float* lse, int64_t B, int64_t T, int64_t H, int64_t hd, float scale,
                      int32_t dtype, void* stream);
int vit_attn_bwd_row0(const void* qkv, const void* d_o0, int64_t ldo, void* dqkv, int64_t B, int64_t T, int64_t H,
                      int64_t hd, float scale, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Reductions / elementwise.
 *   vit_colsum: out[j] = beta*out[j] + alpha * sum_i x[i*ldx + j]  (bias / pos / LN-affine gradients); deterministic.
 *   vit_colsum_finish: outs[s][j] = beta*outs[s][j] + sum_p part[s][p][j] for s < nsets (<= 3), summed in a fixed
 *               order — second stage of the column sums fused into vit_gemm (colsum_part) / vit_layernorm_bwd.
 *   vit_copy2d: dst[orow(i)*ldd + j] = beta*dst + src[irow(i)*lds + j] with optional row grouping on the source
 *               (irow(i) = (i/G)*Gs + i%G) — token-0 gather (vit.py:80), CLS-gradient copy, dropout-free casts.
 *   vit_dropout_bwd: y = x * keep(seed, i) * scale  (transformer.py:47,59 backward: scale = 1/(1-p); the engine
 *                    passes 1 and folds 1/(1-p) into the consumers, so the stored masked gradient is exact).
 *   vit_gelu_fwd/bwd: exact-erf GELU (vit.py:71) on f32.
 *   vit_softmax_xent: per-row softmax cross entropy (train.py:81,93): loss = mean_i(-log p[i][y_i]) and
 *                     dlogits = (softmax - onehot) / rows, in one pass.
 * ------------------------------------------------------------------------------------------------------------ */
int64_t vit_colsum_workspace_bytes(int64_t rows, int64_t cols);
int vit_colsum(const void* x, int64_t ldx, int32_t dtype, int64_t rows, int64_t cols, float* out, float alpha,
               float beta, void* workspace, void* stream);
int vit_colsum_finish(const float* part, int64_t nparts, int64_t cols, int32_t nsets, float* out0, float* out1,
                      float* out2, float beta, void* stream);
/* vit_colsum_finish_batch: up to 8 vit_colsum_finish jobs in one launch (the bias / LN-affine gradients of one encoder
 * block), each job's result bitwise that of its own vit_colsum_finish. */
typedef struct {
  const float* part;  /* [nsets][nparts][cols] */
  int64_t nparts, cols;
  int32_t nsets;      /* 1..3 */
  float* out[3];
  float beta;
} vit_colsum_job;
int vit_colsum_finish_batch(const vit_colsum_job* jobs, int32_t njobs, void* stream);
int vit_copy2d(const void* src, int64_t lds, int32_t src_dtype, void* dst, int64_t ldd, int32_t dst_dtype,
               int64_t rows, int64_t cols, int64_t src_group_rows, int64_t src_group_stride, float beta,
               void* stream);
int vit_dropout_bwd(const void* x, void* y, int32_t dtype, int64_t n, float p, uint32_t seed, float scale,
                    void* stream);
/* dx = dy * (y > 0): ReLU backward for the module-level FeedForward path (transformer.py:57). */
int vit_relu_bwd(const void* dy, const void* y, void* dx, int32_t dtype, int64_t n, void* stream);
/* y[i][j] = x[i][j] * bit(mask, i, j) * scale — a dropout backward from the forward's saved VIT_MASK4 keep bits
 * (transformer.py:59 backward at the head, where the gradient covers the token-0 rows only). */
int vit_mask4_apply(const void* x, int64_t ldx, int32_t x_dtype, void* y, int64_t ldy, int32_t y_dtype,
                    const void* mask, int64_t rows, int64_t cols, float scale, void* stream);
int vit_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int vit_gelu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
int vit_softmax_xent(const float* logits, const int64_t* labels, int64_t rows, int64_t classes, float* loss,
                     float* dlogits, float* workspace, void* stream);
/* vit_softmax_xent against a smoothed two-label target (label smoothing, mixup / CutMix labels; the reference's loss,
 * train.py:81, has neither).  The target of row i is never materialised:
 *   t_i = (1 - eps) * (lam_i * onehot(a_i) + (1 - lam_i) * onehot(b_i)) + eps / C,   eps = smoothing, C = classes,
 *   lam_i = 1 (and b_i = a_i) when `lam` or `labels_b` is NULL;
 *   loss = mean_i( lse_i - (1 - eps) * (lam_i * x[a_i] + (1 - lam_i) * x[b_i]) - (eps / C) * sum_c x[i][c] ),
 *   dlogits = (softmax - t) / rows.
 * = F.cross_entropy(logits, labels, label_smoothing=eps) for hard labels, F.cross_entropy(logits, soft_target,
 * label_smoothing=eps) and timm's SoftTargetCrossEntropy on timm's mixup_target otherwise.  All terms are formed
 * relative to the row maximum; a_i == b_i and lam in {0, 1} need no special case.  One launch over the rows and the
 * fixed-order reduce of vit_softmax_xent: no atomics, bitwise repeatable.  workspace: rows floats.  `lam` is DEVICE
 * memory, [rows].  Refused: a NULL logits / labels_a / loss / dlogits / workspace, rows or classes <= 0, smoothing
 * outside [0, 1) or NaN, lam without labels_b. */
int vit_softmax_xent_mixed(const float* logits, const int64_t* labels_a, const int64_t* labels_b /* may be NULL */,
                           const float* lam /* device, [rows]; may be NULL */, float smoothing, int64_t rows,
                           int64_t classes, float* loss, float* dlogits, float* workspace, void* stream);
/* Knowledge distillation: vit_softmax_xent_mixed blended with a term against a frozen teacher's logits, in one launch
 * over the rows (vit_distill.hip).  For student row x, teacher row z, C = classes:
 *   t      the target of vit_softmax_xent_mixed (same labels_a / labels_b / lam / smoothing rules);
 *   p = softmax(x),  p_tau = softmax(x / tau),  q_tau = softmax(z / tau);
 *   base_r = lse(x) - sum_c t * x             exactly vit_softmax_xent_mixed's row term;
 *   VIT_DISTILL_SOFT:  d_r = tau^2 * KL(q_tau || p_tau),   g_r = tau * (p_tau - q_tau);
 *   VIT_DISTILL_HARD:  yhat = the LOWEST index at which z attains its maximum,
 *                      d_r = lse(x) - x[yhat],             g_r = p - onehot(yhat);   tau is ignored (but checked);
 *   loss    = mean_r((1 - alpha) * base_r + alpha * d_r),
 *   dlogits = ((1 - alpha) * (p - t) + alpha * g_r) / rows.
 * The soft form is Hinton's loss with "batchmean" reduction: F.kl_div(log_softmax(x / tau), log_softmax(z / tau),
 * reduction="batchmean", log_target=True) * tau^2.  DeiT's script divides the KL by rows * C instead; a caller who
 * wants that weighting scales alpha.  No gradient is formed for the teacher.
 * alpha = 0 with a finite teacher gives the loss and dlogits of vit_softmax_xent_mixed bit for bit.  A label outside
 * [0, classes) gives a NaN loss and no stray read.  A NaN in a row of either input makes that row's gradient and the
 * loss NaN and leaves every other row's gradient as it is; inputs are otherwise assumed finite.  No atomics: bitwise
 * repeatable.  workspace: rows floats.  `lam` is DEVICE memory, [rows].
 * Refused (VIT_ERR_INVALID) before any launch: a NULL logits / teacher_logits / labels_a / loss / dlogits /
 * workspace; rows or classes <= 0, rows > 2^31 - 1; smoothing outside [0, 1) or NaN; lam without labels_b; a kind
 * other than the two; alpha outside [0, 1] or NaN; tau not finite or <= 0. */
typedef enum { VIT_DISTILL_SOFT = 0, VIT_DISTILL_HARD = 1 } vit_distill_kind;
int vit_softmax_xent_distill(const float* logits, const float* teacher_logits, const int64_t* labels_a,
                             const int64_t* labels_b /* may be NULL */,
                             const float* lam /* device, [rows]; may be NULL */, float smoothing,
                             int32_t kind /* VIT_DISTILL_SOFT = 0, VIT_DISTILL_HARD = 1 */, float alpha, float tau,
                             int64_t rows, int64_t classes, float* loss, float* dlogits,
                             float* workspace /* rows floats */, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Image pipeline of the training loader (train.py:151-155: convert('RGB') -> transforms.Resize((S, S)) ->
 * ToTensor; BrainTumorDataset.py:35-39 / CIFAR10 :157-159 feed it PIL images).  A batch of raw uint8 HWC images of
 * any sizes (ragged allowed), packed into one byte buffer `src`, described by meta[B][4] = (byte offset, H, W, C)
 * (int64, DEVICE memory; C in {1: L, 2: LA, 3: RGB, 4: RGBA} -> RGB as PIL converts), becomes out[B][3][S_h][S_w]
 * (VIT_F32 or VIT_BF16) = PIL-bilinear-resized pixel / 255, bit-exact with Pillow's 8-bit two-pass resampler.
 *   vit_resize_ksize: taps per output sample for one axis (in_size -> out_size); pass the max over the batch and axes.
 *   workspace: vit_resize_workspace_bytes(B, S_h, S_w, ksize) bytes (per-image coefficient tables).
 * ------------------------------------------------------------------------------------------------------------ */
int vit_resize_ksize(int64_t in_size, int64_t out_size);
int64_t vit_resize_workspace_bytes(int64_t B, int64_t out_h, int64_t out_w, int64_t ksize);
int vit_resize_to_tensor(const void* src, const int64_t* meta, int64_t B, int64_t out_h, int64_t out_w, int64_t ksize,
                         void* out, int32_t out_dtype, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training augmentation inside the resize launch (not in the reference, whose only transform is the resize,
 * train.py:151-155): random resized crop, horizontal flip, normalize and a constant-fill erase of the same packed
 * batch, as torchvision's RandomResizedCrop + RandomHorizontalFlip on the PIL image, ToTensor, Normalize(mean, std)
 * and timm's RandomErasing(mode='const') give.  items_dev[i] (DEVICE memory) describes image i:
 *   crop   img.convert('RGB').crop((x0, y0, x0+cw, y0+ch)).resize((out_w, out_h), BILINEAR), bit-exact with Pillow:
 *          the coefficients are those of cw -> out_w and ch -> out_h and the taps are clamped to the crop, not to the
 *          image (Image.resize(box=) clamps to the image and is a different picture);
 *   flip   out[..., x] = resized[..., out_w-1-x];
 *   value  with mean3 / std3 (HOST float[3] each): ((float)v / 255.0f - mean[c]) / std[c], two IEEE fp32 operations
 *          after the division by 255, bitwise torch's (x - mean) / std on the ToTensor output; without: v / 255.0f;
 *   erase  inside rows [ey0, ey1) x columns [ex0, ex1) of the OUTPUT (after the flip) the value is erase_value and
 *          none of that pixel's source taps is read.
 * The bf16 output is the fp32 value rounded once (nearest even).  ksize is the max over the batch of
 * vit_resize_ksize(cw, out_w) and vit_resize_ksize(ch, out_h).  An identity table (full-image box, no flip, empty
 * erase box, no mean) gives vit_resize_to_tensor bit for bit.
 * The entry point cannot read the table, so the coefficient kernel clamps every box to its image (x0 into [0, w-1],
 * cw into [1, w-x0], rows likewise) and an erase box acts only where it meets the output: a bad table gives a wrong
 * picture, never a read outside the image's bytes [off, off + h*w*c).
 * Two forms compute the same bits.  The direct form is vit_resize_to_tensor's schedule (every output pixel runs the
 * horizontal pass once per vertical tap).  The tiled form gives one workgroup VIT_AUG_TILE_ROWS x VIT_AUG_TILE_COLS
 * output pixels: it runs the horizontal pass once per source row that the tile's vertical taps reach, into LDS, and
 * the vertical pass out of LDS (Pillow's own two-pass schedule); a tile whose taps reach more than
 * VIT_AUG_TILE_MAX_SPAN source rows takes the direct form, decided per workgroup.  Option "augment_path": 0 chooses
 * per launch (the tiled form up to ksize 9, the range where every tile fits and where it measured faster, DESIGN.md
 * §5; the direct form above), 1 the direct form everywhere, 2 the tiled form wherever the span fits.
 * Refused: NULL src / meta / items_dev / out / workspace, only one of mean3 / std3, a zero or non-finite std, a
 * non-finite mean or erase_value, a dtype other than VIT_F32 / VIT_BF16, the size limits of vit_resize_to_tensor, a
 * workspace smaller than vit_augment_workspace_bytes.
 * ------------------------------------------------------------------------------------------------------------ */
#define VIT_AUG_TILE_ROWS 16
#define VIT_AUG_TILE_COLS 64
#define VIT_AUG_TILE_MAX_SPAN 80
typedef struct vit_aug_item {
  int32_t x0, y0, cw, ch;     /* crop box in source pixels: columns [x0, x0+cw), rows [y0, y0+ch) */
  int32_t flip;               /* 1: mirror the output left-right */
  int32_t ey0, ey1, ex0, ex1; /* erase box in output pixels (after the flip); empty when ey1<=ey0 or ex1<=ex0 */
} vit_aug_item; /* 36 bytes */
int64_t vit_augment_workspace_bytes(int64_t B, int64_t out_h, int64_t out_w, int64_t ksize);
int vit_augment_to_tensor(const void* src, const int64_t* meta, const vit_aug_item* items_dev, int64_t B,
                          int64_t out_h, int64_t out_w, int64_t ksize, const float* mean3, const float* std3,
                          float erase_value, void* out, int32_t out_dtype, void* workspace, int64_t workspace_bytes,
                          void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * RandAugment between the flip and ToTensor (not in the reference; the policy is timm's `rand-m9-mstd0.5-inc1`): a
 * chain of up to VIT_RA_MAX_LAYERS image operations per image on the uint8 RGB picture of the output size, every one
 * bit-exact with the Pillow call it stands for.
 *
 * vit_augment_to_u8 is the crop, resize and flip of vit_augment_to_tensor with a uint8 store: out_u8 is
 * [B][out_h][out_w][3] (HWC, RGB), the bytes Pillow's crop().resize().transpose(FLIP_LEFT_RIGHT) gives.  It uses the
 * same tables, workspace, clamps, forms ("augment_path") and refusals; it neither normalizes nor erases (the erase
 * box of the items is ignored here and applied by vit_randaug_to_tensor).
 *
 * vit_randaug_to_tensor takes that picture through the chains and writes the tensor.  items_dev[i] (DEVICE memory)
 * holds image i's chain; layer l of every image runs in one launch, the kind chosen per image (uniform per
 * workgroup):
 *   VIT_RA_NONE          a copy
 *   VIT_RA_AUTOCONTRAST  ImageOps.autocontrast(img): per channel lo / hi = lowest / highest value present; identity if
 *                        hi <= lo, else table[i] = clip((int)(i * scale + offset)), scale = 255.0 / (hi - lo), offset =
 *                        -lo * scale, in fp64, every operation rounded on its own
 *   VIT_RA_EQUALIZE      ImageOps.equalize(img): per channel step = (pixels - count of the highest value present) /
 *                        255; identity if step == 0 or one value only, else table[i] = min(255, (step / 2 + pixels
 *                        below i) / step), in integers
 *   VIT_RA_INVERT        255 - i
 *   VIT_RA_POSTERIZE     ImageOps.posterize(img, iarg0): i & ~(2^(8 - bits) - 1), bits clamped into [0, 8]
 *   VIT_RA_SOLARIZE      ImageOps.solarize(img, iarg0): i < thresh ? i : 255 - i, thresh clamped into [0, 256]
 *   VIT_RA_SOLARIZE_ADD  timm's: i < iarg1 ? min(255, i + iarg0) : i, add clamped into [0, 255], thresh into [0, 256]
 *   VIT_RA_COLOR, VIT_RA_CONTRAST, VIT_RA_BRIGHTNESS, VIT_RA_SHARPNESS
 *                        ImageEnhance.X(img).enhance(farg) = Image.blend(degenerate, img, farg): t = d + f * (v - d) in
 *                        fp32, the product and the sum rounded separately; for 0 <= f <= 1 truncated to uint8, else
 *                        clipped to [0, 255] and truncated.  Degenerate d: Brightness 0; Color the gray L = (19595 R +
 *                        38470 G + 7471 B + 0x8000) >> 16 in all channels; Contrast the constant (int)(mean(L) + 0.5),
 *                        the mean an exact integer sum over the count in fp64; Sharpness ImageFilter.SMOOTH, the
 *                        3x3 kernel (1 1 1; 1 5 1; 1 1 1) with every weight the fp32 quotient by 13, accumulated in
 *                        fp32 from 0.5 row by row from the row below upward and truncated, the one-pixel border copied
 *   VIT_RA_AFFINE        img.transform(size, AFFINE, coef, BILINEAR, fillcolor=fill), which Image.rotate also ends in:
 *                        per output pixel, in fp64 with every operation rounded on its own, xin = a0 (x + 0.5) + a1 (y +
 *                        0.5) + a2, yin likewise with a3..a5; the fill colour if xin is outside [0, W) or yin outside
 *                        [0, H); else both less 0.5, x0 = floor, dx the fraction, the taps x0 and x0 + 1 clamped into
 *                        the row, v1 = p00 + (p01 - p00) dx on row clamp(y0), v2 the same on row y0 + 1 if it exists
 *                        (else v2 = v1), v = v1 + (v2 - v1) dy, truncated to uint8.
 *   Any other kind acts as VIT_RA_NONE.
 * A layer in which some image's kind needs the picture's histograms (AUTOCONTRAST, EQUALIZE, CONTRAST) is named by
 * its bit in stats_layers and gets one launch more, before its apply launch: per such image the three channel
 * histograms and the gray one in LDS, then that image's [3][256] uint8 table in the workspace; nothing is read on the
 * host.  A layer whose bit is missing skips that launch and those kinds then read a stale table: a wrong picture.
 * The last launch writes out [B][3][S_h][S_w] (fp32 / bf16) with vit_augment_to_tensor's value and erase: ((float)v /
 * 255.0f - mean[c]) / std[c], erase_value inside erase_items_dev[i]'s box; bf16 is that value rounded once.
 * Launches: 1 per layer + 1 per layer named in stats_layers + 1.  Nothing is allocated; layer l reads the picture
 * layer l - 1 wrote (two uint8 pictures in the workspace take turns) and u8_in is never written.
 * Safety: the entry point cannot read the tables.  Every tap of every kind is clamped into its image, integer
 * arguments are clamped as stated above, an unknown kind copies: a bad table gives a wrong picture, never an access
 * outside a buffer.  A non-finite coefficient is the caller's to refuse before the upload (it would only choose the
 * fill colour here: comparisons with NaN fail and the pixel counts as outside).
 * Refused: NULL u8_in / items_dev / erase_items_dev / out / workspace, B, S_h or S_w < 1, S_h or B > 65535, an image of
 * 2^31 bytes or more, nlayers outside [1, VIT_RA_MAX_LAYERS], a stats_layers bit at or above nlayers, mean3 / std3 /
 * erase_value / dtype as for vit_augment_to_tensor, a workspace smaller than vit_randaug_workspace_bytes, any
 * two of out, the workspace and u8_in overlapping.
 * ------------------------------------------------------------------------------------------------------------ */
#define VIT_RA_MAX_LAYERS 4
enum {
  VIT_RA_NONE = 0,
  VIT_RA_AUTOCONTRAST = 1,
  VIT_RA_EQUALIZE = 2,
  VIT_RA_INVERT = 3,
  VIT_RA_POSTERIZE = 4,
  VIT_RA_SOLARIZE = 5,
  VIT_RA_SOLARIZE_ADD = 6,
  VIT_RA_COLOR = 7,
  VIT_RA_CONTRAST = 8,
  VIT_RA_BRIGHTNESS = 9,
  VIT_RA_SHARPNESS = 10,
  VIT_RA_AFFINE = 11,
  VIT_RA_KINDS = 12
};
typedef struct vit_ra_layer {
  double coef[6];  /* AFFINE: a0..a5 as Pillow's transform receives them */
  int32_t kind;    /* VIT_RA_* */
  int32_t iarg0;   /* POSTERIZE bits; SOLARIZE threshold; SOLARIZE_ADD addend */
  int32_t iarg1;   /* SOLARIZE_ADD threshold */
  float farg;      /* COLOR / CONTRAST / BRIGHTNESS / SHARPNESS factor */
  uint8_t fill[4]; /* AFFINE: R, G, B of the fill colour; fill[3] unused */
  int32_t pad_;
} vit_ra_layer; /* 72 bytes */
typedef struct vit_ra_item {
  vit_ra_layer layer[VIT_RA_MAX_LAYERS];
} vit_ra_item; /* 288 bytes */
int vit_augment_to_u8(const void* src, const int64_t* meta, const vit_aug_item* items_dev, int64_t B, int64_t out_h,
                      int64_t out_w, int64_t ksize, void* out_u8, void* workspace, int64_t workspace_bytes,
                      void* stream);
int64_t vit_randaug_workspace_bytes(int64_t B, int64_t S_h, int64_t S_w);
int vit_randaug_to_tensor(const void* u8_in, const vit_ra_item* items_dev, int64_t B, int64_t S_h, int64_t S_w,
                          int32_t nlayers, int32_t stats_layers, const float* mean3, const float* std3,
                          const vit_aug_item* erase_items_dev, float erase_value, void* out, int32_t out_dtype,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Batch mix: mixup and CutMix of a contiguous [B][C][H][W] batch, out of place, in one streaming launch (the
 * reference has no augmentation beyond its resize, train.py:151-155).  items_dev[i] (DEVICE memory) describes image i:
 * its partner `src`, its own weight `w` outside the box and the box rows [y0, y1) x columns [x0, x1).  For element
 * (i, c, y, x):
 *   inside the box  (y0 <= y < y1 && x0 <= x < x1):  out = x[src_i]                         bitwise
 *   outside, w_i == 1:                               out = x[i]                             bitwise; x[src_i] is not
 *                                                    read there, so NaN / inf in it cannot leak
 *   outside otherwise:                               out = w_i * x[i] + (1 - w_i) * x[src_i]   in fp32, rounded once
 * mixup: empty box, w = lambda.  CutMix: w = 1, box.  An unmixed image: w = 1, empty box.
 * 16-byte accesses where x, out and the row length (W * element size) are multiples of 16 bytes, element accesses
 * otherwise and for a 16-byte unit that a box edge cuts; both forms give the same bits.  Indexing is 64-bit over the
 * batch (2 GiB and more is fine); one image must have fewer than 2^31 elements.
 * Refused: a NULL pointer, a non-positive dimension, a dtype other than VIT_F32 / VIT_BF16, `out` overlapping `x`
 * (image src is read after image i is written).  The table's contents are the caller's contract:
 * 0 <= src < B, 0 <= w <= 1, 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct vit_mix_item {
  int32_t src;
  float w;
  int32_t y0, y1, x0, x1;
} vit_mix_item; /* 24 bytes */
int vit_mix_batch(const void* x, void* out, int32_t dtype /* VIT_F32 | VIT_BF16 */, int64_t B, int64_t C, int64_t H,
                  int64_t W, const vit_mix_item* items_dev /* [B] */, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimizer (train.py:66,96: torch.optim.AdamW(lr, weight_decay=1e-4), betas (0.9, 0.999), eps 1e-8) as ONE
 * multi-tensor launch over a device-resident chunk table; also refreshes the compute-dtype shadow weights.
 *   p *= 1 - lr*wd;  m = b1*m + (1-b1)*g*gs;  v = b2*v + (1-b2)*(g*gs)^2;
 *   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps);  shadow = (dtype) p   (gs = grad_scale, e.g. 1/world_size)
 * vit_pack: shadow = (dtype) src over the same table layout (used after external writes to the fp32 params).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct vit_tensor_chunk {
  float* p;
  const float* g;
  float* m;
  float* v;
  void* shadow; /* NULL: no shadow for this chunk */
  int64_t n;
} vit_tensor_chunk;

int vit_adamw(const vit_tensor_chunk* table_dev, int64_t nchunks, float lr, float beta1, float beta2, float eps,
              float weight_decay, float bias_corr1, float bias_corr2, float grad_scale, int32_t shadow_dtype,
              void* stream);
int vit_pack(const vit_tensor_chunk* table_dev, int64_t nchunks, int32_t shadow_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Gradient clipping by global norm, fused into the AdamW step (ABI 17).  The reference has no counterpart: its loop
 * goes from loss.backward() straight to optimizer.step() (train.py:94-96); the formulas are those of
 * torch.nn.utils.clip_grad_norm_.  Three launches on one stream, no host sync, no atomics; all sums are fp64 in a
 * fixed order, so the results are bitwise reproducible.
 *   vit_grad_sumsq:       partial[i] = sum over chunk i of (gs * g[t])^2   (gs = grad_scale, the product in fp32 as the
 *                         update forms it, squared and summed in fp64); reads only the `g` and `n` fields of the table.
 *                         Several tables may fill consecutive slices of one `partial` buffer.
 *   vit_grad_clip_finish: one workgroup.  sum = partial[0] + ... + partial[nparts-1] in fp64, then clip[4] (fp32):
 *                           clip[0] = norm = (float)sqrt(sum)
 *                           clip[1] = coef = min(1, |max_norm| / (norm + 1e-6f))
 *                           clip[2] = skip = 1 when max_norm > 0 and norm is inf or NaN, else 0; skip sets coef = 0
 *                           clip[3] += skip   (running count of skipped steps; the caller zeroes it once)
 *                         max_norm < 0 bounds the norm by |max_norm| and never skips: a non-finite norm then gives
 *                         torch's coefficient (0 for inf, NaN for NaN), which reaches the update.  max_norm = 0 or NaN
 *                         is refused.
 *   vit_adamw_clipped:    vit_adamw with gs replaced by gs * clip[1]; when clip[2] != 0 it touches none of p, m, v or
 *                         the shadows.  vit_adamw itself is unchanged.
 * ------------------------------------------------------------------------------------------------------------ */
int vit_grad_sumsq(const vit_tensor_chunk* table_dev, int64_t nchunks, float grad_scale,
                   double* partial /* [nchunks] */, void* stream);
int vit_grad_clip_finish(const double* partial, int64_t nparts, float max_norm,
                         float* clip /* [4]: norm, coef, skip, skipped total */, void* stream);
int vit_adamw_clipped(const vit_tensor_chunk* table_dev, int64_t nchunks, float lr, float beta1, float beta2,
                      float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale,
                      int32_t shadow_dtype, const float* clip, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Weight EMA kept inside the AdamW step (ABI 18).  The reference has no counterpart (train.py:94-96 steps and
 * evaluates the raw weights); the recurrence is timm's ModelEmaV2: e_t = e_{t-1} + (1 - decay) * (p_t - e_{t-1}) with
 * p_t the weights AFTER step t.  The update kernel has p_t in a register when the EMA needs it, so the EMA costs one
 * more read-modify-write stream (38 B per element instead of 30) and no pass or launch of its own.
 * The chunk table keeps its layout; the EMA pointers travel in a parallel DEVICE array, one float* per chunk:
 * ema_dev[i] is the EMA slice of chunk i (n floats, 4-B alignment suffices: it may be a view of a larger buffer),
 * NULL for a chunk that keeps no EMA.
 * ------------------------------------------------------------------------------------------------------------ */
/* vit_adamw (clip == NULL) or vit_adamw_clipped (clip != NULL) followed, for every element of every chunk
 * whose ema[i] is not NULL, by   e += ema_weight * (p_new - e)   in fp32 (ema_weight = 1 - decay, formed in
 * double on the host and rounded once).  p, m, v and the shadows are bitwise those of the kernel it extends.
 * When clip != NULL and clip[2] != 0 (skipped step) nothing is touched, the EMA included. */
int vit_adamw_ema(const vit_tensor_chunk* table_dev, float* const* ema_dev, int64_t nchunks, float lr, float beta1,
                  float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale,
                  int32_t shadow_dtype, float ema_weight, const float* clip, void* stream);
/* For every chunk with ema[i] != NULL: exchange p and e element by element, then shadow = (dtype) p.
 * Other chunks are not touched.  Applying it twice restores every bit.  Reads the p, shadow and n fields only. */
int vit_ema_swap(const vit_tensor_chunk* table_dev, float* const* ema_dev, int64_t nchunks, int32_t shadow_dtype,
                 void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * LAMB: layer-wise trust ratios over the same chunk tables (purely added entry points, ABI 18).  The reference has no
 * counterpart (train.py:66 is AdamW); the formulas are those of timm's Lamb / NVIDIA's FusedLAMB with bias
 * correction, decoupled weight decay added into the update, for a tensor w at step t:
 *   g = grad * gs * coef                          (gs = grad_scale; coef = clip[1] with clip, else 1)
 *   m = b1*m + (1-b1)*g;   v = b2*v + (1-b2)*g^2
 *   u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd * w
 *   r = |w|_2 / |u|_2 over the whole tensor where `adapt` is set and both norms are > 0, else 1;  min(r, 1) with
 *       `trust_clip`
 *   w -= lr * r * u;   shadow = (dtype) w;   e += ema_weight * (w - e) where the chunk keeps an EMA
 * r needs the whole tensor before any element of it moves, so a step is three launches on one stream, no host sync,
 * no atomics, every sum fp64 in a fixed order (bitwise reproducible):
 *   vit_lamb_moments: one workgroup per chunk.  Writes m and v; forms u in fp32 and writes partial[2i] = sum w^2 and
 *                     partial[2i+1] = sum u^2 over chunk i (each fp32 value squared and summed in fp64).  w is read only.
 *   vit_lamb_trust:   one workgroup per tensor.  tensor_first[ntensors + 1] (device, int32) holds the index of each
 *                     tensor's first chunk and nchunks as its last entry: a tensor's chunks are consecutive in the
 *                     table.  Writes trust[tensor] (fp32) by the rule above from the fp64 sums of its chunks' partials;
 *                     any number of chunks per tensor.
 *   vit_lamb_update:  one workgroup per chunk.  Forms u again from the m and v the first pass wrote (u is never stored:
 *                     about 42 B per element over both passes against vit_adamw's 30) with the same arithmetic, so the
 *                     u that moves w is bit for bit the u whose norm was taken, and applies the last line with
 *                     r = trust[tensor_of_chunk[i]] (device, int32 [nchunks]).  ema_dev as in vit_adamw_ema; NULL
 *                     means no EMA at all, and then ema_weight is not read.
 * bias_corr1 = 1 - b1^t and bias_corr2 = 1 - b2^t must lie in (0, 1], eps must not be negative, and the second pass
 * takes the same eps, weight_decay and bias corrections as the first.  clip is NULL or vit_grad_clip_finish's block:
 * when clip[2] != 0 (skipped step) all three return at once, so neither w, m, v, the shadows, the EMA, the partials nor
 * trust[] change.  The AdamW entry points above are untouched.
 * ------------------------------------------------------------------------------------------------------------ */
int vit_lamb_moments(const vit_tensor_chunk* table_dev, int64_t nchunks, float beta1, float beta2, float eps,
                     float weight_decay, float bias_corr1, float bias_corr2, float grad_scale, const float* clip,
                     double* partial /* [2 * nchunks] */, void* stream);
int vit_lamb_trust(const double* partial /* [2 * nchunks] */, const int32_t* tensor_first /* [ntensors + 1] */,
                   int64_t ntensors, int32_t adapt, int32_t trust_clip, float* trust /* [ntensors] */,
                   const float* clip, void* stream);
int vit_lamb_update(const vit_tensor_chunk* table_dev, float* const* ema_dev, const int32_t* tensor_of_chunk,
                    const float* trust, int64_t nchunks, float lr, float eps, float weight_decay, float bias_corr1,
                    float bias_corr2, int32_t shadow_dtype, float ema_weight, const float* clip, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Grouped optimizer steps: the AdamW and LAMB updates above over the chunks of up to VIT_OPT_MAX_GROUPS param groups
 * in ONE launch each (purely added entry points, ABI 18).  With layer-wise learning-rate decay a ViT-B has 28 groups
 * (14 depth levels x {decay, no decay}); stepping them one launch per group gives 28 (AdamW) or 84 (LAMB) launches of
 * a handful of chunks each.  Here the table holds the chunks of every group and a device array names each chunk's
 * group; the groups' hyper-parameters are HOST memory, read during the call, turned into the factors the
 * single-group entry points form (the same floats) and passed to the kernel by value in its argument segment: a
 * learning rate that changes every step costs no copy and no staging buffer.
 *   group_of_chunk[i] (device, int32 [nchunks]) is the index into groups[] of chunk i; chunks of one group need not
 *   be consecutive.  A chunk whose index is not in 0..ngroups-1 is left untouched (so is a tensor of
 *   vit_lamb_trust_groups whose group_of_tensor entry is not).
 *   vit_adamw_groups: every chunk comes out bit for bit as from vit_adamw (clip == NULL, ema_dev == NULL),
 *     vit_adamw_clipped (clip) or vit_adamw_ema (ema_dev; a NULL ema_dev[i] keeps no EMA for chunk i) called with its
 *     group's scalars.  flags must be 0.
 *   vit_lamb_*_groups: the three LAMB passes; p, m, v, the shadows, the EMA, the partials and trust[] are bit for bit
 *     those of per-group calls.  group_of_tensor (device, int32 [ntensors]) gives the trust pass each tensor's group;
 *     VIT_OPT_ADAPT and VIT_OPT_TRUST_CLIP are vit_lamb_trust's `adapt` and `trust_clip`.  All three take the same
 *     groups[].
 * Refused (VIT_ERR_INVALID): NULL pointers (ema_dev and clip may be NULL), a count <= 0, ngroups outside
 * 1..VIT_OPT_MAX_GROUPS, a bias correction outside (0, 1], a negative eps, an lr that is not finite, flags other than
 * the two above (any flag for vit_adamw_groups), and with ema_dev an ema_weight outside (0, 1).
 * ------------------------------------------------------------------------------------------------------------ */
#define VIT_OPT_MAX_GROUPS 64
#define VIT_OPT_ADAPT 1      /* LAMB: trust ratio applies (wd != 0 or always_adapt) */
#define VIT_OPT_TRUST_CLIP 2 /* LAMB: min(r, 1) */
typedef struct vit_opt_group { /* 32 bytes, host memory */
  float lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2;
  int32_t flags; /* AdamW entry point: must be 0 */
} vit_opt_group;

int vit_adamw_groups(const vit_tensor_chunk* table_dev, float* const* ema_dev /* or NULL */,
                     const int32_t* group_of_chunk /* device [nchunks] */, int64_t nchunks,
                     const vit_opt_group* groups /* host [ngroups] */, int32_t ngroups, float grad_scale,
                     int32_t shadow_dtype, float ema_weight, const float* clip /* or NULL */, void* stream);
int vit_lamb_moments_groups(const vit_tensor_chunk* table_dev, const int32_t* group_of_chunk, int64_t nchunks,
                            const vit_opt_group* groups, int32_t ngroups, float grad_scale, const float* clip,
                            double* partial /* [2 * nchunks] */, void* stream);
int vit_lamb_trust_groups(const double* partial, const int32_t* tensor_first /* [ntensors + 1] */,
                          const int32_t* group_of_tensor /* device [ntensors] */, int64_t ntensors,
                          const vit_opt_group* groups, int32_t ngroups, float* trust /* [ntensors] */,
                          const float* clip, void* stream);
int vit_lamb_update_groups(const vit_tensor_chunk* table_dev, float* const* ema_dev, const int32_t* tensor_of_chunk,
                           const float* trust, const int32_t* group_of_chunk, int64_t nchunks,
                           const vit_opt_group* groups, int32_t ngroups, int32_t shadow_dtype, float ema_weight,
                           const float* clip, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Validation metrics on the device (a purely added entry point, ABI 18): top-k counts, the summed loss and the
 * confusion matrix of a batch of logits, accumulated into device state that the host reads once, when the epoch ends
 * (the reference's evaluate, train.py:29-44, moves an argmax to the host per batch and yields one accuracy).
 * Per row i, with x = logits + i * ld (fp32; columns [classes, ld) are never read) and y = labels[i]:
 *   order:     entry c precedes entry d when x[c] > x[d], or when they compare equal and c < d.  A NaN counts as
 *              greater than every number and equal to another NaN; -0.0 equals +0.0.
 *   pred[i]    the first entry of that order — torch.argmax on the CPU: the lowest index among the maxima, the first
 *              NaN when there is one.  Always written.
 *   ignored:   y outside [0, classes): rank[i] = -1, row_loss[i] = 0, counts[1] += 1, and nothing is indexed by y.
 *   scored:    rank[i] = the number of entries that precede y (top-1 is rank == 0, that is pred == y; top-k is
 *              rank < k, with one tie rule for both); row_loss[i] = lse(x) - x[y], formed relative to the row maximum
 *              as vit_softmax_xent forms it; counts[0] += 1; counts[2 + rank] += 1 when rank < maxk;
 *              confusion[y * classes + pred] += 1 when confusion is not NULL; loss_sum += row_loss[i].
 * counts [2 + maxk] int64, loss_sum [1] fp64 and confusion [classes * classes] int64 (row = label, column =
 * prediction) are ACCUMULATED: the caller zeroes them, and launches on one stream add to them with no host
 * involvement.  The integers are exact; loss_sum grows by the fp64 sum of the call's fp32 row terms taken in a fixed
 * order (no floating-point atomics), so the same calls on the same inputs give the same bits.  pred, rank and
 * row_loss ([rows] each) are per-call outputs and the second kernel's input.  Two launches: one wave per row, then one
 * workgroup.
 * Refused (VIT_ERR_INVALID) before any launch: a NULL among logits, labels, pred, rank, row_loss, counts, loss_sum;
 * rows <= 0, classes <= 0, ld < classes; maxk outside [1, min(classes, VIT_EVAL_MAXK)]; rows or classes above INT32_MAX.
 * ------------------------------------------------------------------------------------------------------------ */
#define VIT_EVAL_MAXK 16
int vit_eval_update(const float* logits, int64_t ld, const int64_t* labels, int64_t rows, int64_t classes,
                    int32_t maxk, int64_t* pred /* [rows] */, int32_t* rank /* [rows] */, float* row_loss /* [rows] */,
                    int64_t* counts /* [2 + maxk] */, double* loss_sum /* [1] */,
                    int64_t* confusion /* [classes * classes] or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Attention rollout (purely added entry points, ABI 18): the attention map of one token (Abnar & Zuidema 2020)
 * without the [B][H][T][T] probabilities of vit_attn_fwd's `probs` in memory.  The reference keeps those tensors as
 * `.attention_probs` (transformer.py:26) and its README names "analyzing model attention maps" as a use of them; the
 * rollout of a token is a [T] vector per image, formed as a vector-matrix chain from the last block to the first.
 * One call is one step of that chain for one block.  With P[h][i][j] = softmax_j(scale * q_i(h) . k_j(h)) formed from
 * qkv[B*T][3*D] (the layout and `scale` of vit_attn_fwd):
 *   F[i][j]  = mean, max or min over h of P[h][i][j]                     (fuse)
 *   w[i]     = r_in[i] / (1 + sum_j F[i][j])
 *   r_out[j] = sum_i w[i] * F[i][j] + w[j]
 * which is r_out = r_in A for A = (F + I) with its rows re-normalised.  Starting from a one-hot r at `token` and
 * stepping through the blocks from the last to the first leaves row `token` of A_L ... A_1.
 * The step forms its own softmax (it takes no lse), so the map is a function of qkv alone.  bf16 products are exact;
 * logits, exp, fusing, row and column sums are fp32; r_in and r_out are fp32 [B][T].  Two launches (a workgroup per
 * image and 32 query rows, with its rows of F in LDS; then the sum of the row blocks' partial column sums in a fixed
 * order): no atomics, the same bits on every run.  Nothing outside qkv, r_in, r_out and the workspace's
 * vit_attn_rollout_workspace_bytes bytes is touched, and one image's values never reach another image's output.
 * Forms: bf16 with hd == 64 computes S on v_mfma_f32_32x32x16_bf16 (K tiles through LDS); every other case runs VALU
 * dot products.  vit_attn_rollout_step_form takes the choice as `form`: 0 automatic (what vit_attn_rollout_step
 * runs), 1 the VALU form, 2 the MFMA form — for A/B runs and the per-form tests.
 * Refused (VIT_ERR_INVALID) before any launch: a NULL among qkv, r_in, r_out, workspace; a size <= 0; T > 1024;
 * hd > 128 or hd % 4 != 0; a dtype other than VIT_F32 / VIT_BF16; fuse outside 0..2; form outside 0..2, or 2 where the
 * MFMA form does not apply; r_in and r_out overlapping (the caller alternates two buffers); qkv not 16-B aligned.
 * vit_attn_rollout_workspace_bytes returns 0 for a shape that the step refuses.
 * ------------------------------------------------------------------------------------------------------------ */
#define VIT_ROLLOUT_MEAN 0
#define VIT_ROLLOUT_MAX 1
#define VIT_ROLLOUT_MIN 2
int64_t vit_attn_rollout_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t hd, int32_t dtype, int32_t fuse);
int vit_attn_rollout_step(const void* qkv, const float* r_in, float* r_out, int64_t B, int64_t T, int64_t H,
                          int64_t hd, float scale, int32_t dtype /* VIT_F32 | VIT_BF16 */, int32_t fuse,
                          void* workspace, void* stream);
int vit_attn_rollout_step_form(const void* qkv, const float* r_in, float* r_out, int64_t B, int64_t T, int64_t H,
                               int64_t hd, float scale, int32_t dtype, int32_t fuse, int32_t form, void* workspace,
                               void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Patch dropout (timm's patch_drop_rate; purely added entry points, ABI 18): a training forward keeps K of the N patch
 * tokens of every image, so every block runs on T' = K + 1 rows per image.  Tokens 0 .. N-1 are the patches and token
 * N is CLS (appended last, vit.py:41); the classifier reads token 0.  Patch 0 and CLS are always kept; the kept
 * patches stay in ascending order with CLS last, so token 0 stays token 0.
 *
 * vit_patch_keep draws the table of one forward: idx[b][j] = the patch in row j of image b (ascending, idx[b][0] = 0),
 *   inv[b][n] = the row of patch n, or -1 where it is dropped.  The key of patch n of image b is
 *   vit_hash_u32(site_seed(seed, 2L, 0), b * N + n) (layers 0 .. L-1 of site_seed are the element dropout's streams,
 *   L .. 2L-1 the drop path's); patch n >= 1 is kept iff fewer than K - 1 patches m in 1 .. N-1 have a smaller
 *   (key, m) pair, compared lexicographically: a uniform random (K-1)-subset per image.  One workgroup per image, keys
 *   in LDS, ranks by counting, rows by a prefix sum: no atomics, no host sync, the same bytes for the same seed.
 * vit_im2col_gather is vit_im2col where row b * K + j of cols is patch idx[b][j]; dropped patches are never read.
 * vit_gather_pos fills posg[b * K + j][:] = pos[idx[b][j]][:] (fp32, D % 4 == 0): the residual rows with which the
 *   embedding GEMM keeps its single rounding of acc + bias + pos (res = posg, res_rowmod = B * K, out_group = (K, K+1)).
 * vit_pos_grad_gather: gpos[n] = beta * gpos[n] + sum over b with inv[b][n] >= 0 of dx[b * (K+1) + inv[b][n]] for n < N
 *   and gpos[N] = beta * gpos[N] + sum over b of the CLS rows dx[b * (K+1) + K]; dx is [B * (K+1)][D] in `dtype`, gpos
 *   fp32 [N + 1][D].  The sum runs over b ascending in one thread: bitwise repeatable.  beta == 0 never reads gpos.
 * vit_col2im_scatter is vit_col2im reading row b * K + inv[b][n] of cols [B * K][C*P*P]; dropped patches get zeros.
 * A table entry outside its range (a caller's own table) is clamped (idx) or read as dropped (inv), never addressed.
 * Refused (VIT_ERR_INVALID) before any launch: a NULL pointer; B <= 0; N, K outside 1 <= K <= N <=
 * VIT_PATCH_KEEP_MAX_N; L < 0; B * N >= 2^31; the image / patch / dtype conditions of vit_im2col and vit_col2im.
 * ------------------------------------------------------------------------------------------------------------ */
#define VIT_PATCH_KEEP_MAX_N 4096
int vit_patch_keep(uint32_t seed, int64_t L, int64_t B, int64_t N, int64_t K, int32_t* idx /* [B][K] */,
                   int32_t* inv /* [B][N] */, void* stream);
int vit_im2col_gather(const void* x, int32_t x_dtype, void* cols, int32_t dtype, const int32_t* idx, int64_t B,
                      int64_t C, int64_t H, int64_t W, int64_t P, int64_t K, void* stream);
int vit_gather_pos(const float* pos, const int32_t* idx, float* posg, int64_t B, int64_t N, int64_t K, int64_t D,
                   void* stream);
int vit_pos_grad_gather(const void* dx, int32_t dtype, const int32_t* inv, float* gpos, int64_t B, int64_t N, int64_t K,
                        int64_t D, float beta, void* stream);
int vit_col2im_scatter(const void* cols, int32_t dtype, const int32_t* inv, void* x, int32_t x_dtype, int64_t B,
                       int64_t C, int64_t H, int64_t W, int64_t P, int64_t K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_HIP_H */
