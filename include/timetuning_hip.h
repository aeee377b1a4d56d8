/*
 * timetuning_hip.h - C ABI of libtimetuning_hip.so (gfx950 / MI355X).
 *
 * The reference (SMSD75/Timetuning) is pure Python on top of ATen; it has no FFI of its own.
 * The entry points below are the op sites of its training hot path (SURVEY.md section 2.4,
 * k1-k19) restated as a C ABI: what a maintainer would bind with ctypes in place of the
 * ATen calls.  Each declaration cites the reference lines it replaces (paths relative to the
 * reference checkout).  INTEGRATION.md shows the reference-side ctypes stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (row-major, contiguous unless a leading
 *     dimension is passed) unless the parameter says otherwise;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls enqueue work
 *     and return, they never synchronise, allocate or free (ABI 7: also true of the K-split
 *     workspace of the persistent GEMMs, which is the caller's - tt_linear_ksplit_workspace_*);
 *     every call can be captured into a hipGraph;
 *   - return value: 0 on success, a negative TT_E* code otherwise; tt_last_error() returns a
 *     thread-local message for the last failing call;
 *   - workspaces are caller-owned; the matching *_workspace_bytes() gives the size.
 */
#ifndef TIMETUNING_HIP_H
#define TIMETUNING_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TT_OK 0
#define TT_EINVAL (-1)   /* bad shape / alignment / null pointer */
#define TT_ELAUNCH (-2)  /* HIP launch error */
#define TT_EUNSUPPORTED (-3)

typedef void* tt_stream_t;

const char* tt_last_error(void);
int tt_abi_version(void);   /* 8 = this header (7: before `precision` became an argument - tt_set_gemm_precision, a process-wide switch, is gone; 6: before the caller-owned K-split workspace and the range flag; 5: before the transpose-free weight gradient, the batched operand refresh and the distributed Sinkhorn steps; 4: before the fp16-pair entry points; 3: before tt_vit_params.patch_wp; 2: before the coarse entry points) */
/* Still 8 without the two host queries of the one-launch Sinkhorn solve (a default-off experiment, retired): only this
 * repository's own front end and tests called them, no signature a caller relies on changed, and a binding that still asks for them
 * fails loudly at symbol lookup, not silently. */
/* Tuning knobs of the dispatchers (names and defaults: the one list TT_KNOB_LIST in csrc/common.hpp) are read ONCE from the
 * environment; this setter changes one afterwards - for the A/B tools and tests only.  An unknown name is TT_EINVAL. */
int tt_set_tuning_knob(const char* name, int value);
/* Row `index` of that list: fills the non-null outputs with the knob's environment name (a static string), its default and its current
 * value.  TT_EINVAL for an index outside the list - so a caller enumerates from 0 until it is refused; that refusal is no failure and
 * leaves tt_last_error as it was. */
int tt_tuning_knob_info(int index, const char** name, int* default_value, int* value);
/* Fills name (<= cap bytes) with the gcnArchName of the current device; returns CU count or <0. */
int tt_device_info(char* name, int cap);

/* ---- ABI 7: the K-split workspace of the persistent GEMM kernels (gemm_pairs8.hip / gemm_planes8.hip behind tt_linear_fwd_pairs,
 * tt_linear_fwd_planes, tt_linear_bwd_data_pairs, tt_linear_bwd_data_planes).  The output tiles beyond the last whole round over the CUs
 * are split along K over several workgroups, which exchange fp32 partials and (tile, wave) arrival counters through this buffer.
 *   tt_linear_ksplit_workspace_bytes   its size for the current device (counters + partials; 64 MB + 8 KB on MI355X);
 *   tt_linear_ksplit_workspace_init    zeroes the counter block (a hipMemsetAsync on `stream`): ONCE after allocation - every launch
 *                                      leaves the counters zero again - and again after a launch that was aborted.
 * One buffer serves any sequence of launches on ONE stream (launches on different streams may overlap: give each stream its own).
 * workspace == NULL (or too small): such a call never splits K - the left-over tiles are cut into half tiles or dealt round-robin;
 * same arithmetic per output element, a different summation order across the K-tiles of those tiles (results may differ in the last bit
 * from a call with a workspace). */
size_t tt_linear_ksplit_workspace_bytes(void);
int tt_linear_ksplit_workspace_init(void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* ---- k4,k6,k7,k8,k9: nn.Linear forward  (dino_vision_transformer.py:94-103,115-117,122,130;
 *      models.py:915-926,1075-1077)
 *   y[M,N] = act(x[M,K] @ w[N,K]^T + bias) (+ residual)
 *   act: 0 none, 1 exact-erf GELU.  pre_act (optional, [M,N]) receives x@w^T+bias before the
 *   activation (saved for backward).  residual (optional, [M,N]) is added after the activation;
 *   it may alias y. */
int tt_linear_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y,
                  float* pre_act, int M, int N, int K, int act, int precision, tt_stream_t stream);

/* ---- k16: nn.Linear backward (autograd of the sites above)
 *   dx[M,K] = dy[M,N] @ w[N,K]            (* gelu'(gelu_pre[M,K]) if gelu_pre != NULL)
 *   dw[N,K] = dy[M,N]^T @ x[M,K],  db[N] = column sums of dy (db may be NULL)
 *   workspace for tt_linear_bwd_weight: tt_colsum_workspace_bytes(M, N) when db != NULL. */
int tt_linear_bwd_data(const float* dy, const float* w, const float* gelu_pre, float* dx, int M, int N, int K,
                       tt_stream_t stream);
int tt_linear_bwd_weight(const float* dy, const float* x, float* dw, float* db, int M, int N, int K,
                         void* workspace, size_t workspace_bytes, tt_stream_t stream);
size_t tt_linear_bwd_weight_workspace_bytes(int M, int N, int K); /* split-K partials and/or the column-sum scratch */
/* Both products of one nn.Linear in one call (they share dy and do not depend on each other): dx as tt_linear_bwd_data, dw / db as
 * tt_linear_bwd_weight, bit for bit.  Where both lean kernels apply and the weight gradient is split along its reduction, ONE launch carries
 * the dgrad tiles and the weight-gradient slices (neither fills the chip on the target frames alone), else the two are launched one after
 * the other.  x is the layer's input [M, Kx] with Kx = K; workspace: tt_linear_bwd_weight_workspace_bytes(M, N, K). */
int tt_linear_bwd(const float* dy, const float* w, const float* x, const float* gelu_pre, float* dx, float* dw, float* db, int M, int N, int K,
                  void* workspace, size_t workspace_bytes, tt_stream_t stream);
size_t tt_colsum_workspace_bytes(int M, int N);
/* out[N] = sum over rows of a[M,N] (deterministic two-stage reduction). */
int tt_colsum(const float* a, float* out, int M, int N, void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* ---- generic fp32 MFMA GEMM used by the sites above and by k11/k14:
 *   C[M,N] = alpha * op(A)[M,K] @ op(B)[K,N]
 *   a_mmajor = 0: A stored [M][lda] (k contiguous); 1: stored [K][lda] (m contiguous)
 *   b_nmajor = 0: B stored [N][ldb] (k contiguous, the nn.Linear weight layout); 1: stored [K][ldb]
 *   batch > 1 runs `batch` independent problems at the given element strides. */
int tt_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                int a_mmajor, int b_nmajor, float alpha, int batch, long long strideA, long long strideB,
                long long strideC, tt_stream_t stream);

/* Which tile shape the launcher picks for an M x N (x batch) product: 0 = 128x128, 1 = 64x128, 2 = 128x64,
 * 3 = 64x64 (block tile; 4 waves each).  Exposed so that profilers can attribute launches to instantiations. */
int tt_gemm_tile_choice(int M, int N, int batch);
/* Which kernel an fp32 tt_linear_fwd of this shape runs: bits 0-1 tile (0 128x128, 1 64x128, 2 128x64, 3 64x64), bit 8 set = the
 * lean whole-tile instance (gemm_nt_fast_kernel), clear = the general kernel.  For profilers' labels only. */
int tt_linear_fwd_route(int M, int N, int K);
/* Which kernel a tt_linear_fwd_planes call with these arguments runs: 8 = the persistent 8-phase kernel (gemm_planes8_kernel: whole
 * 256-wide column tiles, a grid that fills the chip, one of its compiled epilogues), 0 = gemm_planes_kernel.  For profilers' labels only. */
int tt_linear_fwd_planes_route(int planes, int M, int N, int K, int act, int has_bias, int has_residual, int has_y, int y_nplanes,
                               int has_pre_out);

/* ---- k1b: interpolate_pos_encoding for inputs whose token grid differs from the stored one
 *      (dino_vision_transformer.py:214-234): bicubic resampling of the patch position table, as
 *      nn.functional.interpolate(..., scale_factor=(scale_h, scale_w), mode="bicubic") computes it (align_corners False,
 *      coordinate scale 1/scale_factor, A = -0.75, border-clamped taps); the class row is copied.
 *   pos [1 + g*g, D] -> out [1 + gh*gw, D].  The reference passes scale = (rows + 0.1) / g, (cols + 0.1) / g.
 *   Accepted domain: D a multiple of 4, pos and out 16-byte aligned, positive scales; any g, gh, gw > 0 (gh != gw, 1 included). */
int tt_pos_embed_interpolate(const float* pos, float* out, int g, int gh, int gw, int D, float scale_h, float scale_w,
                             tt_stream_t stream);
/* Its adjoint (autograd of the nn.functional.interpolate call at dino_vision_transformer.py:226-230, and of the torch.cat at :233):
 * the gradient of the stored position table from the gradient of the resampled one, dtable [1 + gh*gw, D] -> dpos [1 + g*g, D].
 * Gather form - every source cell sums, output rows then columns ascending, the outputs that tap it, with the forward's own weights
 * (same scales, A = -0.75, border-clamped taps adding up on the border cells); the class row is copied.  No atomics: the same bits on
 * every call.  Accepted domain: as tt_pos_embed_interpolate. */
int tt_pos_embed_interpolate_bwd(const float* dtable, float* dpos, int g, int gh, int gw, int D, float scale_h, float scale_w,
                                 tt_stream_t stream);

/* `precision`: the arithmetic of the fp32-OPERAND forward products - an ARGUMENT of every entry point that has one (ABI 8; until ABI 7 a
 * process-wide switch, tt_set_gemm_precision: hidden state this interface promises not to have).  Taken by tt_linear_fwd,
 * tt_label_propagate[_maps], tt_mlp_head_forward, tt_scores_sinkhorn and, as tt_vit_params.precision, tt_vit_forward (planes == 0):
 *   TT_PRECISION_F32    0  f32 MFMA (exact fmaf chain)
 *   TT_PRECISION_BF16X3 1  operands split into bf16 hi + lo while staged, three bf16 MFMAs per product term (~2^-16 relative per product)
 *   TT_PRECISION_BF16   2  operands rounded to bf16 (BASELINE config C4's "MFMA bf16 path"; does not meet the 1e-3 fp32 contract);
 *                          tt_label_propagate[_maps] then computes its cosine similarities on bf16 MFMA too (what torch.autocast makes of
 *                          them); 0 and 1 leave them exact
 * Inputs / outputs stay fp32 in memory in every case.  The fp32-accurate split modes are not a `precision` but an operand FORMAT with
 * entry points of its own (fp16 pairs: tt_*_pairs*; three bf16 planes: tt_*_planes*).  tt_linear_bwd* always run in f32 (the bf16 path's
 * backward products have their own entry points: tt_linear_bwd_data_planes, tt_linear_bwd_weight_planes, tt_attention_bwd_bf16). */
#define TT_PRECISION_F32 0
#define TT_PRECISION_BF16X3 1
#define TT_PRECISION_BF16 2

/* ---- k1,k2: PatchEmbed conv (kernel = stride = P) + cls token + pos-embed
 *      (dino_vision_transformer.py:166-171, 236-247)
 *   img [F_src,C,H,W]; frame_map (optional int32[F]): output frame f reads img[frame_map[f]];
 *   w [D, C*P*P]; bias [D]; cls [D]; pos [(n+1), D]; tokens [F, n+1, D], n = (H/P)*(W/P). */
int tt_patch_embed_fwd(const float* img, const int32_t* frame_map, const float* w, const float* bias,
                       const float* cls, const float* pos, float* tokens, int F, int C, int H, int W, int P, int D,
                       tt_stream_t stream);
/* ---- k1,k2 backward: the adjoint of prepare_tokens (autograd of dino_vision_transformer.py:166-171, 236-247) for everything below
 *      block 0.  dtok [F, n+1, D] = the gradient of the tokens; img, frame_map as in the forward.  Any of the four outputs may be NULL:
 *   dw     [D, C*P*P] = sum over (f, p) of dtok[f, 1+p, :] (x) patch(img[frame_map[f]], p)   (PatchEmbed.proj.weight, :166-171)
 *   dbias  [D]        = sum over (f, p) of dtok[f, 1+p, :]                                   (PatchEmbed.proj.bias)
 *   dcls   [D]        = sum over f of dtok[f, 0, :]                                          (cls_token, :239-240)
 *   dtable [n+1, D]   = sum over f of dtok[f]                                                (the position table added at :243; on
 *                       the stored square grid this IS the gradient of pos_embed, otherwise tt_pos_embed_interpolate_bwd takes it there)
 *   dw is an exact-f32 MFMA product (v_mfma_f32_32x32x2_f32) whose patch operand is gathered from img inside the kernel (no im2col
 *   buffer); its F*n rows are split across workgroups, partial tiles go to `workspace` and are folded in slice order.  Every sum has a
 *   fixed order and there are no float atomics: two calls give the same bits.  Nothing allocates or synchronises (legal under stream
 *   capture); img may be NULL when dw is.
 *   Accepted domain (tt_patch_embed_bwd_shape_ok; a refusal names the rule in tt_last_error and launches nothing): P % 4 == 0,
 *   W % 4 == 0, D % 4 == 0, H and W multiples of P, every pointer 16-byte aligned, n < 2^20, F (n+1) D < 2^31 - any F, C, D / 64 and
 *   C*P*P / 64 remainders included.  workspace: tt_patch_embed_bwd_workspace_bytes(...) bytes, 16-byte aligned (needed when dw's rows are split
 *   or dbias is asked for without dtable; contents on entry are irrelevant). */
int tt_patch_embed_bwd(const float* dtok, const float* img, const int32_t* frame_map, float* dw, float* dbias, float* dcls,
                       float* dtable, int F, int C, int H, int W, int P, int D, void* workspace, size_t workspace_bytes,
                       tt_stream_t stream);
size_t tt_patch_embed_bwd_workspace_bytes(int F, int C, int H, int W, int P, int D);
int tt_patch_embed_bwd_shape_ok(int F, int C, int H, int W, int P, int D);   /* 1 = taken, 0 = refused */
/* The same on bf16 operands - BASELINE C4's bf16 path, what torch.autocast makes of the conv (dino_vision_transformer.py:166-171):
 * w_planes = tt_split_planes(w, 1 plane) [D, C*P*P] bf16, the patches rounded to bf16 on the way into an im2col buffer, fp32
 * accumulation, fp32 tokens.  One row pass + ONE tt_linear_fwd_planes over all F (n + 1) token rows (the class-token rows are zero
 * rows that meet cls + pos[0] in the residual).  Needs P % 4 == 0, W % 4 == 0, C P P % 64 == 0, D % 64 == 0; workspace of
 * tt_patch_embed_planes_workspace_bytes = F (n + 1) C P P bf16. */
size_t tt_patch_embed_planes_workspace_bytes(int F, int C, int H, int W, int P);
int tt_patch_embed_fwd_planes(const float* img, const int32_t* frame_map, const void* w_planes, const float* bias, const float* cls,
                              const float* pos, float* tokens, int F, int C, int H, int W, int P, int D, void* workspace,
                              size_t workspace_bytes, tt_stream_t stream);

/* ---- k3: LayerNorm over the last dim (dino_vision_transformer.py:139,143,196; eps = 1e-6)
 *   mean/rstd (optional, [rows]) are saved for backward.  `rows` counts OUTPUT rows.
 *   skip_group = 0: x is [rows, D].  skip_group = N (tokens per frame): x is [F, N, D] and the output
 *   [F*(N-1), D] drops token 0 of every frame - the final norm followed by `[:, 1:]` (models.py:966-967). */
int tt_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                     int rows, int D, float eps, int skip_group, tt_stream_t stream);
/*   dx has x's layout; dgamma/dbeta [D] optional (NULL for frozen norms).  add_to_dx != 0 accumulates
 *   into dx (residual branch).  With skip_group the rows of dx that belong to token 0 are not touched.
 *   workspace: tt_layernorm_bwd_workspace_bytes(rows, D). */
/* amax_out (ABI 7, here and on tt_attention_bwd / tt_l2norm_bwd / tt_linear_bwd_data_pairs): an "amax slot" - tt_amax_slot_bytes()
 * bytes of device memory (16 floats 256 bytes apart: the waves of a kernel spread their atomics over them, thousands on one address
 * serialise) that the caller ZEROED - or NULL.  The kernel raises the slot to max |.| of the gradient it writes (relaxed atomic max on
 * the non-negative floats' bits: deterministic).  That gradient is the dy of the next Linear's backward: tt_split_pairs_dual_parts takes
 * the slot as amax_in and needs no max pass of its own for the power-of-two scale of the split (measured: C2 -0.8 %, C1 -1 %).
 * The published value is max |dx| over the rows the call WROTE.  tt_layernorm_bwd with skip_group never visits token 0's rows of dx:
 * without add_to_dx the caller zeroed them and the value is max |dx| of the whole tensor; with add_to_dx they keep what was accumulated
 * before, which the maximum would miss - amax_out together with add_to_dx and skip_group is therefore REFUSED (no call site needs it:
 * the residual-branch norms accumulate without skip_group, the final norm drops token 0 into a zeroed dx). */
size_t tt_amax_slot_bytes(void);
int tt_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                     float* dx, float* dgamma, float* dbeta, int rows, int D, int add_to_dx, int skip_group,
                     void* workspace, size_t workspace_bytes, float* amax_out, tt_stream_t stream);
size_t tt_layernorm_bwd_workspace_bytes(int rows, int D);

/* ---- k5 (+k10): multi-head self-attention core (dino_vision_transformer.py:122-129)
 *   qkv [F, N, 3*H*hd] as written by the qkv Linear (q | k | v, each head-major);
 *   out [F, N, H*hd] = softmax(q k^T * scale) v ; lse [F,H,N] optional (saved for backward);
 *   probs [F,H,N,N] optional (get_last_selfattention, :256-263).  hd must be 64, N <= 256. */
int tt_attention_fwd(const float* qkv, float* out, float* lse, float* probs, int F, int N, int H, int hd,
                     float scale, tt_stream_t stream);
/*   dqkv [F,N,3*H*hd] from dout [F,N,H*hd]; workspace: tt_attention_bwd_workspace_bytes. */
int tt_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int F,
                     int N, int H, int hd, float scale, void* workspace, size_t workspace_bytes, float* amax_out, tt_stream_t stream);
size_t tt_attention_bwd_workspace_bytes(int F, int N, int H, int hd);
/* The same backward on bf16 MATRIX operands (BASELINE C4's bf16 path; what torch.autocast makes of the backward of q k^T and attn v,
 * dino_vision_transformer.py:125-129): q, k, v, dout, P and dS are rounded to bf16 where they enter a product, products on
 * v_mfma_f32_16x16x16_bf16 with fp32 accumulation; the softmax statistics (lse), delta = <dout, out>, P and dS themselves are fp32.
 * Inputs and outputs stay fp32 in memory; same arguments and workspace as tt_attention_bwd. */
int tt_attention_bwd_bf16(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int F, int N, int H, int hd,
                          float scale, void* workspace, size_t workspace_bytes, tt_stream_t stream);
/* The same backward with its matrix products on fp16-PAIR operands (round 6: the "f16x3" mode's attention backward; fp32-class like
 * tt_attention_bwd: q (scaled), k, v, dout, P and dS are split into (hi, lo) where they enter a product, three fp16 MFMAs per product term,
 * two fp32 accumulators; lse, delta, P and dS themselves are fp32).  dout is a gradient: it is split as dout times the power of two S that
 * brings max |dout| into [2^13, 2^14), dS = P (dP - delta) as dS S 2^-12 (exact; the outputs are divided by the scales again).  dout_amax:
 * the amax slot the kernel that wrote dout raised (amax_out of tt_linear_bwd_data_pairs ...), or NULL - the call then measures the maximum
 * itself (one small launch).  range_flag: the pair entry points' range flag (below) - raised when a hi half of q, k, v, the scaled dout
 * or the scaled dS is not finite (dS: |v| beyond ~128).
 * Inputs and outputs fp32 in memory; workspace: tt_attention_bwd_pairs_workspace_bytes; amax_out as tt_attention_bwd. */
int tt_attention_bwd_pairs(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int F, int N, int H, int hd,
                           float scale, const float* dout_amax, void* workspace, size_t workspace_bytes, int* range_flag, float* amax_out,
                           tt_stream_t stream);
size_t tt_attention_bwd_pairs_workspace_bytes(int F, int N, int H, int hd);

/* ---- k11: F.normalize(x, dim=-1) (time_tuning.py:136; mask_propagation.py:418-419)
 *   xn[rows,D] = x / max(||x||, 1e-12); inv_norm[rows] optional.  x rows may be strided (ldx). */
int tt_l2norm_fwd(const float* x, int ldx, float* xn, float* inv_norm, int rows, int D, tt_stream_t stream);
/*   dx = (dxn - xn * <xn, dxn>) * inv_norm */
int tt_l2norm_bwd(const float* dxn, const float* xn, const float* inv_norm, float* dx, int rows, int D, float* amax_out,
                  tt_stream_t stream);
/* ---- k18: in-place row L2 normalisation of the prototypes (time_tuning.py:124-128).  D <= 1024 (as tt_l2norm_fwd). */
int tt_normalize_rows_inplace(float* w, int rows, int D, tt_stream_t stream);

/* ---- k12: Sinkhorn-Knopp (time_tuning.py:157-168 + my_utils.py:246-274)
 *   scores [B_total, K] (all columns of the global problem: local batch, queue rows, and for
 *   world_size > 1 every rank's rows after an all-gather); q_out [rows_out, K] receives the
 *   assignment of rows [row0, row0+rows_out).  Implements Q=exp(scores/eps)^T, Q/=sum,
 *   `iters` x (row-normalise to 1/K, column-normalise to 1/B_total), final column normalise,
 *   in scaling-vector form.  workspace: tt_sinkhorn_workspace_bytes(B_total, K). */
int tt_sinkhorn(const float* scores, float* q_out, int B_total, int K, int row0, int rows_out, float eps,
                int iters, void* workspace, size_t workspace_bytes, tt_stream_t stream);
size_t tt_sinkhorn_workspace_bytes(int B_total, int K);
/*   The reference's own DISTRIBUTED form (my_utils.py:250-272: the columns stay on their rank, the K row sums are all-reduced once per
 *   iteration), one rank's share in steps - the caller all-reduces u[K] (sum) between them and passes the SAME workspace to all three:
 *     tt_sinkhorn_local_begin   scores [B_loc, K] -> E = exp(scores / eps) in the workspace, u_out[k] = the local row sums
 *     tt_sinkhorn_local_step    u_in = the all-reduced row sums: row step, column step with c = 1 / B_total, u_out = the next local row sums
 *     tt_sinkhorn_local_end     the last row step (u_in NULL: none - zero iterations) + final column normalisation -> q_out [rows_out, K]
 *   iters iterations = begin, (all-reduce, step) x (iters - 1), all-reduce, end.  Equal to tt_sinkhorn on the gathered rows up to fp32
 *   rounding (the sums fold in a different order). */
size_t tt_sinkhorn_local_workspace_bytes(int B_loc, int K);
int tt_sinkhorn_local_begin(const float* scores, float* u_out, int B_loc, int K, float eps, void* workspace, size_t workspace_bytes,
                            tt_stream_t stream);
int tt_sinkhorn_local_step(const float* u_in, float* u_out, int B_loc, int B_total, int K, void* workspace, size_t workspace_bytes,
                           tt_stream_t stream);
int tt_sinkhorn_local_end(const float* u_in, float* q_out, int B_loc, int rows_out, int K, void* workspace, size_t workspace_bytes,
                          tt_stream_t stream);
/*   The reference-signature entry, my_utils.sinkhorn(Q, nmb_iters, world_size) (my_utils.py:246): takes the POSITIVE matrix
 *   exp(scores / eps) itself (no log / exp round trip) - as Q [K, B_total] (transposed = 0: the reference's layout) or as
 *   Q^T [B_total, K] (transposed = 1: what an all-gather of the ranks' columns yields; read in place).  Same iterations,
 *   same workspace. */
int tt_sinkhorn_from_q(const float* Q, int transposed, float* q_out, int B_total, int K, int row0, int rows_out, int iters,
                       void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* ---- bf16-plane operands: BASELINE config C4's "MFMA bf16 path" (planes = 1) and the fp32-accurate split mode (planes = 3)
 *   of the forward nn.Linear sites (dino_vision_transformer.py:94-103,115-130).  A tensor "in P planes" is P bf16 arrays of
 *   the tensor's shape, `plane_stride` ELEMENTS apart, with value = plane0 + plane1 + plane2 (plane0 = bf16(x), plane1 =
 *   bf16(x - plane0), plane2 = bf16(x - plane0 - plane1): 8 / 16 / 24 significant bits).  Producers write planes, consumers
 *   read planes: nothing is converted on the GEMM's own path.
 *   tt_split_planes          fp32 [n] -> planes (weights; activations produced by fp32 kernels).  n % 8 == 0.
 *   tt_layernorm_fwd_planes  tt_layernorm_fwd with the result in planes (optional mean / rstd as there).
 *   tt_linear_fwd_planes     y = act(x @ w^T + bias) (+ residual): x [M,K] and w [N,K] in `planes` planes each; products
 *                            x_i w_j with i + j <= planes + 1 (1 / 3 / 6 bf16 MFMAs per term), fp32 accumulate.  Outputs, any of:
 *                            y fp32 [M,N], pre_out fp32 (pre-activation), y_planes (y_nplanes planes of y).  residual fp32 may
 *                            alias y.  N % 64 == 0, K % 64 == 0; any M.
 *   tt_attention_fwd_bf16    softmax(q k^T * scale) v on bf16 qkv [F,N,3*H*64] -> bf16 out [F,N,H*64]; fp32 scores and
 *                            accumulation, N <= 256 (dino_vision_transformer.py:122-129). */
int tt_split_planes(const float* src, void* dst_planes, long long plane_stride, int planes, long long n, tt_stream_t stream);
int tt_layernorm_fwd_planes(const float* x, const float* gamma, const float* beta, void* y_planes, long long plane_stride,
                            int planes, float* mean, float* rstd, int rows, int D, float eps, int skip_group,
                            tt_stream_t stream);
int tt_linear_fwd_planes(const void* x_planes, long long x_plane_stride, const void* w_planes, long long w_plane_stride, int planes,
                         const float* bias, const float* residual, float* y, float* pre_out, void* y_planes,
                         long long y_plane_stride, int y_nplanes, int M, int N, int K, int act, void* workspace, size_t workspace_bytes,
                         tt_stream_t stream);   /* workspace: tt_linear_ksplit_workspace_bytes() or NULL (ABI 7) */
int tt_attention_fwd_bf16(const void* qkv, void* out, int F, int N, int H, int head_dim, float scale, tt_stream_t stream);

/* ---- fp16-PAIR operands: the fp32-accurate split mode "f16x3" (round 4) of the forward nn.Linear sites
 *   (dino_vision_transformer.py:94-103,115-130; models.py:915-926).  An fp32 value x is held as hi = fp16(x) and lo = fp16((x - hi) * 2^11):
 *   x = hi + lo * 2^-11 to <= 2^-23 relative.  A tensor "in pairs" has its elements in groups of 32 consecutive ones, each group stored
 *   as [hi x 32][lo x 32] fp16 - 4 bytes per element, rows as long as in fp32.  A product term costs three fp16 MFMAs (hi hi into one
 *   fp32 accumulator, hi lo + lo hi into a second one folded in with the exact 2^-11); the dropped lo lo term is <= 2^-22 relative.
 *   Operands must lie in fp16's range (|x| <= 65504: beyond it the result is inf / NaN, as an fp16 autocast's would be).
 *   The RANGE FLAG (ABI 7): every entry point that PRODUCES pairs from fp32 values - tt_split_pairs, tt_layernorm_fwd_pairs,
 *   tt_linear_fwd_pairs (y_pairs), tt_split_pairs_dual(_multi), tt_patch_embed_fwd_pairs, tt_vit_params.range_flag - takes `range_flag`, a
 *   DEVICE int (or NULL): the kernel stores 1 to it when a value it splits is beyond fp16's range or not finite (hi = inf / NaN) and never
 *   clears it.  The caller zeroes it, reads it at its own synchronisation points and decides (the Python host raises PairRangeError and names
 *   --precision f32; tests/test_hip_pairs.py).  tt_attention_fwd_pairs needs none: its outputs are convex combinations of v.
 *   tt_split_pairs          fp32 [n] -> pairs, n % 32 == 0 (weights; activations produced by fp32 kernels).  tt_join_pairs: back.
 *   tt_layernorm_fwd_pairs  tt_layernorm_fwd with the result in pairs [rows][2 D] (D % 32 == 0; optional mean / rstd as there).
 *   tt_linear_fwd_pairs     y = act(x @ w^T + bias) (+ residual): x [M,K], w [N,K] in pairs.  Outputs, any of: y fp32 [M,N], pre_out
 *                           fp32 (pre-activation), y_pairs [M][2 N].  residual fp32 may alias y.  N % 64 == 0, K % 32 == 0; any M.
 *   tt_linear_fwd_pairs_route  which kernel such a call runs: 8 = the persistent gemm_pairs8s_kernel (N % 128 == 0, K % 32 == 0,
 *                           M >= 256, at least 96 tiles of 256 x 128; every epilogue incl. pre_out + GELU pairs), 0 = the general
 *                           kernel.  Profilers' labels only. */
int tt_split_pairs(const float* src, void* dst_pairs, long long n, int* range_flag, tt_stream_t stream);
int tt_join_pairs(const void* src_pairs, float* dst, long long n, tt_stream_t stream);
int tt_layernorm_fwd_pairs(const float* x, const float* gamma, const float* beta, void* y_pairs, float* mean, float* rstd, int rows, int D,
                           float eps, int skip_group, int* range_flag, tt_stream_t stream);
int tt_linear_fwd_pairs(const void* x_pairs, const void* w_pairs, const float* bias, const float* residual, float* y, float* pre_out,
                        void* y_pairs, int M, int N, int K, int act, void* workspace, size_t workspace_bytes, int* range_flag,
                        tt_stream_t stream);   /* workspace: tt_linear_ksplit_workspace_bytes() or NULL (ABI 7) */
int tt_linear_fwd_pairs_route(int M, int N, int K, int act, int has_bias, int has_residual, int has_y, int has_y_pairs, int has_pre_out);

/* The fused attention core on pair operands (dino_vision_transformer.py:120-132): qkv [F N][2 x 3 H 64] in pairs (the qkv Linear's y_pairs) ->
 * any of out_pairs [F N][2 H 64] (the proj Linear's operand), out_f32 [F, N, H 64] and lse [F, H, N] (what tt_attention_bwd recomputes from).
 * Both products take three fp16 MFMAs per term, as the pair GEMMs do; fp32 scores, softmax and accumulation.  head_dim 64; any N (K / V of a
 * head resident in LDS up to 256 tokens, KV-tiled with an online softmax beyond). */
int tt_attention_fwd_pairs(const void* qkv_pairs, void* out_pairs, float* out_f32, float* lse, int F, int N, int H, int head_dim, float scale,
                           tt_stream_t stream);

/* The backward products of an nn.Linear on pair operands (the "f16x3" mode's backward; autograd of dino_vision_transformer.py:94-103,
 * 115-130 and of the projection head, models.py:915-926):
 *   tt_split_pairs_dual           fp32 [R][C] -> transposed pairs [C][2 Rpad] (rows R..Rpad-1 zero, Rpad % 32 == 0) and, optionally in the
 *                                 same pass, row-major pairs [R][2 C] (C % 32 == 0) and the fp32 column sums [C]: a dy is read ONCE for
 *                                 the operand of its weight-gradient product, the operand of its data-gradient product and its bias
 *                                 gradient.  workspace (tt_split_pairs_dual_workspace_bytes; needed for column sums / a scale).
 *                                 dst_t_pairs may be null (row pairs + column sums only: all the transpose-free weight gradient
 *                                 below needs).  scale_out (device float, or null): a gradient's whole magnitude may sit below fp16's
 *                                 normal range (2^-14: a C2 step's dy tensors peak at 1e-3 .. 1e-6) - the source is then multiplied
 *                                 by the power of two S that brings max |src| into [2^13, 2^14) before the split (exact), S is
 *                                 written to *scale_out, and the products below divide by it (their dy_scale argument, a DEVICE
 *                                 pointer: no host round trip).  The column sums are those of the unscaled source.
 *   tt_transpose_pairs            pairs [R][2 C] -> transposed pairs [C][2 Rpad]: a saved forward operand for the weight gradient.
 *   tt_linear_bwd_data_pairs      dx[M,K] = dy[M,N] @ w[N,K] (* gelu'(gelu_pre[M,K])): dy in pairs [M][2 N], the weight transposed in pairs
 *                                 wT [K][2 N]; N % 32 == 0, K % 64 == 0.
 *   tt_linear_bwd_weight_pairs    dw[N,K] = dy^T @ x: dyT [N][2 Mpad], xT [K][2 Mpad] (K % 64 == 0); split-K partials in the workspace,
 *                                 folded in a fixed order.
 *   tt_linear_bwd_weight_pairs_tn the same product from ROW pairs - dy [M][2 N] (the data-gradient product's operand) and the layer's
 *                                 input x [M][2 K] as the forward kept it: no transposed copies (gemm_pairs_tn.hip: the fragments are
 *                                 gathered by transposing LDS reads).  N % 128 == 0, K % 128 == 0, any M (_ok says whether a shape is
 *                                 taken); partials of the split m range in the workspace, folded in a fixed order.
 *   dy_scale (all three products)  device scalar S or NULL: the dy pairs hold dy * S (tt_split_pairs_dual's scale_out) - the result is
 *                                 divided by S in the epilogue (exact: S is a power of two). */
size_t tt_split_pairs_dual_workspace_bytes(int R, int C, int Rpad);
int tt_split_pairs_dual(const float* src, void* dst_t_pairs, void* dst_row_pairs, float* colsum, float* scale_out, int R, int C, int Rpad,
                        void* workspace, size_t workspace_bytes, int* range_flag, tt_stream_t stream);
/* tt_split_pairs_dual that LEAVES the column partial sums - colsum_parts [ceil(Rpad / 64)][C] fp32, caller-owned - unfolded, for
 * tt_linear_bwd_weight_pairs_tn_bias to fold in the launch that folds the weight gradient's split partials (one launch less per dy;
 * the bias gradient has the same bits either way).  workspace: as tt_split_pairs_dual (needed for a scale only). */
int tt_split_pairs_dual_parts(const float* src, void* dst_t_pairs, void* dst_row_pairs, float* colsum_parts, float* scale_out, const float* amax_in,
                              int R, int C, int Rpad, void* workspace, size_t workspace_bytes, int* range_flag, tt_stream_t stream);
/* amax_in (with scale_out): the amax slot the kernel that wrote src raised (amax_out above) - the split then needs no max pass and no
 * workspace; NULL: it makes its own. */
int tt_transpose_pairs(const void* src_pairs, void* dst_t_pairs, int R, int C, int Rpad, tt_stream_t stream);
/* tt_split_pairs_dual (without column sums) for n matrices in ONE launch per 32 of them: host arrays of n pointers / sizes; dst_t_pairs[i] or
 * dst_row_pairs[i] may be null.  What a training step needs of every weight the optimizer rewrote (row pairs: forward and weight-gradient
 * operand; transposed pairs: the data-gradient operand). */
int tt_split_pairs_dual_multi(const float* const* src, void* const* dst_t_pairs, void* const* dst_row_pairs, const int* R, const int* C,
                              const int* Rpad, int n, int* range_flag, tt_stream_t stream);
int tt_linear_bwd_data_pairs(const void* dy_pairs, const void* wT_pairs, const float* gelu_pre, float* dx, const float* dy_scale, int M, int N, int K,
                             void* workspace, size_t workspace_bytes, float* amax_out, tt_stream_t stream);   /* workspace: the K-split block or NULL (ABI 7) */
size_t tt_linear_bwd_weight_pairs_workspace_bytes(int N, int K, int Mpad);
int tt_linear_bwd_weight_pairs(const void* dyT_pairs, const void* xT_pairs, float* dw, const float* dy_scale, int N, int K, int Mpad, void* workspace,
                               size_t workspace_bytes, tt_stream_t stream);
int tt_linear_bwd_weight_pairs_tn_ok(int N, int K, int M);
size_t tt_linear_bwd_weight_pairs_tn_workspace_bytes(int N, int K, int M);
int tt_linear_bwd_weight_pairs_tn(const void* dy_pairs, const void* x_pairs, float* dw, const float* dy_scale, int N, int K, int M, void* workspace,
                                  size_t workspace_bytes, tt_stream_t stream);
/* ... and the bias gradient db [N] = the column sums of dy from their partials (colsum_parts [colsum_count][N] of
 * tt_split_pairs_dual_parts) in the same fold launch. */
int tt_linear_bwd_weight_pairs_tn_bias(const void* dy_pairs, const void* x_pairs, float* dw, const float* dy_scale, int N, int K, int M, void* workspace,
                                       size_t workspace_bytes, const float* colsum_parts, int colsum_count, float* db, tt_stream_t stream);
/*   prepare_tokens (dino_vision_transformer.py:166-171,236-247) on pair operands: tt_patch_embed_fwd with the conv weight in pairs
 *   [D][2 C P P] (tt_split_pairs of patch_w viewed [D, C P P]); the patches are split into pairs on their way into an im2col buffer
 *   (workspace: the rows, then the GEMM's K-split block, whose counters the call zeroes itself), ONE pair GEMM over all F (n + 1) rows
 *   leaves the tokens.  P % 4 == 0, W % 4 == 0, C P P % 32 == 0, D % 64 == 0. */
size_t tt_patch_embed_pairs_workspace_bytes(int F, int C, int H, int W, int P);
int tt_patch_embed_fwd_pairs(const float* img, const int32_t* frame_map, const void* w_pairs, const float* bias, const float* cls, const float* pos,
                             float* tokens, int F, int C, int H, int W, int P, int D, void* workspace, size_t workspace_bytes, int* range_flag,
                             tt_stream_t stream);
/*   The backward products of the same nn.Linear sites on bf16-plane operands (autograd of dino_vision_transformer.py:94-103,
 *   115-130; the bf16 path only - the fp32 modes keep the f32-MFMA backward kernels):
 *   tt_transpose_planes               fp32 [R][C] -> bf16 [C][Rpad], transposed, columns R..Rpad-1 zero (reduction index contiguous)
 *   tt_linear_bwd_data_planes         dx[M,K] = dy[M,N] @ w[N,K] (* gelu'(gelu_pre[M,K]) when given): dy in planes [M][N], the weight
 *                                     transposed in planes wT [K][N]; N % 64 == 0, K % 64 == 0
 *   tt_linear_bwd_weight_planes       dw[N,K] = dy[M,N]^T @ x[M,K]: dyT [N][Mpad] and xT [K][Mpad] from tt_transpose_planes with the
 *                                     same Mpad (a multiple of 64); split-K over Mpad with a fixed-order fold; N, K % 64 == 0 */
int tt_transpose_planes(const float* src, void* dst, int R, int C, int Rpad, tt_stream_t stream);
/* The same pass that ALSO leaves the fp32 column sums of src in colsum [C] (the bias gradient dy.sum(0) of an nn.Linear whose dy is
 * being transposed for tt_linear_bwd_weight_planes: one read of dy instead of two); workspace: ceil(Rpad / 64) x C floats. */
size_t tt_transpose_planes_colsum_workspace_bytes(int R, int C, int Rpad);
int tt_transpose_planes_colsum(const float* src, void* dst, int R, int C, int Rpad, float* colsum, void* workspace, size_t workspace_bytes,
                               tt_stream_t stream);
int tt_linear_bwd_data_planes(const void* dy_planes, long long dy_plane_stride, const void* wT_planes, long long wT_plane_stride,
                              int planes, const float* gelu_pre, float* dx, int M, int N, int K, void* workspace, size_t workspace_bytes,
                              tt_stream_t stream);   /* workspace: the K-split block or NULL (ABI 7) */
int tt_linear_bwd_weight_planes(const void* dyT_planes, long long dyT_plane_stride, const void* xT_planes, long long xT_plane_stride,
                                int planes, float* dw, int N, int K, int Mpad, void* workspace, size_t workspace_bytes,
                                tt_stream_t stream);
size_t tt_linear_bwd_weight_planes_workspace_bytes(int N, int K, int Mpad);

/* ---- k14: temporal label propagation (time_tuning.py:143-154 -> mask_propagation.py:396-496)
 *   xn   [fs, bs, n, D]  L2-normalised backbone tokens, time-major (frame t of clip b at [t][b])
 *   seg0 [bs, n, K] fp32 Sinkhorn assignment of frame 0 (the seed labels)
 *   labels [bs, n] int64 = argmax_K of the propagated map of the LAST frame
 *   pmap_last [bs, n, K] fp64 optional (the map itself).
 *   workspace: tt_label_propagate_workspace_bytes(...).
 * Accepted domain of the square entries (tt_label_propagate, _sims, _from_sims, _maps) - anything else is refused before a launch:
 *   fs >= 2, g, D, K, topk >= 1;  D % 4 == 0;  0 <= n_last_frames <= 7;  radius > 0 (the unrestricted variant is the grid entry's);
 *   win^2 * contexts <= 4096 candidates per query, win = min(2 * radius + 1, g), contexts = 1 + min(fs - 2, n_last_frames);
 *   bs <= 65535.  The per-query wave kernels (win <= 16, g * g <= 4096, K <= 512) put no bound on bs themselves, but every route
 *   computes its similarities with one batched product of bs x chunk problems on gridDim.y - the chunk of target frames is shortened so
 *   that bs * chunk <= 65535 - and the workgroup-per-query kernels carry bs on gridDim.y too: both limits are checked, each with a
 *   message of its own.  topk may exceed the candidates of a query (everything is then kept).
 * tt_label_propagate_route: the per-query kernel target frame t (1 <= t < fs) of such a call runs - 0 = the shape or the frame is
 *   refused, 1..4 = the wave kernel for <= 3 contexts and K <= 256, <= 3 and K <= 512, <= 8 and K <= 256, <= 8 and K <= 512 (contexts
 *   of THAT frame: 1 + min(t - 1, n_last_frames)), 5 / 6 = the workgroup kernel for <= 2048 / <= 4096 candidates.  Host only; the
 *   launcher dispatches on this value. */
int tt_label_propagate_route(int fs, int g, int K, int n_last_frames, int radius, int t);
int tt_label_propagate(const float* xn, const float* seg0, int64_t* labels, double* pmap_last, int bs, int fs, int g,
                       int D, int K, int n_last_frames, int radius, int topk, float temperature, int precision, void* workspace,
                       size_t workspace_bytes, tt_stream_t stream);
size_t tt_label_propagate_workspace_bytes(int bs, int fs, int g, int D, int K, int n_last_frames);
/* The same in two calls, for a caller that overlaps the halves with other work (round 6: the cosine similarities do not depend on seg0 - the
 * training step computes them on a side stream beside the Sinkhorn solve that produces seg0):
 *   tt_label_propagate_sims       the similarities of ALL target frames into `workspace` (tt_label_propagate_workspace_bytes).  Returns TT_OK,
 *                                 or 1 when they do not fit one chunk of this workspace (nothing is written: call tt_label_propagate);
 *   tt_label_propagate_from_sims  tt_label_propagate on a workspace tt_label_propagate_sims prepared (same shapes, same workspace).
 * Together they launch exactly what tt_label_propagate launches. */
int tt_label_propagate_sims(const float* xn, int bs, int fs, int g, int D, int K, int n_last_frames, int precision, void* workspace,
                            size_t workspace_bytes, tt_stream_t stream);
int tt_label_propagate_from_sims(const float* xn, const float* seg0, int64_t* labels, double* pmap_last, int bs, int fs, int g, int D, int K,
                                 int n_last_frames, int radius, int topk, float temperature, void* workspace, size_t workspace_bytes,
                                 tt_stream_t stream);

/* ---- N4: label-propagation EVALUATION (mask_propagation.py:816-833, DAVIS protocol
 *      n_last_frames 4, size_mask_neighborhood 12, topk 5), reusing k14.
 *   tt_label_propagate_maps  same propagation, but ALL fs-1 maps are returned, as propagate_labels does
 *                            (mask_propagation.py:448-496): pmap_all [fs-1, bs, n, K] fp64.  Workspace as above.
 *   tt_upsample_argmax       nn.functional.interpolate(maps, (R,R), mode="bilinear", align_corners=False) followed by
 *                            torch.max(dim=1) (mask_propagation.py:828-829), fused: maps [M, n, K] fp64 ->
 *                            labels_out [M, R, R] int64; the upsampled fp64 tensor is never written.  One kernel template
 *                            (csrc/upsample.hip) serves this entry, tt_upsample_argmax_hw (N9) and tt_upsample_argmax_f32 (N2);
 *                            taps, weights and the first maximum are the shared rule of csrc/interp.hpp.
 *   tt_confusion_counts      counts[gt*C + pred] += 1 over n pixels (labels outside [0,C) ignored), uint64 [C,C],
 *                            C <= 4096: the confusion matrix from which the Jaccard index (J) of the propagated masks and
 *                            the evaluator's matched mIoU (metrics.py:357-432) follow.  An LDS histogram up to C = 96,
 *                            global integer atomics beyond; any n > 0.
 *   tt_upsample_argmax takes M <= 65535 maps per call (they ride on gridDim.y) and R <= 32768. */
int tt_label_propagate_maps(const float* xn, const float* seg0, double* pmap_all, int bs, int fs, int g, int D, int K,
                            int n_last_frames, int radius, int topk, float temperature, int precision, void* workspace,
                            size_t workspace_bytes, tt_stream_t stream);
int tt_upsample_argmax(const double* maps, int64_t* labels_out, int M, int g, int K, int R, tt_stream_t stream);
int tt_confusion_counts(const int64_t* pred, const int64_t* gt, long long n, int C, unsigned long long* counts,
                        tt_stream_t stream);

/* ---- N15: segmented confusion counts - the matrices of every PredsmIoU.compute of one evaluate_localizations call (evaluation.py:250-310:
 *      per frame :266-275, per clip :276-289, per dataset :290-307 with Pascal's ignore label :304-305) and the per-frame counts behind
 *      PredsmIoU.compute_propagation_score (metrics.py:271-346, called by evaluation.py:228-246), in one launch.
 *   tt_confusion_counts_segments  pred [S, n] (pred_dtype: TT_LABELS_I16 = int16, what cluster_features returns, or TT_LABELS_I64 = int64,
 *                                 what proto_clustering returns), gt [S, n] int64 -> counts uint64 [S, Cg, Cp]:
 *                                   counts[s][g][p] += 1 for every element of segment s with 0 <= g < Cg, 0 <= p < Cp and, where
 *                                   has_ignore != 0, g != ignore_gt; every other element is skipped.
 *                                 tt_confusion_counts made rectangular, with an ignore value and a segment axis.  The entry zeroes counts.
 *                                 Integer atomics only: the result depends on neither order nor grid.  The segments ride on gridDim.y,
 *                                 65535 per launch, any S >= 1; pred and gt need only the alignment of their elements (16-byte loads are
 *                                 used where the addresses allow).  Element offsets are 64-bit.
 *   tt_confusion_segments_route   host only: 0 = (Cg, Cp) refused, 1 = a u32 histogram per workgroup in LDS (Cg * Cp <= 16384 cells, 64 KB:
 *                                 the over-clustering shape 21 x 500 among them), 2 = 64-bit global atomics (beyond, Cg, Cp <= 4096).
 *   Refused with TT_EINVAL and a message naming the numbers, nothing launched: null pointers, an unknown dtype code, S < 1, n < 1, Cg or Cp
 *   outside [1, 4096], S * Cg * Cp > 2^32 cells (32 GB of counts: the bound this entry addresses), S * n > 2^59, a misaligned pointer. */
#define TT_LABELS_I16 0
#define TT_LABELS_I64 1
int tt_confusion_segments_route(int Cg, int Cp);
int tt_confusion_counts_segments(const void* pred, int pred_dtype, const int64_t* gt, int S, long long n, int Cg, int Cp, long long ignore_gt,
                                 int has_ignore, unsigned long long* counts, tt_stream_t stream);

/* ---- N20: matching and scoring of every segment on the device - what PredsmIoU.compute_miou (metrics.py:357-432, with compute_score_matrix
 *      :435-474, scipy's linear_sum_assignment in _hungarian_match :481-488 and _original_match :489-505) derives from one confusion matrix, for ALL segments of an
 *      evaluate_localizations call in one launch straight behind tt_confusion_counts_segments.
 *   tt_match_segments           counts uint64 [S, Cg, Cp] (what tt_confusion_counts_segments wrote) -> per segment s
 *                                 score[s]       fp64: the mean Jaccard index over the present gt values (without gt value 0 unless
 *                                                involve_bg; 0.0 where nothing is left), summed in numpy's order;
 *                                 matched_bg[s]  fp64: 1 / n_gt (Hungarian), or the share of the present preds matched to the FIRST present
 *                                                gt class (many-to-one);
 *                                 tp, fp, fn     int64 [S, Cg], indexed by gt VALUE, 0 where the value is absent: the counts after every
 *                                                present pred value is renamed to its matched gt value (unmatched ones to 0);
 *                                 lut            int64 [S, Cp]: pred value -> matched gt value, 0 where unmapped or absent;
 *                                 info           int32 [S, 4]: status, n_gt, n_pred (present values), largest present pred value.
 *                               mode TT_MATCH_HUNGARIAN: linear_sum_assignment(1 - IoU) as scipy computes it, ties included (the transpose
 *                               where n_pred < n_gt, a descending column list, the last minimal unassigned or else the first minimal
 *                               position, swap-remove); TT_MATCH_MANY_TO_ONE: every present pred goes to the present gt class of largest
 *                               IoU, or precision where precision_based != 0 (read in this mode only), the first maximum in ascending
 *                               gt order.  fp64 throughout, correctly rounded divisions, no contraction: the bits of the host path.
 *                               status 0 = scored; 1 = no present gt value (an empty segment); 2 = a search overran its bound or met a
 *                               non-finite minimum; 3 = the segment total is 2^53 or more (counts no longer exact in fp64).  With a
 *                               non-zero status the segment's other outputs are 0 (n_gt, n_pred and the largest pred value stay).
 *                               One wave64 per segment, segments on the grid, any S >= 1; no allocation, no synchronisation, no
 *                               workspace.
 *   tt_match_segments_shape_ok  host only: 1 where 1 <= Cg <= 128 (numpy's mean stays inside one summation block) and 1 <= Cp <= 1024
 *                               (the per-segment vectors fit in LDS: 54 KB at 128 x 1024), else 0.
 *   Refused with TT_EINVAL and a message naming the numbers, nothing launched: null pointers, S < 1, a shape outside the rule, an unknown
 *   mode code, a misaligned pointer (8 bytes; info 4). */
#define TT_MATCH_HUNGARIAN 0
#define TT_MATCH_MANY_TO_ONE 1
int tt_match_segments_shape_ok(int Cg, int Cp);
int tt_match_segments(const unsigned long long* counts, int S, int Cg, int Cp, int mode, int precision_based, int involve_bg, double* score,
                      double* matched_bg, long long* tp, long long* fp, long long* fn, long long* lut, int* info, tt_stream_t stream);

/* ---- N17: overlay rendering and the prototype histogram - the qualitative side (time_tuning.py:305-457, evaluation.py:255-300).
 *   tt_overlay_grid   renders ALL F frames of a batch in one launch as out uint8 [F, 3, H + 2 pad, n W + (n + 1) pad]:
 *                     torchvision.utils.make_grid's layout for n tiles in one row (pad value 0, tile t at column t (W + pad) + pad, row
 *                     pad), which the reference fills on the host frame by frame (time_tuning.py:332-341 make_overlayed_grid, :305-319
 *                     localize_objects; evaluation.py:271-272,288,293 through my_utils.localize_objects, my_utils.py:41-65).
 *                       TT_OVERLAY_PHOTO   n = 2: [base | blend(base, colour(A))], frames float32 [F, 3, H, W];
 *                                          base_c = (uint8) clamp(trunc((x_c * std_c + mean_c) * 255), 0, 255), NaN -> 0 - three rounded
 *                                          fp32 operations, my_utils.denormalize (my_utils.py:68-70) and (img * 255).type(torch.uint8).
 *                                          mean3 / std3: HOST pointers to 3 floats, NULL = 0 / 1 (frames already in [0, 1]).
 *                       TT_OVERLAY_LABELS  n = 3: [colour(B) | colour(A) | blend(colour(B), colour(A))], B the ground truth, A the
 *                                          prediction; frames is not read.
 *                     colour(v) = palette[idx mod P] (palette uint8 [P, 3]; a true modulo, negative indices wrap) with
 *                     idx = lut[f * lut_stride + v] for labels_a where lut (int32) is given - lut_stride 0 = one table of lut_len entries
 *                     for all frames, else lut_stride >= lut_len; a v outside [0, lut_len) gives idx 0 - and idx = v otherwise.  The
 *                     LUT is a matching's pred value -> gt value table: labels_b, the ground truth, is never mapped.
 *                     blend = (uint8) trunc(fl(fl(a (1 - alpha)) + fl(b alpha))), three rounded fp32 operations without contraction:
 *                     draw_segmentation_masks' img * (1 - alpha) + colour * alpha and .to(uint8) with every pixel masked.  alpha is a
 *                     double: (float)alpha and (float)(1.0 - alpha) are what the kernel multiplies by, as torch rounds a Python scalar.
 *                     labels_a / labels_b [F, Hl, Wl] of label_dtype TT_LABELS_U8 / _I16 / _I64; where (Hl, Wl) != (H, W) they are read
 *                     through the DEVICE tables ytab int32 [H] (entries in [0, Hl)) and xtab int32 [W] (in [0, Wl)), which the kernel
 *                     does not check (timetuning_amd.hip_ops.overlay_grid checks the host copies); both NULL = maps of the frames' size.
 *                     A thread owns one 16-byte-aligned piece of an output row (tt_img_gather_nearest's idiom) and writes the padding
 *                     too; offsets are 64-bit; no LDS, no atomics, no workspace.
 *                     Refused with TT_EINVAL, nothing launched: null out / labels_a / palette (frames in the photo mode, labels_b in the
 *                     labels mode), an unknown mode or dtype code, F, H, W, Hl, Wl <= 0, P <= 0, pad < 0, one table without the other or
 *                     none with (Hl, Wl) != (H, W), a lut with lut_len <= 0 or 0 < lut_stride < lut_len, alpha outside [0, 1], an output
 *                     row (or row count) of more than 2^31 - 1 bytes, a misaligned frames / labels pointer.
 *   tt_upsample_argmax_hist_f32   maps [M, g * g, K] fp32 -> counts[k] += the number of the M * R * R output pixels whose bilinear arg-max
 *                     is k: the histogram of tt_upsample_argmax_f32's labels without the labels (time_tuning.py:354-375
 *                     get_similarity_histogram: proto_clustering's [N, 224, 224] map on the host, then torch.histc).  Per pixel the
 *                     device function tt_upsample_argmax_f32's kernel calls (csrc/upsample.hip): the same labels by construction.  counts uint64 [K] is ADDED to: the
 *                     caller zeroes it, and a loop over batches adds up.  A u32 histogram per workgroup in LDS, 64-bit integer atomics
 *                     for its non-zero bins: exact, independent of order and grid.  Refused with TT_EINVAL: null pointers, M, g, K, R
 *                     <= 0, K > 16384 (the LDS limit of tt_confusion_counts_segments), M > 65535, g or R > 32768, counts misaligned. */
#define TT_LABELS_U8 2        /* with TT_LABELS_I16 / TT_LABELS_I64 above; tt_overlay_grid only */
#define TT_OVERLAY_PHOTO 0
#define TT_OVERLAY_LABELS 1
int tt_overlay_grid(unsigned char* out, int mode, const float* frames, const float* mean3, const float* std3, const void* labels_a,
                    const void* labels_b, int label_dtype, int Hl, int Wl, const int* ytab, const int* xtab, const int* lut, int lut_len,
                    int lut_stride, const unsigned char* palette, int P, double alpha, int F, int H, int W, int pad, tt_stream_t stream);
int tt_upsample_argmax_hist_f32(const float* maps, unsigned long long* counts, int M, int g, int K, int R, tt_stream_t stream);

/* ---- N9: the evaluation propagation on RECTANGULAR token grids (frames at native size, e.g. 480 x 848 -> 30 x 53 tokens at patch 16)
 *   tt_label_propagate_grid_maps  tt_label_propagate_maps on a gh x gw grid (n = gh * gw, row-major tokens): xn [fs, bs, n, D], seg0
 *                                 [bs, n, K], pmap_all [fs-1, bs, n, K] fp64.  The window is restrict_neighborhood(gh, gw, radius)
 *                                 (mask_propagation.py:377-391), clipped at the row and the column edges separately; radius 0 is the
 *                                 unrestricted variant (no mask: the top-k over all ctx * n sources).  No cap on the candidates of a
 *                                 query; n_last_frames <= 7, radius >= 0, D % 4 == 0, bs <= 65535 (clips ride on gridDim.y; the chunk of
 *                                 target frames is shortened so that bs * chunk <= 65535, as on the square entries).  Workspace: tt_label_propagate_grid_workspace_bytes(...), the
 *                                 [ctx, n, n] fp32 similarities of each target frame held at once (as tt_label_propagate_maps'; about
 *                                 0.8 GB per target frame at 60 x 106 tokens with n_last_frames 4).
 *   tt_upsample_argmax_hw         tt_upsample_argmax for a gh x gw grid and an H x W output: maps [M, gh*gw, K] fp64 -> labels_out
 *                                 [M, H, W] int64 (bilinear, align_corners = False, then the first maximum over K). */
size_t tt_label_propagate_grid_workspace_bytes(int bs, int fs, int gh, int gw, int D, int K, int n_last_frames, int radius);
int tt_label_propagate_grid_maps(const float* xn, const float* seg0, double* pmap_all, int bs, int fs, int gh, int gw, int D, int K,
                                 int n_last_frames, int radius, int topk, float temperature, int precision, void* workspace,
                                 size_t workspace_bytes, tt_stream_t stream);
int tt_upsample_argmax_hw(const double* maps, int64_t* labels_out, int M, int gh, int gw, int K, int H, int W, tt_stream_t stream);

/* ---- N10: the optical-flow baseline of the evaluation (mask_propagation.py:265-346, :803-815; cv2 replaced, parity with cv2 unpinned)
 *   tt_farneback_plan             (host only) the pyramid of cv2.calcOpticalFlowFarneback: levels cut to the largest k with H, W * pyr_scale^k
 *                                 >= 32; levels_out = that k, sizes_out [2 (k + 1)] = (h, w) of levels 0..k, cvRound(side * pyr_scale^i)
 *                                 (half to even; the caller's array holds 2 (levels + 1) ints).  0 < pyr_scale < 1, 1 <= levels <= 64.
 *   tt_farneback_workspace_bytes  (host only) the workspace of tt_farneback_flow for F frames and P pairs of H x W (0: bad arguments):
 *                                 about (60 F + 40 P) H W bytes plus two coarse flow fields.
 *   tt_flow_gray_u8               replaces :807-813: clip [F, 3, H, W] fp32 RGB -> gray [F, H, W] uint8.  x 255 in fp32, torch's CPU uint8
 *                                 cast ((int64) trunc, modulo 256), then RGB2BGR + BGR2GRAY (R 4899 + G 9617 + B 1868 + 8192) >> 14.
 *   tt_farneback_flow             replaces dense_optical_flow's cv2.calcOpticalFlowFarneback(new, old, None, 0.5, 3, 15, 3, 5, 1.2, 0)
 *                                 (:299) for P pairs at once: frames [F, H, W] uint8, pairs int32 [P, 2] (DEVICE) = (prev, next) frame
 *                                 indices -> flow [P, H, W, 2] fp32 (dx, dy) with prev(x) ~ next(x + flow(x)).  Each frame's level images
 *                                 and polynomial expansions are computed once and shared by its pairs.  flags 0 only (the box-filter
 *                                 variant; OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_FARNEBACK_GAUSSIAN return TT_EINVAL), poly_n 5 or 7,
 *                                 1 <= winsize <= 127, iterations >= 1; a level Gaussian above 255 taps (frames beyond ~3 400 px at
 *                                 pyr_scale 0.5) returns TT_EINVAL.  A pair index outside [0, F) gives that pair a NaN flow and reads
 *                                 nothing.  Workspace: tt_farneback_workspace_bytes; no allocation, no float atomics (deterministic).
 *   tt_remap_nearest_labels       replaces interpolate_frames / propagate (:322-346): out[n, s] = cv2.remap(s == 0 ? first[n] :
 *                                 out[n, s - 1], coords + scale * flows[n, s], INTER_NEAREST) for s = 0..steps-1; first [N, H, W],
 *                                 flows [N, steps, H, W, 2], out [N, steps, H, W], labels uint8 (label_bytes 1) or int64 (8).  The map is
 *                                 fp32 with separate roundings (numpy's), rounded half to even, saturated to int16; outside reads 0. */
int tt_farneback_plan(int H, int W, double pyr_scale, int levels, int* levels_out, int* sizes_out);
size_t tt_farneback_workspace_bytes(int F, int P, int H, int W, double pyr_scale, int levels);
int tt_flow_gray_u8(const float* clip, uint8_t* gray, int F, int H, int W, tt_stream_t stream);
int tt_farneback_flow(const uint8_t* frames, int F, int H, int W, const int32_t* pairs, int P, double pyr_scale, int levels, int winsize,
                      int iterations, int poly_n, double poly_sigma, int flags, float* flow, void* workspace, size_t workspace_bytes,
                      tt_stream_t stream);
int tt_remap_nearest_labels(const void* first, const float* flows, void* out, int N, int steps, int H, int W, float scale, int label_bytes,
                            tt_stream_t stream);

/* ---- k15: CrossEntropyLoss(scores/temp, labels), mean over patches then batch
 *      (time_tuning.py:296-302), with its gradient w.r.t. scores.
 *   scores [rows,K]; labels int64[rows]; loss_out[1]; dscores [rows,K] (= d loss / d scores).
 *   row_weight [rows] or NULL: the --use_mask form, CrossEntropyLoss(reduction='none') * mask followed by the
 *   mean over ALL rows (time_tuning.py:226-227,298-300).
 *   workspace: tt_ce_workspace_bytes(rows). */
int tt_ce_loss_fwd_bwd(const float* scores, const int64_t* labels, const float* row_weight, float* loss_out, float* dscores,
                       int rows, int K, float temperature, void* workspace, size_t workspace_bytes, tt_stream_t stream);
size_t tt_ce_workspace_bytes(int rows);

/* ---- k13: queue FIFO update (time_tuning.py:258-261): shift down by m rows, write feats[idx[i]]
 *   at the head.  queue [Q,D]; feats [R,D]; idx int64[m].  scratch [Q,D] (caller-owned). */
int tt_queue_push(float* queue, float* scratch, const float* feats, const int64_t* idx, int Q, int D, int m,
                  tt_stream_t stream);

/* ---- k17: AdamW over a table of tensors (time_tuning.py:413-429; torch.optim.AdamW defaults)
 *   1 .. TT_MAX_TENSORS entries per call (tt_adamw_step and tt_scale_tensors refuse more; tt_adamw_ema_step takes any count and
 *   walks it in chunks of TT_MAX_TENSORS).  Lengths are free and may differ: the grid is sized by the longest entry, up to 1024
 *   workgroups, and strides.  step is the 1-based step count of every tensor in the call (>= 1). */
#define TT_MAX_TENSORS 40
typedef struct {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long n;
  float lr;
  float weight_decay;
} tt_adamw_tensor;
int tt_adamw_step(const tt_adamw_tensor* tensors, int count, int step, float beta1, float beta2, float eps,
                  tt_stream_t stream);

/* g[i] *= *scale_device for the `g` buffers (n floats each) of up to TT_MAX_TENSORS table entries (p, m, v, lr, weight_decay are
 * ignored), one launch: the chain rule of `loss.backward()` applied to the gradients the fused step produced
 * (time_tuning.py:420-423 calls backward on the scalar loss; its incoming gradient is a device scalar). */
int tt_scale_tensors(const tt_adamw_tensor* tensors, int count, const float* scale_device, tt_stream_t stream);

/* ---- k19: EMA teacher update (time_tuning.py:109-118): t = t*(1-m) + s*m over n floats.  Any n > 0 (n & 3 trailing floats
 *   included); both buffers 16-byte aligned. */
int tt_ema_update(float* teacher, const float* student, long long n, double momentum, tt_stream_t stream);

/* ---- misc elementwise used between the sites above (any n > 0; no alignment requirement) */
int tt_add_inplace(float* dst, const float* src, long long n, tt_stream_t stream);
/* Number of positions where two fp32 buffers differ BITWISE.  Decides, once, whether the EMA teacher's frozen tensors still equal the student's
 * (time_tuning.py:113-114 blends identical tensors for every frozen parameter), i.e. whether the teacher pass may reuse the
 * student's frozen-block activations.  count_out: device int64. */
int tt_count_mismatch(const float* a, const float* b, long long n, long long* count_out, tt_stream_t stream);

/* ---- N1: attention foreground mask, models.process_attentions (models.py:93-131), used by
 *      apply_attention_mask (models.py:133-144) on the --use_mask branch of TimeT.get_loss.
 *   Per frame: cls-query attention of the LAST block averaged over heads -> Gaussian blur (ksize x ksize, sigma,
 *   reflect padding; the reference uses 7 / 0.6) -> keep `threshold` (0.65) of the mass by ascending sort +
 *   cumulative sum -> drop 8-connected components of <= 2 pixels.  One launch, no host round trip (the
 *   reference labels components with skimage on the CPU).
 *   tt_foreground_mask           qkv [F,N,3*H*hd]: the last block's qkv activations (same buffer tt_attention_fwd
 *                                reads); the cls-row probabilities softmax(q_cls k_j * scale) are recomputed in the
 *                                kernel, so attn[F,H,N,N] is never materialised.
 *   tt_foreground_mask_from_probs cls_probs [F,H,N]: row 0 of the attention probabilities, already computed.
 *   mask_out [F,g*g] floats in {0,1}; blurred_out [F,g*g] optional (the blurred mean attention);
 *   margin_out [F,g*g] optional (|cumulative mass - (1-threshold)| per pixel: how far it is from the cut).
 *   Accepted domain: N = g*g + 1 with g*g <= 1024 patches (one workgroup holds a frame in LDS); ksize odd, <= 15, and
 *   ksize / 2 < g (reflect padding: the 7-tap blur needs g >= 4); 0 < threshold < 1; sigma > 0; H > 0; any F > 0.
 *   tt_foreground_mask also: head_dim a multiple of 4, <= 128, qkv 16-byte aligned. */
int tt_foreground_mask(const float* qkv, float* mask_out, float* blurred_out, float* margin_out, int F, int N, int H, int hd, int g,
                       float scale, float threshold, float sigma, int ksize, tt_stream_t stream);
int tt_foreground_mask_from_probs(const float* cls_probs, float* mask_out, float* blurred_out, float* margin_out, int F, int N,
                                  int H, int g, float threshold, float sigma, int ksize, tt_stream_t stream);

/* ---- N2: evaluator clustering - the device side of clustering.cluster_features / proto_clustering
 *      (clustering.py:20-117), my_utils.normalize_and_transform (my_utils.py:19-37) and of the Lloyd iterations the
 *      reference delegates to faiss.Kmeans(d, k, niter=50, nredo=5, seed=1).
 *   tt_col_moments              per-column mean and population variance (StandardScaler, my_utils.py:24-30), fp64.
 *   tt_upsample_bilinear_tokens token maps [M, g*g, C] -> [M, R*R, C] as nn.functional.interpolate(x.double(), (R,R),
 *                               mode="bilinear").float() (clustering.py:34-36).  Its taps are csrc/interp.hpp's lin_tap in fp64,
 *                               the function tt_bilinear_adjoint_tokens (N5) takes its own from.
 *   tt_upsample_argmax_f32      fp32 twin of tt_upsample_argmax for proto_clustering's prototype scores (clustering.py:101-104).
 *   tt_kmeans_assign            labels[p] = argmin_j |x_p - c_j|^2 (first minimum) over centroids [k, d]; dist2 optional.
 *   tt_kmeans_accumulate        sums[k, d] (fp64) and counts[k] of the points per label, deterministic (no atomics).
 *   THE K-MEANS CONTRACT, shared by every k-means entry here, in N12 and in N13 (one statement in the code as well: csrc/kmeans.hpp), so
 *   that wherever two of them take a shape their outputs are equal bit for bit:
 *     distance      per centroid j one fp32 accumulator: s = 0.f, then over the columns in increasing order df = x - c, s += df * df
 *                   (contracted to one fma);
 *     assignment    the FIRST minimum: from best = INFINITY, besti = 0, updated by a strict s < best in increasing j;
 *     accumulation  the points are cut into clamp(ceil(P / 128), 1, 4096) blocks of consecutive points; per (cluster, column) fp32 from
 *                   0.f in point order inside a block, the partials widened to fp64 and added in block order; integer counts.
 *   Accepted domains (each refusal is a TT_EINVAL with the entry's own message; nothing is launched):
 *     tt_col_moments              0 < cols <= 1024; any rows > 0 (1024 workgroups from 262 144 rows on).  The sums are taken about
 *                                 the column's first row, so a small variance beside a large mean survives.
 *     tt_upsample_bilinear_tokens, tt_upsample_argmax_f32, tt_upsample_argmax (N4): M <= 65535 maps per call (they ride on
 *                                 gridDim.y), R <= 32768; any g, C / K > 0 - R < g (down-sampling), R = g and g = 1 included.
 *     tt_kmeans_assign, tt_kmeans_accumulate: ONE rule for both, tt_kmeans_shape_ok(d, k) - a Lloyd iteration calls one after the
 *                                 other, and clustering.Kmeans asks before its first assignment.  Both hold k * d <= 16384 floats
 *                                 of centroids (sums) in LDS; for d <= 64 the assignment's tile of 256 points shares it,
 *                                 k * d + 256 (d | 1) floats <= 128 KB, which binds at d = 64 only (k <= 252).  k = 300 at d = 50,
 *                                 the N6 over-clustering, fits.  Any P > 0: beyond 4096 x 256 points the assignment strides, beyond
 *                                 4096 x 128 a workgroup of the accumulation sums ceil(P / 4096) points.  Labels given to the
 *                                 accumulation must lie in [0, k). */
int tt_kmeans_shape_ok(int d, int k);   /* 1 when tt_kmeans_assign and tt_kmeans_accumulate take (d, k), else 0 */
int tt_kmeans_assign_route(int d);      /* which kernel tt_kmeans_assign runs at d: 16 / 64 = the point in that many registers, 0 = rows
                                           read in place (d > 64).  The three compute the same bits; for tests and profilers' labels. */
int tt_affine_cols_inplace(float* x, const float* scale, const float* shift, long long rows, int cols,
                           tt_stream_t stream); /* x[r][c] = x[r][c] * scale[c] + shift[c] (StandardScaler.transform) */
size_t tt_col_moments_workspace_bytes(long long rows, int cols);
int tt_col_moments(const float* x, double* mean, double* var, long long rows, int cols, void* workspace, size_t workspace_bytes,
                   tt_stream_t stream);
int tt_upsample_bilinear_tokens(const float* x, float* out, int M, int g, int C, int R, tt_stream_t stream);
int tt_upsample_argmax_f32(const float* maps, int64_t* labels_out, int M, int g, int K, int R, tt_stream_t stream);
int tt_kmeans_assign(const float* x, const float* centroids, int32_t* labels, float* dist2, long long P, int d, int k,
                     tt_stream_t stream);
size_t tt_kmeans_accumulate_workspace_bytes(long long P, int d, int k);
int tt_kmeans_accumulate(const float* x, const int32_t* labels, double* sums, long long* counts, long long P, int d, int k,
                         void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* ---- N12: k-means beyond the LDS limit - the same two passes for centroid sets tt_kmeans_shape_ok refuses, which
 *      the reference's over-clustering needs: faiss.Kmeans(50, 500) at clustering.py:39-41,55-57,69-71 (cluster_features, the three
 *      protocols; evaluation.py:431-441 with many_to_one) and faiss.Kmeans(256, num_classes) at clustering.py:108-110 (proto_clustering).
 *   The centroids (the sums) pass through LDS in tiles of tile_k rows; the arithmetic per output number is the k-means contract (N2
 *   above), so wherever both pairs take a shape the outputs are equal bit for bit, whatever tile_k is.
 *   tt_kmeans_tiled_shape_ok      1 for 1 <= d <= 1024, k >= 1, k * d < 2^31, else 0.
 *   tt_kmeans_tile_centroids      the default tile at d: the most rows of d floats that fill at most 64 KB (0 outside 1 <= d <= 1024).
 *   tt_kmeans_assign_tiled        tt_kmeans_assign (clustering.py:39-41,55-57,69-71,108-110: index.search(x, 1) and the assignment of every
 *                                 Lloyd iteration of train): first minimum, also across tile boundaries; dist2 optional.
 *   tt_kmeans_accumulate_tiled    tt_kmeans_accumulate (the same sites: the centroid update of every Lloyd iteration of train);
 *                                 labels outside [0, k) are skipped.  No atomics; the workspace is that of tt_kmeans_accumulate,
 *                                 one fp64 partial per (workgroup, cluster, column) - 8 k (d + 1) bytes per 128 points, at most 4096 times.
 *   tile_k: 0 = the default, or any value in 1 ... tt_kmeans_tile_centroids(d); a larger one is refused (TT_EINVAL, the message
 *   names both numbers), as is a shape beyond tt_kmeans_tiled_shape_ok.  Nothing is launched on a refusal.  Any P > 0. */
int tt_kmeans_tiled_shape_ok(int d, int k);   /* 1 when the two tiled entries take (d, k): what clustering.py:39-41,55-57,69-71,108-110 may ask */
int tt_kmeans_tile_centroids(int d);          /* the default and largest tile_k at d; pure host function, like the shape rule */
int tt_kmeans_assign_tiled(const float* x, const float* centroids, int32_t* labels, float* dist2, long long P, int d, int k, int tile_k,
                           tt_stream_t stream);
size_t tt_kmeans_accumulate_tiled_workspace_bytes(long long P, int d, int k, int tile_k);
int tt_kmeans_accumulate_tiled(const float* x, const int32_t* labels, double* sums, long long* counts, long long P, int d, int k,
                               int tile_k, void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* ---- N13: the whole Lloyd loop of B k-means problems in one launch - what the frame-wise and sample-wise protocols of
 *      cluster_features ask per frame / per clip: faiss.Kmeans(50, k, niter=50, nredo=5).train(x) at clustering.py:39-41,55-57
 *      (Clustering::train as configured there, after its subsample) and the index.search(x, 1) that follows it.
 *   tt_kmeans_fit_batched      x [B, n, d] (B problems of equal shape), init int32 [nredo, k] (rows of a problem's points that seed
 *                              redo r, shared by all problems; init_host is a HOST copy of it, checked before the launch) ->
 *                              centroids [B, nredo, k, d], obj fp64 [B, nredo], status int32 [B, nredo].  One workgroup per
 *                              (problem, redo) runs niter iterations; no workgroup waits on another.  Per output number the
 *                              arithmetic is that of the loop over tt_kmeans_assign / tt_kmeans_accumulate:
 *                                assignment, accumulation   the k-means contract (N2 above);
 *                                update        c = (float)(sum / (double)count) where count > 0, the old centroid otherwise;
 *                                objective     obj[b][r] is the LAST iteration's fp64 sum of the points' best distances (to the
 *                                              centroids before the last update), summed in an order fixed by n alone;
 *                                empty cluster an iteration whose counts hold a zero ends that (problem, redo): status = the 1-based
 *                                              iteration, its centroids and obj are unspecified.  Otherwise status = 0.  faiss'
 *                                              split is not done here: the caller reruns such a problem on the loop.
 *   tt_kmeans_assign_batched   x [B, N, d], centroids [B, k, d] -> labels int32 [B, N] (+ dist2 [B, N], optional): tt_kmeans_assign
 *                              per problem, bit for bit (tt_kmeans_assign IS this kernel at one problem); the problems ride on
 *                              gridDim.y, 65535 per launch, any B >= 1.
 *   tt_kmeans_fit_shape_ok     1 for 1 <= d <= 64 (the point's row in registers), 1 <= k <= n <= 2^20 and 16 k d + 4 k bytes within
 *                              128 KB of LDS (fp64 sums, centroids, one block's fp32 sums, counts): k <= 127 at d = 64, k <= 163 at
 *                              d = 50; every 1 <= d, k <= 64 with k <= n <= 256 k is inside.  Else 0.
 *   tt_kmeans_fit_workspace_bytes   the labels of every (problem, redo), 4 B nredo n bytes; 0 for a refused shape.
 *   tt_kmeans_assign_batched takes the (d, k) of tt_kmeans_shape_ok.  Refused with TT_EINVAL and a message naming the numbers, nothing
 *   launched: null pointers, B outside 1 ... 65535 (fit), niter < 1, nredo < 1, n < k, an init index outside [0, n), a shape beyond
 *   the rule, a workspace that is too small. */
int tt_kmeans_fit_shape_ok(long long n, int d, int k);   /* pure host function, like tt_kmeans_shape_ok */
size_t tt_kmeans_fit_lds_bytes(long long n, int d, int k);   /* the LDS a fit workgroup asks for: as many blocks' fp32 sums side by side
                                                                as fit 72 KB (two workgroups per CU), at least one; 0 = refused */
size_t tt_kmeans_fit_workspace_bytes(int B, int nredo, long long n, int d, int k);
int tt_kmeans_fit_batched(const float* x, const int32_t* init, const int32_t* init_host, float* centroids, double* obj, int32_t* status,
                          int B, long long n, int d, int k, int nredo, int niter, void* workspace, size_t workspace_bytes,
                          tt_stream_t stream);
int tt_kmeans_assign_batched(const float* x, const float* centroids, int32_t* labels, float* dist2, int B, long long N, int d, int k,
                             tt_stream_t stream);

/* ---- N18: tt_kmeans_fit_batched with faiss' split of empty clusters done on the device - what Clustering::train does between the
 *      iterations of the same faiss.Kmeans(50, k, niter=50, nredo=5).train(x) calls (clustering.py:39-41,55-57; split_clusters as
 *      clustering.Kmeans._split_empty restates it), the normal case under use_mask=True (evaluation.py:411-427,461-462), where the
 *      background tokens are one and the same point.
 *   tt_kmeans_fit_batched_split   the arguments, outputs, arithmetic and refusals of tt_kmeans_fit_batched, plus draws fp64 [n_draws]
 *                              in device memory: the first n_draws values of numpy.random.RandomState(1234).random_sample(), the
 *                              generator the host re-creates at every split call.  After the update of an iteration whose counts
 *                              hold a zero the workgroup splits on its own centroids and counts and goes on (the draw index starts
 *                              at 0 at every such call):
 *                                the empty clusters ci in increasing order; the whole call stops where n <= k or the largest count
 *                                is <= 1; the donor walk starts at cj = 0 and accepts where draw < (double)(count[cj] - 1) /
 *                                (double)(n - k), else cj = (cj + 1) % k, and after more than 64 k refusals takes the first arg-max
 *                                of the counts; c[ci][j] = c[cj][j] * s_j from the old donor row, then c[cj][j] = c[cj][j] * (2 - s_j),
 *                                s_j = 1 + 2^-10 (j even), 1 - 2^-10 (j odd), single fp32 products; count[ci] = count[cj] / 2, then
 *                                count[cj] -= count[ci].  Later splits of a call see what earlier ones changed.
 *                              obj is taken before the split, which also runs after the last update.  status = 0, or the 1-based
 *                              iteration whose split would have read past the table: that (problem, redo) ends there, centroids and
 *                              obj unspecified, and the caller reruns the problem on the loop.  Trip counts are bounded by n_draws
 *                              and 64 k + 1 tries per empty cluster; no workgroup waits on another; the LDS rule is unchanged.
 *   Refused like tt_kmeans_fit_batched, and for a null draws or n_draws < 1. */
int tt_kmeans_fit_batched_split(const float* x, const int32_t* init, const int32_t* init_host, float* centroids, double* obj,
                                int32_t* status, int B, long long n, int d, int k, int nredo, int niter, void* workspace,
                                size_t workspace_bytes, const double* draws, int n_draws, tt_stream_t stream);

/* ---- N28: the large k-means fits as one enqueued device loop - the faiss.Kmeans(50, k, niter=50, nredo=5).train(x) of the dataset-wise
 *      protocol (clustering.py:69-71; k = 500 in the over-clustering evaluation) and the faiss.Kmeans(dim, k_fg_extraction).train of
 *      cluster-based foreground extraction (cluster_based_foreground_extraction.py:273-275, 384 raw feature columns), whose centroids
 *      do not fit one workgroup's LDS (tt_kmeans_fit_shape_ok refuses them), so that they ran clustering.Kmeans._iterate: per Lloyd
 *      iteration a dozen launches and two host synchronisations.
 *   tt_kmeans_fit_loop         x [n, d], init int32 [nredo, k] (+ init_host, a HOST copy checked before the first launch) -> centroids
 *                              [nredo, k, d], obj fp64 [nredo], status int32 [nredo].  Every redo and iteration is enqueued on
 *                              `stream`: between the first launch and the caller's read-back of obj and status there is no host
 *                              synchronisation, no read-back and no allocation (it can be captured into a graph).  Kernel
 *                              boundaries are the only ordering between workgroups: no flag, no counter another workgroup spins on,
 *                              no cooperative launch.  Per output number the arithmetic is that of the host loop over the N2 / N12
 *                              entries, so a fit returns that loop's bits:
 *                                assignment    the k-means contract (N2 above) - the resident kernel where tt_kmeans_shape_ok(d, k)
 *                                              and tile_k == 0, else the tiled one (a tile_k given asks for it; the bits are the same) -
 *                                              with the redo on a grid axis: every redo reads the ONE point set, its own centroids;
 *                                accumulation  the k-means contract, the redo on a grid axis;
 *                                update        c = (float)(sum / (double)count) where count > 0, the old centroid otherwise;
 *                                split         after the update, once per (redo, iteration) whose counts hold a zero: the statement of
 *                                              N18 above (the same device function), on an int copy of that iteration's counts that is
 *                                              not carried on; at d > 64 lane j of the one wave owns columns j, j + 64, ..., each still
 *                                              a single fp32 product of the old donor row.  draws == NULL or n_draws == 0: no split;
 *                                objective     obj[r] = the LAST iteration's dist2 summed in fp64 in an order fixed by n alone; it
 *                                              agrees with another fp64 summation order to about n * 2^-53 relative.
 *                              status[r] = 0, or the 1-based iteration whose split would have read past the table (without a table:
 *                              the first iteration with an empty cluster).  Every later launch leaves that redo alone (a uniform
 *                              early exit on the status word); its centroids and obj are unspecified and the caller reruns the fit
 *                              on the host loop.
 *   redo_group                 how many redos ride one launch: 0 = all of them, fewer = several passes over the iterations.  The
 *                              result does not depend on it; the workspace does.
 *   tt_kmeans_loop_shape_ok    1 for the tiled pair's rule (1 <= d <= 1024, k >= 1, k * d < 2^31) with k <= n <= 2^31 - 1, else 0.
 *   tt_kmeans_loop_workspace_bytes   for redo_group (0 = nredo) redos in flight: the accumulation's fp64 partials
 *                              (tt_kmeans_accumulate_workspace_bytes each: 200 MB at n = 128 000, d = 50, k = 500), the folded sums
 *                              and counts, the labels and the last dist2 (4 n bytes each), the split's counts; 0 for a refused shape,
 *                              nredo outside 1 ... 65535 or redo_group < 0.
 *   Refused with TT_EINVAL and a message naming the numbers, nothing launched: null pointers, niter < 1, nredo outside 1 ... 65535,
 *   redo_group < 0, n_draws < 0 (or > 0 without a table), a shape beyond the rule, a tile_k outside 0 ... tt_kmeans_tile_centroids(d),
 *   an init index outside [0, n), a workspace that is too small or not aligned to 8 bytes. */
int tt_kmeans_loop_shape_ok(long long n, int d, int k);   /* pure host function, like tt_kmeans_fit_shape_ok */
size_t tt_kmeans_loop_workspace_bytes(long long n, int d, int k, int nredo, int redo_group);
int tt_kmeans_loop_last_offsets(long long n, int d, int k, int nredo, int redo_group, size_t* labels_offset,
                                size_t* dist2_offset);   /* byte offsets, in a workspace of that query, of the last iteration's labels int32
                                                            [g][n] and dist2 fp32 [g][n] of the LAST pass's g redos in flight (for tests
                                                            and tools; the layout is the library's); 1, or 0 for what the query refuses */
int tt_kmeans_fit_loop(const float* x, const int32_t* init, const int32_t* init_host, float* centroids, double* obj, int32_t* status,
                       long long n, int d, int k, int nredo, int niter, int tile_k, int redo_group, const double* draws, int n_draws,
                       void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* ---- N3(SURVEY.md 8(f)): the clip input pipeline - the pixel work of video_transformations.py as wired at
 *      time_tuning.py:588-593, bit-exact with Pillow (which the reference calls per frame on the host).
 *   Frames are interleaved uint8 RGB [F, H, W, 3] in device memory.
 *   tt_img_resample_h   horizontal pass of Image.resize(BILINEAR) (Resample.c) over the crop rows y0..y0+h, columns starting
 *                       at x0: out [F, h, OW, 3].  coeffs int32 [OW, ksize] / bounds int32 [OW, 2] are Resample.c's 22-bit taps
 *                       (device memory; timetuning_amd.video_transformations.resample_coeffs builds them on the host).
 *   tt_img_resample_v   vertical pass over in [F, Hin, W, 3] starting at row y0: either out_u8 [F, OH, W, 3] or out_f32
 *                       [F, 3, OH, W] = ClipToTensor(mean, std) of the (optionally horizontally flipped) result
 *                       (video_transformations.py:168-179,262-276); mean3 / std3 are HOST pointers to 3 floats.
 *   tt_img_color        in place: mode 0 RandomGrayscale's convert("L") replicated to 3 channels; 1 / 2 / 3 torchvision
 *                       adjust_brightness / adjust_contrast / adjust_saturation (ImageEnhance = Blend.c); 4 adjust_hue
 *                       (hue_shift = uint8(hue_factor * 255)).  gray_sums: F uint64 of workspace for mode 2.
 *   tt_img_box_blur     one pass of BoxBlur.c along x (direction 0) or y (1); ImageFilter.GaussianBlur(radius) is three x
 *                       passes then three y passes with (radius, ww, fw) from the box radius (video_transformations.py:604-647). */
int tt_img_resample_h(const unsigned char* in, unsigned char* out, const int* coeffs, const int* bounds, int F, int H, int W, int y0, int x0,
                      int h, int OW, int ksize, tt_stream_t stream);
int tt_img_resample_v(const unsigned char* in, unsigned char* out_u8, float* out_f32, const int* coeffs, const int* bounds, int F, int Hin,
                      int W, int y0, int OH, int ksize, int flip, const float* mean3, const float* std3, tt_stream_t stream);
int tt_img_color(unsigned char* img, int F, int H, int W, int mode, float factor, int hue_shift, unsigned long long* gray_sums,
                 tt_stream_t stream);
int tt_img_box_blur(const unsigned char* in, unsigned char* out, int F, int H, int W, int direction, int radius, unsigned ww, unsigned fw,
                    tt_stream_t stream);

/* ---- N11: annotation clips through the input pipeline - nearest-neighbour gathering, the only resampling a label map may
 *      see (video_transformations.py:149-157,189-237,366-419,498-601 and Image.rotate of :551), bit-exact with Pillow.
 *   Clips are uint8 [F, H, W, C] in device memory with C = 1 (label maps, [F, H, W]) or C = 3 (interleaved RGB frames).
 *   tt_img_gather_nearest   out[f, y, x, :] = in[f, ytab[y], xtab[x], :].  ytab int32 [OH] / xtab int32 [OW] are device memory
 *                       and built by the caller (timetuning_amd.video_transformations.nearest_table: crop offset + Pillow's
 *                       NEAREST resize + a flip as a reversed table); every entry must lie in [0, Hin) / [0, Win) - the
 *                       kernel does not look (timetuning_amd.hip_ops.img_gather_nearest checks the host copies).
 *                       Exactly one output: out_u8 [F, OH, OW, C], or out_f32 planar [F, C, OH, OW] = ClipToTensor:
 *                       C = 3 ((float)v / 255 - mean[c]) / std[c] with the arithmetic of tt_img_resample_v (mean3 / std3 HOST
 *                       pointers to 3 floats, required), C = 1 (float)v / 255 as one IEEE fp32 division (mean3 / std3 ignored).
 *                       Domain: C in {1, 3}; 1 <= Hin, Win, OH, OW <= 32767; F >= 1 and F (uint8 output) or F * C (float
 *                       output) <= 65535.  Buffers may exceed 2^31 bytes (64-bit element offsets).
 *   tt_img_affine_nearest   Pillow's nearest affine transform with zero fill (Geometry.c affine_fixed; what Image.rotate(angle)
 *                       runs): out [F, H, W, C], out[f, y, x] = in[f, yin, xin] with xin = (a2 + a1 y + a0 x) >> 16,
 *                       yin = (a5 + a4 y + a3 x) >> 16 (64-bit, arithmetic shifts) when 0 <= xin < W and 0 <= yin < H, else 0.
 *                       a6 = {a0 .. a5}: HOST pointer to the six 16.16 fixed-point integers
 *                       (timetuning_amd.video_transformations.rotate_coeffs).  out must not alias in.
 *                       Domain: C in {1, 3}; 1 <= H, W <= 16384; 1 <= F <= 65535; the four corners (0 | W, 0 | H) must map
 *                       strictly inside +-32768 source pixels - beyond that Pillow leaves its fixed-point path.
 *   Outside its domain a call returns TT_EINVAL and launches nothing. */
int tt_img_gather_nearest(const unsigned char* in, unsigned char* out_u8, float* out_f32, const int* ytab, const int* xtab, int F, int Hin,
                          int Win, int C, int OH, int OW, const float* mean3, const float* std3, tt_stream_t stream);
int tt_img_affine_nearest(const unsigned char* in, unsigned char* out, int F, int H, int W, int C, const int* a6, tt_stream_t stream);

/* ---- N5: linear-probe fine-tuning, linear_finetune.py - a 1x1-conv head on frozen features
 *      (linear_finetune.py:13-31), CrossEntropyLoss(ignore_index=255) at mask resolution and torch.optim.SGD (:66-86).
 *      The reference upsamples the D-channel features to R x R and then applies the conv; both are linear and the bilinear
 *      weights sum to 1, so here the head runs at token resolution on C channels and only the C logits are upsampled.
 *   Shapes: B images, g x g tokens (g <= 64), D feature channels (D % 4 == 0, D <= 1024), C classes (1..256), R x R masks
 *   (R <= 1024); anything else returns TT_EINVAL before any launch.
 *   tt_probe_logits             logits [rows, C] = feats [rows, D] W^T + b, W = the conv weight [C, D, 1, 1] as [C, D]; b may be
 *                               NULL (linear_finetune.py:30, in the commuted order).  fp32 FMA, one pass over feats.
 *   tt_probe_upsample_ce        nn.functional.interpolate(logits, (R,R), mode="bilinear") -> CrossEntropyLoss(ignore_index=255)
 *                               -> backward (linear_finetune.py:26-30,81-84), fused: logits_low [B, g*g, C], labels int64
 *                               [B, R, R] -> loss_out[1] (mean over the valid pixels; NaN if there are none), dlogits_low
 *                               [B, g*g, C] = d loss / d logits_low (0 if there are no valid pixels), counts_out int64[2] =
 *                               {valid pixels, invalid labels (outside [0, C) and not 255)}.  Invalid labels are only counted.
 *                               The mask-resolution logits are never written; no float atomics (bitwise repeatable).  Two
 *                               launches.  workspace: tt_probe_upsample_ce_workspace_bytes(B, g).
 *   tt_bilinear_adjoint_tokens  d_low [B, g*g, C] from d_hi [B, R*R, C]: the adjoint of tt_upsample_bilinear_tokens (autograd of
 *                               linear_finetune.py:26-27 in the commuted order), the same deterministic gather.
 *   tt_probe_wgrad              dw [C, D] = dlogits^T feats, db [C] = column sums of dlogits (db may be NULL), over `rows` rows,
 *                               times *scale_device if it is not NULL (the incoming gradient of the loss).  Split rows, fixed
 *                               fold order, no atomics.  workspace: tt_probe_wgrad_workspace_bytes(rows, D, C).
 *   tt_sgd_step                 torch.optim.SGD (linear_finetune.py:66,85; dampening 0, no Nesterov) over up to TT_MAX_TENSORS
 *                               tt_adamw_tensor entries: d = g + weight_decay p; with momentum != 0, m = d if first_step else
 *                               momentum m + d, and d = m (m is the momentum buffer, v is unused); p -= lr d. */
int tt_probe_logits(const float* feats, const float* weight, const float* bias, float* logits, long long rows, int D, int C,
                    tt_stream_t stream);
size_t tt_probe_upsample_ce_workspace_bytes(int B, int g);
int tt_probe_upsample_ce(const float* logits_low, const int64_t* labels, float* dlogits_low, float* loss_out, long long* counts_out,
                         int B, int g, int C, int R, void* workspace, size_t workspace_bytes, tt_stream_t stream);
int tt_bilinear_adjoint_tokens(const float* d_hi, float* d_low, int B, int g, int C, int R, tt_stream_t stream);
size_t tt_probe_wgrad_workspace_bytes(long long rows, int D, int C);
int tt_probe_wgrad(const float* dlogits, const float* feats, const float* scale_device, float* dw, float* db, long long rows, int D,
                   int C, void* workspace, size_t workspace_bytes, tt_stream_t stream);
int tt_sgd_step(const tt_adamw_tensor* tensors, int count, float momentum, int first_step, tt_stream_t stream);

/* ---- N6: cluster-based foreground extraction, cluster_based_foreground_extraction.py - over-cluster maps scored
 *      against the ViT-attention foreground, a precision cut tuned on the train set, foreground masks on the val set.  Everything the
 *      reference computes with per-image, per-cluster Python loops reduces to per-(image, cluster) integer counts.
 *   Shapes: M images of P = R * R pixels (P <= 2^24), k clusters (1..4096); anything else returns TT_EINVAL before any launch.
 *   range_flag: a device int the kernels set to 1 when a cluster id lies outside [0, k) (the caller zeroes and reads it).
 *   tt_cbfe_cluster_stats       clusters, attn, gt: int64 [M, P] -> stats int32 [M, k, 3] = {n, tp_attn, tp_gt} per (image, cluster):
 *                               pixels of the cluster, of those the ones with attn == 1, and the ones in the GT foreground;
 *                               gt_fg int32 [M] = GT foreground pixels per image.  GT foreground is gt != 0 (ignore < 0) or
 *                               gt != 0 && gt != ignore (eval_jac's with_boundary True / False, :117-120).  attn and gt may
 *                               be NULL (their counts are 0).  Pixels with an out-of-range id raise range_flag and are not counted.  Integer
 *                               LDS atomics, one workgroup per image: the result is independent of the order of the adds.
 *                               Replaces get_cluster_precs' loops (:85-101) and eval_jac's sums (:117-125).
 *   tt_cbfe_cluster_precs       stats -> precs fp64 [k], occurrences int32 [k]: get_cluster_precs (:85-107) bit for bit - per cluster
 *                               the sum of tp_attn / n (fp64, IEEE division) over the images with n > 0 in increasing image order,
 *                               divided by the occurrence count (NaN for a cluster that never occurs).
 *   tt_cbfe_cut_jaccard         find_good_threshold's Jaccards (:140-153 through eval_jac, :111-129): candidate c marks the clusters
 *                               order[starts[c] .. k) as foreground; per image inter = the suffix sum of tp_gt, union = gt_fg +
 *                               suffix(n) - inter, iou = float(inter) / float(union) (fp32, correctly rounded; 0 / 0 = NaN);
 *                               jac [C] = the sequential fp32 sum of iou over the images in order, divided by M in fp32.  iou
 *                               (optional, fp32 [C, M]) receives the per-image values.  order int32 [k], starts int32 [C]; the
 *                               kernel never sorts.  workspace: tt_cbfe_cut_jaccard_workspace_bytes(M, C).
 *   tt_cbfe_apply_fg            make_post_matching_maps (:221-227): mask int64 [total] = fg_table[clusters[i]] (uint8 [k], 0 / 1).
 *   tt_nearest_upsample_labels  token labels int32 [M, g * g] -> pixel labels int64 [M, R * R] through the row / column tables iy, ix
 *                               (int32 [R], entries in [0, g)) of F.interpolate(mode="nearest") (:229-235 applied to labels). */
int tt_cbfe_cluster_stats(const int64_t* clusters, const int64_t* attn, const int64_t* gt, int32_t* stats, int32_t* gt_fg, int M, long long P,
                          int k, long long ignore, int* range_flag, tt_stream_t stream);
int tt_cbfe_cluster_precs(const int32_t* stats, double* precs, int32_t* occurrences, int M, int k, tt_stream_t stream);
size_t tt_cbfe_cut_jaccard_workspace_bytes(int M, int C);
int tt_cbfe_cut_jaccard(const int32_t* stats, const int32_t* gt_fg, const int32_t* order, const int32_t* starts, float* jac, float* iou,
                        int M, int k, int C, void* workspace, size_t workspace_bytes, tt_stream_t stream);
int tt_cbfe_apply_fg(const int64_t* clusters, const uint8_t* fg_table, int64_t* mask, long long total, int k, int* range_flag,
                     tt_stream_t stream);
int tt_nearest_upsample_labels(const int32_t* tok, const int32_t* iy, const int32_t* ix, int64_t* out, int M, int g, int R,
                               tt_stream_t stream);

/* ---- N7: DAVIS J&F, the semi-supervised VOS metrics of mask_propagation.py:501-715 (db_eval_iou, db_eval_boundary /
 *      f_measure / _seg2bmap) as integer counts; the host turns them into J and F with the reference's fp64 expressions.
 *   tt_davis_jf_counts   pred, gt: label maps [T, H, W] of dtype 0 = uint8 or 1 = int64 (pred_dtype / gt_dtype, independently);
 *                        void_mask: uint8 [T, H, W] or NULL (non-zero = void).  Object o (1..O) is label == o; any other value is
 *                        "not object o" (no range error).  counts: int64 [O, T, 6] = {J intersection, J union, n_fg, n_gt, fg_match,
 *                        gt_match}: the J pixels are the non-void ones; for F both masks are multiplied by "not void" first, their
 *                        boundary maps are _seg2bmap's (interior s^e | s^s | s^se, last row s^e, last column s^s, bottom-right 0 -
 *                        at the image edge), and fg_match = |fg_boundary & dilate(gt_boundary)|, gt_match the other way round, with
 *                        cv2.dilate's rule (dst(y, x) = OR over the set (i, j) of src(y + i - anchor_y, x + j - anchor_x), pixels
 *                        outside the image contribute nothing).  The structuring element is passed from the HOST as spans (int
 *                        [el_rows][2] = first, last set column of each row; first > last: an empty row) with its anchor (cv2's default
 *                        is (rows / 2, cols / 2)); el_rows, el_cols <= 127 (a disk of radius 63: 4K frames at bound_th 0.008), and the
 *                        anchor at most 63 columns from either side; a larger element returns TT_EINVAL.  The call clears counts
 *                        (hipMemsetAsync on `stream`), then adds per-tile sums with 64-bit integer atomics: deterministic.
 *   tt_davis_seg2bmap    seg uint8 [T, H, W] (non-zero = set) -> bmap uint8 [T, H, W] in {0, 1}: _seg2bmap (:582-638) per frame. */
int tt_davis_jf_counts(const void* pred, int pred_dtype, const void* gt, int gt_dtype, const uint8_t* void_mask, long long* counts, int T,
                       int H, int W, int O, const int* spans, int el_rows, int el_cols, int anchor_y, int anchor_x, tt_stream_t stream);
int tt_davis_seg2bmap(const uint8_t* seg, uint8_t* bmap, int T, int H, int W, tt_stream_t stream);

/* ---- N8: the boundary F1 score of bfscore.py:21-165 (calc_precision_recall / bfscore / evaluate_bf_score) as
 *      integer counts; the host forms precision, recall and F1 with the reference's fp64 expressions and branches.
 *   tt_bf_counts   gt, pr: binary maps uint8 [P, H, W] (any non-zero value is set), P (image, class) pairs.  counts: int64 [P, 4] =
 *                  {n_pr, hit_pr, n_gt, hit_gt}.  n = the number of contour points of the map as cv2.findContours(RETR_LIST,
 *                  CHAIN_APPROX_NONE) lists them over all its borders, with multiplicity (zero-padded image, 8-connected
 *                  foreground): the sum over the set pixels of m(p), a table of the 8 neighbour bits (0 inside, 1 for an isolated
 *                  pixel, up to 4).  hit = the same sum over the pixels p that have a pixel q of the OTHER map with m(q) > 0 and
 *                  (q - p) in the element: calc_precision_recall's hits (d < t^2).  The element is centred and symmetric, passed from
 *                  the HOST as spans (int [el_rows][2] = first, last set column of each row, columns 0..el_rows - 1 with the centre
 *                  at el_rows / 2; first > last: an empty row); el_rows = 2 r + 1 <= 127 (t <= 64), anything else returns
 *                  TT_EINVAL.  The call clears counts (hipMemsetAsync on `stream`), then adds per-tile sums with 64-bit integer
 *                  atomics: deterministic.  No workspace, no allocation, no synchronisation. */
int tt_bf_counts(const uint8_t* gt, const uint8_t* pr, long long* counts, int P, int H, int W, const int* spans, int el_rows,
                 tt_stream_t stream);

/* ---- Coarse entry points: whole reference functions as ONE call each.  They sequence the op-level entry
 *      points above on `stream` (same kernels, same results bit for bit as calling those one by one; they honour
 *      their `precision` argument / tt_vit_params.precision the way tt_linear_fwd does) and add nothing but the scratch layout.  Parameter tables are HOST
 *      arrays of DEVICE pointers, read during the call only.
 *
 *   tt_vit_forward       VisionTransformer.prepare_tokens + blocks + norm (dino_vision_transformer.py:236-252,265-273; Block
 *                        :135-153, Attention :108-132, Mlp :89-105), i.e. FeatureExtractor.get_features' backbone pass
 *                        (models.py:965-969).  img [F_src, C, H, W] and frame_map (int32 [F], optional) as tt_patch_embed_fwd;
 *                        img == NULL: `tokens` already holds a residual stream [F, N, D] (an EMA teacher continuing from the
 *                        student's frozen blocks) and p->patch_* / cls / pos are not read.  Blocks p->blocks[0 .. n_blocks) run
 *                        in place on tokens [F, N, D], N = 1 + (H / patch)(W / patch).  normed (optional): the final LayerNorm of
 *                        the tokens, [F, N, D] or, with drop_cls != 0, [F, N - 1, D] (get_features drops the cls token).
 *                        last_qkv (optional, [F, N, 3 D]): the last block's qkv activations (what tt_foreground_mask reads);
 *                        last_probs (optional, [F, heads, N, N]): its attention probabilities (get_last_selfattention, :256-263).
 *   tt_mlp_head_forward  the projection head (models.py:915-926,1075-1077): Linear (GELU Linear)*, x [M, layers[0].in_features]
 *                        -> out [M, layers[n - 1].out_features].
 *   tt_scores_sinkhorn   TimeT.get_scores (time_tuning.py:195-217) for one rank: scores = normalize(z) @ prototypes^T for the
 *                        batch rows z [B, dim] and, when queue != NULL, the queue rows [queue_rows, dim] (:207-211), then the
 *                        Sinkhorn assignment over all B + queue_rows columns; q_out [rows_out, K] = the first rows_out rows.
 *                        scores [B + queue_rows, K] is an output too (batch_scores = its first B rows).  For world_size > 1 the
 *                        caller all-gathers `scores` and calls tt_sinkhorn on the gathered rows (the "gathered pointer" form).
 *   tt_adamw_ema_step    optimizer.step() + normalize_prototypes() + update_momentum_teacher() (time_tuning.py:659-663 ->
 *                        :413-429, :124-128, :109-122): AdamW over `tensors` (any count), prototypes [K, dim] renormalised in
 *                        place (skipped when NULL), then - when teacher_flat != NULL - teacher <- teacher (1 - m) + student m
 *                        over the flat parameter buffers and the teacher prototypes, which are renormalised too. */
typedef struct {
  const float *norm1_w, *norm1_b, *qkv_w, *qkv_b, *proj_w, *proj_b, *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
  const void *qkv_wp, *proj_wp, *fc1_wp, *fc2_wp;   /* planes > 0: the four weights as bf16 planes [planes][out][in] (tt_split_planes),
                                                       or, planes == 2, as fp16 pairs [out][2 in] (tt_split_pairs) */
} tt_vit_block_params;
typedef struct {
  const float *patch_w, *patch_b, *cls, *pos;   /* [D, C P P], [D], [D], [N, D] (position table at the input's grid) */
  const tt_vit_block_params* blocks;            /* host array, n_blocks entries */
  int n_blocks;
  const float *norm_w, *norm_b;                 /* final LayerNorm (may be NULL when normed == NULL) */
  int dim, heads, hidden, patch;                /* D, attention heads (head_dim = D / heads), MLP width, patch size */
  int planes;                                   /* 0: fp32 operands (tt_linear_fwd); 1 / 3: the bf16-plane path of the blocks
                                                   (tt_linear_fwd_planes; 1 = BASELINE C4's bf16 path, 3 = fp32-accurate), D % 64 == 0;
                                                   2: fp16 PAIRS (tt_linear_fwd_pairs, the fp32-accurate "f16x3" mode; *_wp are
                                                   tt_split_pairs of the weights), D % 64 == 0 and hidden % 64 == 0 */
  const void* patch_wp;                         /* optional.  planes == 1: patch_w as one bf16 plane [D, C P P] - prepare_tokens then runs
                                                   tt_patch_embed_fwd_planes where its shape rules hold (ABI 4); planes == 2: patch_w in
                                                   pairs [D][2 C P P] - tt_patch_embed_fwd_pairs where ITS rules hold and C P P <= 3 D
                                                   (the rows then fit the scratch) (ABI 6) */
  int* range_flag;                              /* planes == 2: the pair producers' range flag (device int or NULL; ABI 7) */
  int precision;                                /* planes == 0: the `precision` of the blocks' tt_linear_fwd products (TT_PRECISION_*; ABI 8) */
} tt_vit_params;
typedef struct {
  const float* w;   /* [out_features, in_features] */
  const float* b;   /* [out_features] or NULL */
  int out_features, in_features;
} tt_linear_params;
size_t tt_vit_forward_workspace_bytes(int F, int N, int D, int hidden, int planes);
int tt_vit_forward(const tt_vit_params* p, const float* img, const int32_t* frame_map, int F, int C, int H, int W, float* tokens,
                   float* normed, int drop_cls, float* last_qkv, float* last_probs, void* workspace, size_t workspace_bytes,
                   tt_stream_t stream);
size_t tt_mlp_head_forward_workspace_bytes(int M, const tt_linear_params* layers, int n_layers);
int tt_mlp_head_forward(const float* x, int M, const tt_linear_params* layers, int n_layers, float* out, int precision, void* workspace,
                        size_t workspace_bytes, tt_stream_t stream);
size_t tt_scores_sinkhorn_workspace_bytes(int B, int queue_rows, int K, int dim);
int tt_scores_sinkhorn(const float* z, int B, const float* queue, int queue_rows, const float* prototypes, int K, int dim,
                       float* scores, float* q_out, int rows_out, float eps, int iters, int precision, void* workspace,
                       size_t workspace_bytes, tt_stream_t stream);
int tt_adamw_ema_step(const tt_adamw_tensor* tensors, int count, int step, float beta1, float beta2, float eps, float* prototypes,
                      int K, int dim, float* teacher_flat, const float* student_flat, long long n_flat, float* teacher_prototypes,
                      double momentum, tt_stream_t stream);

/* features * mask[..., None] (models.py:142) and its backward: x[r][:] *= row_scale[r], cols % 4 == 0, x 16-byte aligned. */
int tt_scale_rows_inplace(float* x, const float* row_scale, int rows, int cols, tt_stream_t stream);

/* ---- N21: JPEG frames decoded on the device - what Image.open does inside the reference's DataLoader workers (data_loader.py:595-614),
   bit-equal to Pillow's decode (libjpeg-turbo defaults: accurate integer IDCT, triangle-filter chroma up-sampling, 16-bit colour tables).
   The HOST half (jpeg_scan.cpp: no HIP, no state, no allocation, re-entrant; every read checked against `len`) parses the markers and
   undoes the Huffman coding; the DEVICE half (jpeg.hip) dequantises, runs the IDCT, up-samples and colour-converts a whole batch in two
   launches.
   Supported: SOF0 / 8-bit SOF1, three components, luma 1x1 / 2x1 / 2x2 over chroma 1x1, DRI / RSTn, one interleaved scan, YCbCr.
   Status of both host entries: TT_JPEG_OK; > 0 a well-formed file this decoder does not take (the caller falls back); < 0 a broken file
   or a bad argument. */
#define TT_JPEG_OK 0
#define TT_JPEG_UNSUPPORTED_FRAME 1        /* progressive, lossless, hierarchical, a DNL height */
#define TT_JPEG_UNSUPPORTED_ARITHMETIC 2
#define TT_JPEG_UNSUPPORTED_COMPONENTS 3   /* grayscale, CMYK */
#define TT_JPEG_UNSUPPORTED_PRECISION 4    /* 12-bit samples */
#define TT_JPEG_UNSUPPORTED_SAMPLING 5
#define TT_JPEG_UNSUPPORTED_SCANS 6        /* more than one scan */
#define TT_JPEG_UNSUPPORTED_QTABLE 7       /* 16-bit quantisation tables */
#define TT_JPEG_UNSUPPORTED_COLOUR 8       /* RGB stored without a transform */
#define TT_JPEG_EMALFORMED (-1)            /* markers / segment lengths / tables */
#define TT_JPEG_ETRUNCATED (-2)            /* the scan data ends early */
#define TT_JPEG_EHUFFMAN (-3)              /* a code no table holds */
#define TT_JPEG_ERUN (-4)                  /* a run past coefficient 63 */
#define TT_JPEG_ERESTART (-5)              /* a missing or misnumbered RSTn */
#define TT_JPEG_EARGUMENT (-6)             /* null pointer, coefficient buffer too small */
#define TT_JPEG_444 0                      /* sampling codes: luma 1x1, */
#define TT_JPEG_422 1                      /* 2x1, */
#define TT_JPEG_420 2                      /* 2x2 */
/* Per component the block grid is (ceil(H / (8 vmax)) v) x (ceil(W / (8 hmax)) h) blocks; n_coeffs = 64 x the three grids' blocks. */
int tt_jpeg_probe(const uint8_t* data, size_t len, int* H, int* W, int* sampling, long long* n_coeffs);
/* coeffs: int16, 64 per block in natural (row-major) order, component after component, each in block-grid raster order; all n_coeffs are
   written (zeros included).  qtables: uint16 [3][64], natural order, the table OF component 0, 1, 2.  On a non-zero status the buffers'
   contents are unspecified, but nothing outside them is touched. */
int tt_jpeg_scan(const uint8_t* data, size_t len, int16_t* coeffs, long long coeffs_capacity, uint16_t* qtables);
/* One row per frame.  Offsets: coeff_off in int16 elements into `coeffs` (multiples of 8), qslot in 64-entry tables into `qtables`,
   plane_off in bytes into the workspace (multiples of 8; component c's plane is its block grid x 64 bytes), out_off in bytes into `out`
   (the frame's uint8 [H, W, 3]). */
typedef struct {
  int64_t H, W, sampling;
  int64_t coeff_off[3], qslot[3], plane_off[3];
  int64_t out_off;
  int64_t reserved[3];
} tt_jpeg_frame;
/* The workspace the table's plane offsets need (0: a row is not a frame).  Pure host function. */
size_t tt_jpeg_decode_batch_workspace_bytes(const tt_jpeg_frame* frame_table, int n_frames);
/* Decodes n_frames frames, which may differ in size and sampling, in two launches.  frame_table is the HOST copy of the table and is
   checked in full - every offset and extent against n_coeffs, n_qtables, out_bytes and workspace_bytes - before anything is launched
   (TT_EINVAL, no launch); frame_table_dev is the same table in device memory, which the kernels read and trust.  coeffs and qtables are
   device pointers, 16-byte aligned.  Allocates nothing. */
int tt_jpeg_decode_batch(const int16_t* coeffs, long long n_coeffs, const uint16_t* qtables, int n_qtables, const tt_jpeg_frame* frame_table,
                         const tt_jpeg_frame* frame_table_dev, int n_frames, uint8_t* out, long long out_bytes, void* workspace,
                         size_t workspace_bytes, tt_stream_t stream);

/* ---- N24: the Huffman streams decoded on the device.  tt_jpeg_prepare (host, jpeg_scan.cpp: no state, no allocation, every read and
   write checked) copies a file's scan once without decoding it - stuffing and fill bytes dropped, cut at the RSTn markers, every restart
   segment on a 4-byte boundary - behind the DHT bytes of its six tables; tt_jpeg_entropy_batch (jpeg_entropy.hip) turns the streams of
   a batch into the SAME int16 coefficients tt_jpeg_scan writes, which tt_jpeg_decode_batch reads where they lie.  The scheme, its
   bounds and the status rules: csrc/jpeg_huff.hpp, DESIGN.md N24.
   One row per frame.  scan_off / huff_off: bytes into `scan` (multiples of 4) of the frame's clean stream (scan_len bytes) and of its
   tables (6 x 272 bytes: 16 counts + 256 values of the DC, AC table of component 0, 1, 2).  Rows seg_off ... seg_off + n_segments - 1 of
   the segment table (uint32 [n][2]) hold each segment's start in bytes from scan_off (a multiple of 4) and its length in bits.
   restart: MCUs per segment, 0 = no DRI.  coeff_off: as in tt_jpeg_frame. */
typedef struct {
  int64_t H, W, sampling, restart;
  int64_t scan_off, scan_len, huff_off;
  int64_t seg_off, n_segments;
  int64_t coeff_off[3];
  int64_t reserved[4];
} tt_jpeg_stream;
/* The capacities tt_jpeg_prepare needs for a file of `len` bytes, from len alone: bytes of `scan`, rows of `segs`. */
int tt_jpeg_prepare_bytes(size_t len, size_t* scan_bytes, size_t* n_segments);
/* Status as tt_jpeg_scan's (a missing or misnumbered RSTn: TT_JPEG_ERESTART; a capacity too small: TT_JPEG_EARGUMENT).  Writes the
   tables at scan[0], the stream behind them, the segment rows from segs[0], the row with offsets RELATIVE to these two (huff_off 0,
   scan_off 1632, seg_off 0, coeff_off from 0: the caller adds where it put them) and qtables as tt_jpeg_scan does. */
int tt_jpeg_prepare(const uint8_t* data, size_t len, uint8_t* scan, size_t scan_capacity, uint32_t* segs, size_t seg_capacity,
                    tt_jpeg_stream* row, uint16_t* qtables);
/* Bytes of workspace of a batch (per frame four int32 of statistics: rounds, tiles, subsequences, the first failing subsequence or -1);
   0: bad arguments.  Pure host function. */
size_t tt_jpeg_entropy_batch_workspace_bytes(const tt_jpeg_stream* stream_table, int n_frames, int subseq_bits);
/* One workgroup per frame, one launch behind a memset of `coeffs` (all n_coeffs).  The HOST copies of the segment table and the stream
   table are checked in full against scan_bytes, n_segs, n_coeffs and workspace_bytes before anything is launched (TT_EINVAL, no launch,
   nothing written); the kernel reads the device copies.  subseq_bits: a multiple of 32 in [128, 4096].  status: device int32 [n_frames],
   0 or the TT_JPEG_E* code of the frame's first error; a failed frame's coefficients are unspecified, the others' are not affected.
   scan 4-byte, coeffs 16-byte aligned.  Allocates nothing, synchronises nothing. */
int tt_jpeg_entropy_batch(const uint8_t* scan, long long scan_bytes, const uint32_t* segs_host, const uint32_t* segs_dev, long long n_segs,
                          const tt_jpeg_stream* stream_table_host, const tt_jpeg_stream* stream_table_dev, int n_frames, int subseq_bits,
                          int16_t* coeffs, long long n_coeffs, int32_t* status, void* workspace, size_t workspace_bytes, tt_stream_t stream);
/* The same arguments as host pointers (the *_dev ones and `stream` are not looked at): the emulation of the kernel, lane by lane through
   the same header, bit-equal to it in coefficients, status and statistics.  No GPU call. */
int tt_jpeg_entropy_host(const uint8_t* scan, long long scan_bytes, const uint32_t* segs_host, const uint32_t* segs_dev, long long n_segs,
                         const tt_jpeg_stream* stream_table_host, const tt_jpeg_stream* stream_table_dev, int n_frames, int subseq_bits,
                         int16_t* coeffs, long long n_coeffs, int32_t* status, void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* ---- N22: ragged image kernels - the pixel work of the Pascal VOC reader (leoloader.py:241-264: Resize((S, S)) + ToTensor + Normalize of
   the image, Resize((R, R), NEAREST) + ToTensor of the palette PNG) for a batch whose items DIFFER in size, one launch per batch; bit-equal
   to Pillow like the tt_img_* entries above, whose arithmetic they share.
   One row per item.  src_off: byte offset of the item's image in `in` - uint8 [H, W, 3] for the resize, [H, W] for the gather; ANY byte
   value (a decoder's out_off, a packed buffer), no source read is wider than a byte.  (x0, y0, w, h): the crop box, inside the image.
   flip: 0 / 1, the output row is written mirrored.  The *_off fields are offsets in int32 elements into one `pool`: hk_off / hb_off the
   horizontal taps int32 [OW, hksize] and bounds int32 [OW, 2] (first column RELATIVE TO THE BOX and tap count, what
   timetuning_amd.video_transformations.resample_coeffs(w, OW) builds), vk_off / vb_off / vksize the vertical ones for (h, OH); ytab_off /
   xtab_off the gather's int32 [OH] / [OW] tables of ABSOLUTE source rows / columns (video_transformations.nearest_table with the crop offset
   and the flip folded in; the gather does not look at the box beyond checking it, nor at flip).  Output item i is row i of the output. */
typedef struct {
  int64_t src_off, H, W;
  int64_t x0, y0, w, h;
  int64_t flip;
  int64_t hk_off, hb_off, hksize;
  int64_t vk_off, vb_off, vksize;
  int64_t ytab_off, xtab_off;
} tt_img_ragged_item;
#define TT_IMG_RAGGED_BAND 16             /* output rows a workgroup of tt_img_resize_ragged owns */
#define TT_IMG_RAGGED_LDS_BUDGET 65536    /* bytes of LDS per workgroup: two workgroups fit the 160 KiB of a CU */
/* tt_img_resize_ragged   out[i] = crop(box_i).resize((OW, OH), BILINEAR) by Resample.c: 22-bit taps, uint8 rounding after the horizontal
                          pass and again after the vertical pass; a pass with w == OW (h == OH) is the identity and its pool fields are not
                          read.  Exactly one output: out_u8 [n, OH, OW, 3], or out_f32 [n, 3, OH, OW] = ((float)v / 255 - mean[c]) / std[c]
                          with the arithmetic of tt_img_resample_v (mean3 / std3 HOST pointers to 3 floats).  A workgroup owns one item and
                          a band of TT_IMG_RAGGED_BAND output rows; it runs the horizontal pass for the box rows min(bounds.ymin) ..
                          max(bounds.ymin + cnt) of its band into LDS as uint8 [rows, OW, 3] and the vertical pass from there: the
                          intermediate never reaches device memory.
   tt_img_resize_ragged_lds_bytes   the largest band of an (h, w) box resized to (OH, OW) with Pillow's bounds, in bytes of LDS (0: a size
                          outside 1 .. 32767); tt_img_resize_ragged_shape_ok: 1 when every size is inside 1 .. 32767 and that figure is within
                          TT_IMG_RAGGED_LDS_BUDGET.  Pure host functions over one item's sizes, like tt_kmeans_fit_shape_ok.  Strong
                          down-scaling of a wide image is what falls outside; the caller takes such an item through tt_img_resample_h / _v.
   tt_img_gather_nearest_ragged   out[i, y, x] = in_i[ytab_i[y], xtab_i[x]] on label maps: out_u8 [n, OH, OW], or out_f32 [n, 1, OH, OW] =
                          (float)v / 255 as one IEEE fp32 division (the C = 1 rule of tt_img_gather_nearest).
   `items` and `pool` are the HOST copies and are checked in full before anything is launched - 1 <= n_items <= 65535, sizes and outputs in
   1 .. 32767, every image inside in_bytes, every box inside its image, flip 0 / 1, every used pool range inside pool_len, every
   bounds[...] >= 0 with cnt <= ksize and bounds + cnt inside the box's line, the LDS need of every band (from the vertical bounds handed
   in) within the budget, every table entry inside its image: TT_EINVAL with a message naming the item, nothing launched.  items_dev /
   pool_dev are the same data in device memory, which the kernels read and trust.  Both calls are one launch and allocate nothing. */
size_t tt_img_resize_ragged_lds_bytes(int h, int w, int OH, int OW);
int tt_img_resize_ragged_shape_ok(int h, int w, int OH, int OW);
int tt_img_resize_ragged(const uint8_t* in, long long in_bytes, const tt_img_ragged_item* items, const tt_img_ragged_item* items_dev,
                         int n_items, const int32_t* pool, const int32_t* pool_dev, long long pool_len, uint8_t* out_u8, float* out_f32,
                         int OH, int OW, const float* mean3, const float* std3, tt_stream_t stream);
int tt_img_gather_nearest_ragged(const uint8_t* in, long long in_bytes, const tt_img_ragged_item* items, const tt_img_ragged_item* items_dev,
                                 int n_items, const int32_t* pool, const int32_t* pool_dev, long long pool_len, uint8_t* out_u8,
                                 float* out_f32, int OH, int OW, tt_stream_t stream);

/* ---- N23: label maps as byte streams (csrc/label_map.hip) - which label values occur in a segment, and the YouTube-VOS remap of per-video
   instance ids to dataset-wide category ids built on it (data_loader.py:453-464 make_categories_dict, :497-506 map_instances, :774-796
   YVOSDataset; the per-frame torch.unique of clustering.py:95-103).  Segment s is elements s P ... s P + P - 1 of `labels`; neither P nor
   the base pointer needs any alignment beyond the element's own.  No workgroup waits on another; nothing is allocated.
   tt_label_presence_segments   labels: uint8 (elem_bytes 1) or int64 (elem_bytes 8).  words uint32 [S][8]: bit (v & 31) of word v >> 5 is
                          set iff value v in 0 .. 255 occurs in segment s.  status int32 [S]: 1 where an int64 value lies outside 0 .. 255
                          (it sets no bit; the caller then counts that segment some other way), else 0.  The entry zeroes words and status
                          on the stream; one launch.
   tt_map_instances       labels_out[e] = lut_s[labels_in[e]] on uint8 [S][P], two launches: the presence pass into words_ws
                          (tt_map_instances_workspace_bytes(S) = 32 S bytes, 4-byte aligned), then the apply pass, whose workgroups each
                          compose lut_s in LDS.  cat int32 [S][256]: the category of object id v of segment s's video, -1 = not in the meta
                          file.  sequential = 1 reproduces the reference's in-place loop `frame[frame == obj] = category` over the ascending
                          torch.unique of the clip: from the identity, for obj = 1 .. 255 in order, if obj occurs in the ORIGINAL segment
                          every entry whose CURRENT value equals obj becomes cat[obj] - a pixel mapped onto a later, present object id is
                          mapped again (the reference's chaining, kept as a quirk).  sequential = 0: v -> cat[v] for present v >= 1.  Value 0
                          is never remapped.  A present object whose cat is outside 0 .. 255 makes status[s] the smallest such id and
                          lut_s the identity (the segment is copied unmapped); else status[s] = 0.  lut_out uint8 [S][256] receives lut_s.
                          The ranges of labels_in and labels_out must not overlap (workgroups of one segment read all of it for the
                          presence pass while others would write): TT_EINVAL.
   Refusals (null pointers, S or P < 1, another elem_bytes / sequential, overlap, a short or misaligned workspace) return TT_EINVAL with the
   numbers in tt_last_error, and nothing is launched. */
int tt_label_presence_segments(const void* labels, int elem_bytes, int S, long long P, uint32_t* words, int32_t* status, tt_stream_t stream);
size_t tt_map_instances_workspace_bytes(int S);
int tt_map_instances(const uint8_t* labels_in, uint8_t* labels_out, const int32_t* cat, int S, long long P, int sequential, uint8_t* lut_out,
                     int32_t* status, void* words_ws, size_t words_ws_bytes, tt_stream_t stream);

/* ---- N26: annotation PNGs decoded on the device - what Image.open does for the label maps in the reference's readers
   (data_loader.py:595-614 read_clips, leoloader.py:220-235 VOCDataset.__getitem__), bit-equal to np.asarray(Image.open(...)).
   The HOST half (png_scan.cpp: no HIP, no state, no allocation, re-entrant; every read checked against `len`, every write against the
   caller's capacity) walks the chunks, checks the CRC-32 of the critical ones and concatenates the IDAT payloads; the DEVICE half
   (png_decode.hip) inflates, checks the Adler-32, undoes the row filters and unpacks, one wave per file.  The scheme, its bounds and the
   status rules: csrc/png_inflate.hpp, DESIGN.md N26.
   Supported: non-interlaced palette maps at depth 1 / 2 / 4 / 8 (the output is the index) and gray maps at depth 8.
   Status: TT_PNG_OK; > 0 a well-formed file this decoder does not take (the caller falls back); < 0 a broken file or a bad argument. */
#define TT_PNG_OK 0
#define TT_PNG_UNSUPPORTED_INTERLACE 1     /* Adam7 */
#define TT_PNG_UNSUPPORTED_COLOUR 2        /* a colour type other than 3 (palette) or 0 (gray) */
#define TT_PNG_UNSUPPORTED_GRAY_DEPTH 3    /* gray below 8 bits: Pillow rescales those */
#define TT_PNG_UNSUPPORTED_16BIT 4
#define TT_PNG_UNSUPPORTED_SIZE 5          /* a side above 32767: more than the kernels that read the maps take */
#define TT_PNG_EMALFORMED (-1)             /* signature, IHDR, chunk order, zlib header; stored-block length check, reserved block type */
#define TT_PNG_ETRUNCATED (-2)             /* a chunk past the end of the file; the stream or the output ends early */
#define TT_PNG_EHUFFMAN (-3)               /* a refused code-length set or a code no table holds */
#define TT_PNG_EDISTANCE (-4)              /* a back-reference before the first byte */
#define TT_PNG_EOVERRUN (-5)               /* more than H (1 + row_bytes) inflated bytes */
#define TT_PNG_ECHECKSUM (-6)              /* CRC-32 of a critical chunk (host), Adler-32 of the inflated bytes (device) */
#define TT_PNG_EFILTER (-7)                /* a filter byte above 4 */
#define TT_PNG_EARGUMENT (-8)              /* null pointer, capacity too small, a table row that is no file */
int tt_png_probe(const uint8_t* data, size_t len, int* H, int* W, int* bit_depth, int* color_type);
/* One row per file.  row_bytes = ceil(W depth / 8).  stream_off: bytes into `streams` (a multiple of 4) of the file's deflate stream from
   its first block on, stream_len bytes, the Adler-32 trailer included.  out_off: bytes into `out` of the file's uint8 [H, W] map.  ws_off:
   bytes into the workspace of the file's H (1 + row_bytes) inflated bytes. */
typedef struct {
  int64_t H, W, depth, color_type, row_bytes;
  int64_t stream_off, stream_len;
  int64_t out_off, ws_off;
  int64_t reserved[7];
} tt_png_stream;
/* The capacity tt_png_prepare needs for a file of `len` bytes, from len alone. */
int tt_png_prepare_bytes(size_t len, size_t* stream_bytes);
/* Status as tt_png_probe's (a wrong CRC-32 in IHDR / PLTE / IDAT / IEND: TT_PNG_ECHECKSUM; a capacity too small: TT_PNG_EARGUMENT).  Writes
   the stream behind its two-byte zlib header (checked: method 8, window <= 32 KB, check bits, no preset dictionary) at stream[0], zero-padded
   to 4 bytes, and the row with stream_off, out_off and ws_off 0: the caller sets where it put them. */
int tt_png_prepare(const uint8_t* data, size_t len, uint8_t* stream, size_t stream_capacity, tt_png_stream* row);
/* Bytes of workspace of a batch: the slices the table's ws_off place, rounded to 16, then per file eight int32 of statistics (block kinds
   seen as a bit mask, longest literal/length and distance code used, smallest and largest distance, longest match, filters seen as a bit
   mask, inflated bytes); 0: a row is not a file.  Pure host function. */
size_t tt_png_decode_batch_workspace_bytes(const tt_png_stream* table, int n_files);
/* One wave per file, one launch.  table_host is checked in full against stream_bytes, out_bytes and workspace_bytes - offsets, extents,
   4-byte stream alignment, overlapping outputs or slices - before anything is launched (TT_EINVAL, no launch, nothing written); the kernel
   reads table_dev.  status: device int32 [n_files], 0 or the TT_PNG_E* code of the file's first error; a failed file's pixels are
   unspecified inside its own slice, the others' are not affected.  streams and workspace 4-byte aligned.  Allocates nothing, synchronises
   nothing. */
int tt_png_decode_batch(const uint8_t* streams, long long stream_bytes, const tt_png_stream* table_host, const tt_png_stream* table_dev,
                        int n_files, uint8_t* out, long long out_bytes, void* workspace, size_t workspace_bytes, int32_t* status_dev,
                        tt_stream_t stream);
/* The same arguments as host pointers (table_dev and `stream` are not looked at): the sequential loop over the same csrc/png_inflate.hpp
   steps, with the same status codes and statistics.  No GPU call. */
int tt_png_decode_host(const uint8_t* streams, long long stream_bytes, const tt_png_stream* table_host, const tt_png_stream* table_dev,
                       int n_files, uint8_t* out, long long out_bytes, void* workspace, size_t workspace_bytes, int32_t* status,
                       tt_stream_t stream);
/* The same again with the kernel's 64 lanes: 64 host threads run the shared inflate side by side behind a barrier, so that the pending
   literals, the lane-strided copies, the table fill and the Adler partial sums run on the CPU as on the device (lane 0 then runs the
   sequential unfilter).  Same status codes and statistics.  A testing aid for the no-GPU tests and the sanitizer program: it starts
   threads, and a barrier per match makes it slow on large files. */
int tt_png_decode_host_wave(const uint8_t* streams, long long stream_bytes, const tt_png_stream* table_host, const tt_png_stream* table_dev,
                            int n_files, uint8_t* out, long long out_bytes, void* workspace, size_t workspace_bytes, int32_t* status,
                            tt_stream_t stream);

/* ---- N29: label maps written as palette PNGs, deflated on the device - what the reference's my_utils.imwrite_indexed ("Save indexed
   png for DAVIS", my_utils.py:72-79: Image.fromarray + putpalette + save) does for one map, for a batch of maps that never leave the
   device as pixels.  The DEVICE half (png_encode.hip) filters every row with Up and deflates every band of rows ("chunk") of every map
   in a workgroup of its own into one fixed-Huffman block closed by an empty stored block, so that a file's stream is the plain
   concatenation of its chunks; a scan and a gather make ONE compact buffer of all streams.  The HOST half (png_scan.cpp) wraps a stream
   into a file: signature, IHDR, PLTE, ONE IDAT, IEND.  The byte format, its bounds and the table rules: csrc/png_deflate.hpp, DESIGN.md
   N29.  Pixel-equal to Pillow's file, not byte-equal: runs at distance 1 in the fixed code only, about four times Pillow's size.
   8-bit maps uint8 [H, W], 1 <= H, W <= 32767.  Every refusal is TT_PNG_EARGUMENT. */
/* One row per map.  data: the map's first byte (device memory for tt_png_encode_batch, host memory for tt_png_encode_host), rows
   `pitch` >= W bytes apart.  first_chunk, n_chunks: its rows of the chunk table.  out_off: bytes into the slots of the workspace of its
   first chunk's slot, which is also where its stream would begin in the output were every chunk at its capacity. */
typedef struct {
  const uint8_t* data;
  int64_t H, W, pitch;
  int64_t first_chunk, n_chunks, out_off;
  int64_t reserved;
} tt_png_map;
/* One row per chunk: rows row0 .. row0 + rows - 1 of map `map`, deflated into the slot at slot_off of the workspace. */
typedef struct {
  int64_t map, row0, rows, slot_off;
} tt_png_chunk;
/* One row per map, written by the device: where its stream lies in the output, its length, and the Adler-32 of its filtered bytes. */
typedef struct {
  int64_t offset, length, adler;
  int64_t reserved;
} tt_png_result;
/* Builds the tables from data, H, W and pitch of every map: fills first_chunk, n_chunks and out_off, and - with `chunks`, of
   chunk_capacity rows - the chunk table.  *n_chunks: the rows of the chunk table; *out_capacity: the bytes the output must hold (every
   chunk at its capacity of (9 n + 7) / 8 + 7 bytes for n filtered bytes, rounded up to 4).  Call it without `chunks` for the counts.
   Pure host function. */
int tt_png_encode_plan(tt_png_map* maps, int n_maps, tt_png_chunk* chunks, long long chunk_capacity, long long* n_chunks, long long* out_capacity);
/* Bytes of workspace of a batch: one slot per chunk, then four int32 per chunk (stream bytes, Adler a, b, filtered bytes), then the
   chunks' offsets in the output; 0: a row is not a map.  Pure host function. */
size_t tt_png_encode_batch_workspace_bytes(const tt_png_map* maps, int n_maps);
/* Three launches: one workgroup per chunk (filter, runs, bits), one workgroup for the scan of the chunk lengths and the files' Adler-32,
   one workgroup per chunk for the gather.  The HOST tables are checked in full against the plan, out_bytes and workspace_bytes before
   anything is launched (TT_PNG_EARGUMENT, no launch, nothing written); the kernels read maps_dev and chunks_dev.  out: device bytes, the
   streams one behind the other in map order (no zlib header, no Adler-32 trailer); results_dev: device tt_png_result [n_maps].  The
   workspace need not be cleared between calls.  workspace 16-byte, tables and results 8-byte aligned.  No workgroup waits for another;
   allocates nothing, synchronises nothing. */
int tt_png_encode_batch(const tt_png_map* maps_host, const tt_png_map* maps_dev, int n_maps, const tt_png_chunk* chunks_host,
                        const tt_png_chunk* chunks_dev, long long n_chunks, uint8_t* out, long long out_bytes, tt_png_result* results_dev,
                        void* workspace, size_t workspace_bytes, tt_stream_t stream);
/* The same arguments as host pointers (maps_dev, chunks_dev and `stream` are not looked at): the sequential loop over the same
   csrc/png_deflate.hpp steps, bit-equal to the kernels.  No GPU call. */
int tt_png_encode_host(const tt_png_map* maps_host, const tt_png_map* maps_dev, int n_maps, const tt_png_chunk* chunks_host,
                       const tt_png_chunk* chunks_dev, long long n_chunks, uint8_t* out, long long out_bytes, tt_png_result* results,
                       void* workspace, size_t workspace_bytes, tt_stream_t stream);
/* Bytes of the file around a stream of stream_len bytes with a palette of palette_entries colours (0: a gray file). */
size_t tt_png_file_bytes(size_t stream_len, int palette_entries);
/* The finished file around a device-made stream: signature, IHDR (W, H, depth 8, colour type 3 with a palette, 0 without), PLTE
   (palette: 3 palette_entries bytes, 1..256 entries, or null and 0), ONE IDAT (78 01, the stream, `adler` big-endian), IEND, each with
   its CRC-32.  TT_PNG_EARGUMENT: a null pointer, a side outside 1..32767, more than 256 entries, out_capacity below tt_png_file_bytes. */
int tt_png_write_file(const uint8_t* stream, size_t stream_len, uint32_t adler, int H, int W, const uint8_t* palette, int palette_entries,
                      uint8_t* out, size_t out_capacity, size_t* out_len);

/* ---- N31: dense nearest-neighbour retrieval (csrc/nn_retrieval.hip; timetuning_amd/nn_retrieval.py) - the evaluation of
   Balazevic et al., 2023: every patch of a validation image retrieves its k nearest patches of a labelled memory bank by cosine similarity
   and takes the softmax-weighted mean of their label distributions.  The similarities are tt_linear_fwd's, one block of the bank at a
   time; these entries are the exact search step, the bank's label distributions and the weighted gather.  None of them allocates,
   synchronises or frees; every refusal is TT_EINVAL with nothing launched and nothing written.
   tt_topk_merge       sims fp32 [Q, Nc] with rows ld >= Nc floats apart: the similarities of Q queries to bank rows base .. base + Nc - 1.
                       vals fp32 [Q, k], idx int64 [Q, k]: per query the k best seen so far, REPLACED by the k best of (list U block).
                       The order is total: the larger similarity first, among equal similarities the smaller bank index first.  An
                       empty list is k times (-inf, -1): init = 1 starts from it without reading vals / idx, init = 0 merges into them.
                       A NaN is never selected, and neither is a -inf (it ties with the empty entry, whose index -1 is the smaller):
                       the tail of a list that has seen fewer than k finite similarities stays (-inf, -1).  Lists are always sorted, so
                       vals[q][k - 1] is the query's threshold.  The result is a function of the multiset of (similarity, index)
                       offered so far: not of the cut into blocks, of their order or of the launch geometry.  Bank indices offered to
                       one list must be distinct.  sims may start at any 4-byte address.  1 <= k <= tt_topk_merge_max_k() = 64;
                       1 <= Q, Nc <= 2^31 - 1; ld <= 2^40; 0 <= base, base + Nc <= 2^62.  One wave per query, no LDS, no atomics.
   tt_patch_label_counts   maps uint8 [M, R, R], a grid of g x g cells of (R / g)^2 pixels (R % g == 0): counts int32 [M, g g, C] the pixels
                       of every class in every cell, valid int32 [M, g g] their sum.  A pixel equal to `ignore` (0 .. 255, or -1 for none)
                       is counted nowhere.  A label >= C that is not `ignore` is counted nowhere either and lowers *status (device
                       uint32, set to 0xffffffff by the call) to the index of its map: after the call *status is the FIRST such map, or
                       0xffffffff.  C <= 256, R <= 16384, M g g <= 2^23.  Integer LDS atomics: exact and independent of order.  maps
                       may start at any address.
   tt_nn_label_aggregate   vals fp32 [Q, k], idx int64 [Q, k] (tt_topk_merge's), labels fp32 [N, C], beta > 0:
                       out[q][c] = sum_j w_j labels[idx_j][c] with w = softmax(vals / beta) over the entries whose idx is a bank row
                       (0 <= idx < N; the others are left out and never read).  The maximum is subtracted, j runs 0 .. k - 1 in order,
                       fp32 throughout, no atomics; a query without a valid entry gets a zero row.  1 <= k <= 64, C <= 2^20. */
int tt_topk_merge_max_k(void);
int tt_topk_merge_shape_ok(long long Q, long long Nc, long long ld, int k);
int tt_topk_merge(const float* sims, long long Q, long long Nc, long long ld, long long base, float* vals, int64_t* idx, int k, int init,
                  tt_stream_t stream);
int tt_patch_label_counts_shape_ok(int M, int R, int g, int C);
int tt_patch_label_counts(const uint8_t* maps, int M, int R, int g, int C, int ignore, int32_t* counts, int32_t* valid, uint32_t* status,
                          tt_stream_t stream);
int tt_nn_label_aggregate_shape_ok(long long Q, int k, long long N, int C);
int tt_nn_label_aggregate(const float* vals, const int64_t* idx, const float* labels, long long Q, int k, long long N, int C, float beta,
                          float* out, tt_stream_t stream);

/* ---- N32: FCN-head fine-tuning (csrc/conv_tokens.hip; timetuning_amd/leopart.py, timetuning_amd/fcn_finetune.py) - the
   FCNHead of leopart.py:83-147 (num_convs 3x3 conv + ReLU layers, an optional conv_cat over cat([x, convs(x)]), Dropout2d, a 1x1
   conv_seg) on frozen token features, forward and backward.  Tokens are [B, gh*gw, C] (NHWC); a convolution is an implicit GEMM in fp32
   on v_mfma_f32_32x32x2_f32 whose A operand is gathered from the neighbouring token rows, zeros off the grid.  None of these allocates,
   synchronises or frees; no float atomics, every sum in a fixed order (two calls give the same bits); every refusal is TT_EINVAL with
   tt_last_error() text, nothing launched and nothing written.  All tensor pointers except `weight`, `dw`, `db` and `dlogits` must be
   16-byte aligned.  Limits: channel counts % 4 == 0 and <= 1024 per source (so Ca + Cb <= 2048), 1 <= gh, gw <= 64, B gh gw < 2^31.
   The weight is nn.Conv2d's [Cout, Ca + Cb, 3, 3]; each call repacks it tap-major into its workspace (one launch).
   tt_conv3x3_tokens_fwd          y[b, (i, j), co] = act(bias[co] + sum over ci, di, dj of w[co, ci, 1 + di, 1 + dj] x[b, (i + di, j + dj), ci])
                                  * out_scale[b, co], zero padding.  x = channels of xa [B, gh gw, Ca] followed by those of xb
                                  [B, gh gw, Cb] (null with Cb = 0: one source).  act 0 = none, 1 = ReLU; bias [Cout] or null; out_scale
                                  [B, Cout] or null (Dropout2d as a multiplier).  2 launches.
   tt_conv3x3_tokens_bwd_data     dx [B, gh gw, c_count] = the gradient with respect to input channels c_begin .. c_begin + c_count - 1
                                  (c_count % 4 == 0, <= 1024) of dpre [B, gh gw, Cout], the gradient of the pre-activation: the
                                  transposed, flipped convolution.  gate [B gh gw, c_count] or null: dx is zero where gate <= 0 (the
                                  producing layer's ReLU, read from its saved output).  2 launches.
   tt_conv3x3_tokens_bwd_weight   dw [Cout, Ca + Cb, 3, 3] = sum over the rows of dpre[row][co] x[row shifted by the tap][ci], db [Cout]
                                  (or null) = the column sums of dpre, both times *scale_device if that is not null.  Rows are split
                                  over workgroups and folded in slice order (db: the fold of every bias gradient here).  2 launches.
   tt_fcn_head_grad               dpre [B gh gw, channels] = (dlogits [B gh gw, C] wseg [C, channels]) * out_scale[b, c] * [y > 0]: the
                                  gradient entering the last convolution from the gradient of the token-resolution logits; out_scale
                                  [B, channels] and y [B gh gw, channels] (that convolution's output) may be null.  C <= 256.  1 launch. */
size_t tt_conv3x3_tokens_fwd_workspace_bytes(int Ca, int Cb, int Cout);
int tt_conv3x3_tokens_fwd(const float* xa, const float* xb, const float* weight, const float* bias, const float* out_scale, float* y, int B,
                          int gh, int gw, int Ca, int Cb, int Cout, int act, void* workspace, size_t workspace_bytes, tt_stream_t stream);
size_t tt_conv3x3_tokens_bwd_data_workspace_bytes(int Cout, int c_count);
int tt_conv3x3_tokens_bwd_data(const float* dpre, const float* weight, const float* gate, float* dx, int B, int gh, int gw, int Cin, int Cout,
                               int c_begin, int c_count, void* workspace, size_t workspace_bytes, tt_stream_t stream);
size_t tt_conv3x3_tokens_bwd_weight_workspace_bytes(long long rows, int Cin, int Cout);
int tt_conv3x3_tokens_bwd_weight(const float* dpre, const float* xa, const float* xb, const float* scale_device, float* dw, float* db, int B,
                                 int gh, int gw, int Ca, int Cb, int Cout, void* workspace, size_t workspace_bytes, tt_stream_t stream);
int tt_fcn_head_grad(const float* dlogits, const float* wseg, const float* out_scale, const float* y, float* dpre, int B, int gh, int gw,
                     int C, int channels, tt_stream_t stream);

/* ---- N33: batch normalisation of the FCN head's ConvModules (csrc/bn_tokens.hip; timetuning_amd/leopart.py norm_cfg) -
   nn.BatchNorm2d over token-major tensors [rows = B gh gw, C] fp32, channel-contiguous (what the N32 convolutions read and write),
   forward and backward, fused with the ReLU and the Dropout2d multiplier that follow it in a ConvModule.  The rules of N32 hold: no
   allocation, synchronisation or free on a launch path; no float atomics; every column sum is taken in fp64 in a fixed order (per row
   slice: each thread's rows ascending, the 16 row lanes of the workgroup in lane order; then the slices in slice order, as two halves),
   so two calls give the same bits; every refusal is TT_EINVAL with tt_last_error() text, nothing launched and nothing written.
   Limits: C % 4 == 0, 0 < C <= 1024, 0 < rows < 2^31 (rows >= 2 when training), eps > 0, 0 <= momentum <= 1, act 0 or 1 (ReLU);
   z, y, g, dz, out_scale and the workspace 16-byte aligned.  The workspace holds the slice partials (fp64) and is needed by the
   training forward and by the backward.
   tt_bn_tokens_fwd   training = 1: mean[c], var[c] = the mean and the biased variance of column c of z (sums about the column's first row,
                      as tt_col_moments: a small variance beside a large mean survives), rstd = 1 / sqrt(var + eps),
                      y[r, c] = act((z[r, c] - mean[c]) * rstd[c] * gamma[c] + beta[c]) * out_scale[r / rows_per_image, c];
                      save_mean, save_rstd [C] are written for the backward; running_mean = (1 - m) running_mean + m mean and
                      running_var = (1 - m) running_var + m var rows / (rows - 1) (both may be null together: no running statistics).
                      out_scale [rows / rows_per_image, C] or null (then rows_per_image is not read).  2 launches: slice partials; then
                      a kernel whose workgroups fold the partials of their own 64 columns and apply.
                      training = 0: mean = running_mean, var = running_var; only y is written; 1 launch, no workspace.
   tt_bn_tokens_bwd   from g [rows, C], the gradient with respect to the BN output (already gated and scaled by its producer), z and the
                      saved statistics: dbeta[c] = sum_r g, dgamma[c] = sum_r g xhat, dz = gamma rstd (g - dbeta / rows - xhat dgamma /
                      rows) with xhat = (z - mean) rstd: the `dpre` of tt_conv3x3_tokens_bwd_weight / _bwd_data.  2 launches. */
int tt_bn_tokens_shape_ok(long long rows, int C, int training);
size_t tt_bn_tokens_fwd_workspace_bytes(long long rows, int C);
int tt_bn_tokens_fwd(const float* z, const float* gamma, const float* beta, const float* out_scale, float* running_mean, float* running_var,
                     float* y, float* save_mean, float* save_rstd, long long rows, long long rows_per_image, int C, int training, int act,
                     double momentum, double eps, void* workspace, size_t workspace_bytes, tt_stream_t stream);
size_t tt_bn_tokens_bwd_workspace_bytes(long long rows, int C);
int tt_bn_tokens_bwd(const float* g, const float* z, const float* save_mean, const float* save_rstd, const float* gamma, float* dz,
                     float* dgamma, float* dbeta, long long rows, int C, void* workspace, size_t workspace_bytes, tt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TIMETUNING_HIP_H */
