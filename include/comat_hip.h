/*
 * comat_hip.h — C ABI of libcomat_hip.so: the MI355X (gfx950) kernels behind the CoMat training step.
 *
 * The reference (CaraJ7/CoMat) has no FFI: its "operator API" for the hot path is the set of Python call
 * conventions listed in SURVEY.md §8(b).  Every entry point below replaces the third-party kernel class that the
 * cited reference line launches (through diffusers / transformers / torch).  Conventions:
 *   - plain C types only; device pointers are raw `void*`; the caller (PyTorch-ROCm) owns every buffer,
 *     including workspaces; the library never allocates, frees or keeps state between calls;
 *   - all work is enqueued on the caller's `hipStream_t` (passed as void*), no internal synchronisation;
 *   - return 0 on success, a negative COMAT_E* code otherwise; `comat_last_error()` gives a thread-local message;
 *   - activations are channels-last token matrices: an image tensor (B,H,W,C) is the row-major matrix
 *     [B*H*W, C]; attention maps are [B, heads, N, L] row-major (== the reference's (B*h, N, 77) layout,
 *     attn_utils/tc_attn_utils.py:198-217);
 *   - dtype codes: COMAT_F32 (fp32 storage, exact-f32 MFMA 32x32x2) and COMAT_BF16 (bf16 storage,
 *     MFMA 32x32x16, fp32 accumulate).  Biases, norm statistics, losses and optimizer state are always fp32.
 *   - non-finite values: NaN and +-Inf are ordinary values and are CARRIED.  An output whose definition, evaluated on the inputs,
 *     is not finite is not finite (NaN and Inf are not told apart); one that does not depend on the non-finite input is what it
 *     would be without it.  An e4m3 byte made from a NaN is the NaN byte (0x7F / 0xFF), from +-Inf under a finite scale the
 *     saturated +-448; the abs-max of a tensor that holds a NaN is NaN (its word orders above Inf's), and so is the scale made
 *     of it.  What an entry point EXCLUDES is not read, whatever it holds: R when beta == 0, a key under key_mask or the causal
 *     mask (its probability is 0), the logits of a row with ignore_index (its gradient is 0), a convolution tap outside the
 *     image, a window position of comat_resample2d whose weight is 0, the pad columns beyond C of a leading dimension, a table
 *     row or map column that no index names, a comat_weights_refresh_q8 problem of slot -1 (for the bytes and scales), the
 *     scale and history of a site that saw no tensor, eps and stats of comat_ddpm_step2_bwd without deps.  The optimizer's skip (comat_sumsq -> comat_adamw*) relies on this rule.
 */
#ifndef COMAT_HIP_H
#define COMAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COMAT_ABI_VERSION 8

enum { COMAT_F32 = 0, COMAT_BF16 = 1,
       COMAT_FP8_E4M3 = 2 /* OCP e4m3fn bytes; operand dtype of comat_gemm / comat_conv2d only (comat_fp8_quantize) */ };
enum { COMAT_OK = 0, COMAT_EINVAL = -1, COMAT_ELAUNCH = -2, COMAT_EUNSUPPORTED = -3 };
enum { COMAT_ACT_NONE = 0, COMAT_ACT_SILU = 1, COMAT_ACT_GELU = 2 };

int comat_abi_version(void);
const char* comat_last_error(void);
/* 16 hex digits: a hash of the sources (kernels, headers, plan table, build flags) this library was built from.  Profiles of
 * the library (rocprofv3 counter passes under profiles/) record it; bench.py quotes them only for the library they describe. */
const char* comat_build_id(void);
/* Kernel-selection options for A/B runs, microbenchmarks and the parity tests of every kernel variant: "flash_trim",
 * "flash_tr", "flash_kt", "flash_merge", "gemm2", "gemm2_tt", "g2_cfg", "g2_splits", "force_splits", "norm_fused".  Each defaults to the environment variable
 * COMAT_<NAME> (read once) or its built-in default.  They select among kernels that compute the same function; results
 * differ at most in floating-point summation order. */
int comat_set_option(const char* name, int32_t value);
/* Which kernel served the calling thread's last comat_gemm / comat_gemm_segments / comat_conv2d call: 0 the general
 * 64x64 kernel, 1 the LDS-DMA pipelined kernel, 2 its k-major (transA && transB) variant, 3 its fp8 (e4m3, 32x32x64
 * MFMA) variant, 4 the grouped k-major kernel (comat_gemm_tt_grouped), 6 / 7 the pipelined / the general conv weight-gradient
 * kernel (comat_conv2d_wgrad); -1 before the first call.
 * bench.py and the tests use it to attribute time and to assert that a problem runs on the kernel the docs say. */
int comat_last_gemm_kernel(void);

/* ------------------------------------------------------------------------------------------------------------
 * GEMM:  C = act(alpha * op(A) op(B)^T + bias + bias2) + beta * R         (fp32 accumulate on MFMA)
 *   transA == 0: A is [M,K] row-major (lda = row stride);  transA == 1: A is stored [K,M] (lda = stride of k).
 *   transB == 0: B is [N,K] row-major (a torch Linear weight);  transB == 1: B is stored [K,N].
 *   Two-level batch (batch1 x batch2) with independent element strides lets attention heads be addressed in
 *   place inside [tokens, heads*dim] matrices.
 * Replaces: every nn.Linear / 1x1 conv / torch.bmm on the path — UNet to_q/to_k/to_v/to_out + LoRA
 * (training_utils/pipeline.py:94-115), proj_in/out, GEGLU FFN, time embedding; the patched attention's
 * QK^T and `torch.bmm(attention_probs, value)` (attn_utils/tc_attn_utils.py:126-146); BLIP ViT/decoder linears
 * (concept_mat_utils/caption_blip.py:57); the VAE attention (TrainableSDPipeline.py:220).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const void* A; const void* B; void* C;
    const float* bias;   /* [N] fp32 or NULL */
    const float* bias2;  /* [M / rows_per_bias2, N] fp32 or NULL (per-row-group bias, e.g. time embedding) */
    const void* R;       /* residual, same shape as C, or NULL.  May alias C (accumulate). */
    int64_t M, N, K;
    int64_t lda, ldb, ldc, ldr;
    int64_t batch1, batch2;
    int64_t sA1, sA2, sB1, sB2, sC1, sC2, sR1, sR2;
    int64_t rows_per_bias2;
    float alpha, beta;
    int32_t transA, transB;
    int32_t act;
    int32_t in_dtype;   /* dtype of A and B */
    int32_t out_dtype;  /* dtype of C */
    int32_t r_dtype;    /* dtype of R */
    void* ws;           /* optional caller-owned split-K workspace (NULL: never split), see below */
    int64_t ws_bytes;
    /* in_dtype == COMAT_FP8_E4M3: device pointers to the per-tensor dequantisation scales of A and B (value = scale *
     * fp8), NULL = 1.  The product is scaled by *scale_a * *scale_b before bias / activation / residual.  fp8 operands
     * need transA == transB == 0, K % 64 == 0, lda/ldb % 16 == 0; anything else is COMAT_EINVAL (no silent fallback). */
    const float* scale_a;
    const float* scale_b;
    /* Second epilogue (ABI 5; comat_gemm only; ONE launch for the problems the pipelined kernel takes, else the plain product
     * followed by comat_geglu_il_fwd - epi2 = 2 then needs M * N * 2 bytes of `ws` behind the counters - the same function):
     *   epi2 = 1 / 2: GEGLU.  The N = 2 D output columns hold value and gate channels INTERLEAVED in sixteens (columns
     *   32 t .. 32 t + 15 = value channels 16 t .., columns 32 t + 16 .. 32 t + 31 = their gate channels: the caller permutes
     *   the rows of B and the bias once); C2 [M, D] (leading dimension ldc2) receives value * gelu(gate), both rounded to bf16
     *   first.  epi2 = 1 also stores the pre-activations to C (what the backward pass reads), epi2 = 2 does not (C may be
     *   NULL).  bf16 output, N % 32 == 0, 16-byte aligned rows; no residual, bias2, activation or batch.
     *   epi2 = 3 (ABI 6): the GEGLU BACKWARD.  The product is dF [M, N] (the data-gradient of `ff.net.2`: the gradient of the hidden
     *   activations f = value * gelu(gate)); C2 [M, 2 N] holds the saved pre-activations in the interleaved layout (input), C
     *   [M, 2 N] receives their gradient in the same layout: d value = dF * gelu(gate), d gate = dF * value * gelu'(gate), dF
     *   rounded to bf16 first (the bits of the two-launch form).  bf16, N % 16 == 0, ldc, ldc2 >= 2 N, 16-byte aligned rows,
     *   no bias / residual / activation / batch.
     * (epi2 = 1 .. 3) replace the separate GEGLU kernel behind `ff.net.0.proj` of every BasicTransformerBlock (3P diffusers GEGLU, reached
     * from TrainableSDPipeline.py:144-150): one launch and one [M, 2 D] read less per block, and no [M, 2 D] write at all in
     * the no-grad denoise steps.
     *   epi2 = 4 (ABI 7): TAIL COLUMNS.  The product has N = N1 + n2 columns; its last n2 rows of B come from a second matrix B2
     *   (row-major [n2, K], leading dimension ldb like B, batch stride sB2_tail) and its last n2 COLUMNS go to a second output
     *   C2 [M, n2] (leading dimension ldc2, batch stride sC2_tail, out_dtype) as alpha2 * A B2^T - no bias, activation or residual;
     *   the first N1 = N - n2 columns get the whole first epilogue (bias [N1], bias2 [.., N1], R, act) into C.  transA = transB = 0,
     *   batch2 = 1; n2 and N1 multiples of 8 and 16-byte aligned rows for the one-launch form, else (and outside the pipelined
     *   kernel) two launches with the same results.
     *   One launch replaces a frozen-plus-merged projection and the rank-r product that shares its A operand: the forward
     *   `y = x W_eff^T` with `h = s x D^T` (the LoRA down projection, training_utils/pipeline.py:94-115, needed again by the factor
     *   gradient dU += g^T h), and the data-gradient `dx = g W_eff` with `u = s g U` (needed by dD += u^T x). */
    void* C2;
    int64_t ldc2;
    int32_t epi2;
    /* epi2 = 4 only (ABI 7) */
    const void* B2;
    int64_t n2, sB2_tail, sC2_tail;
    float alpha2;
    /* ABI 8, fp8 operands with batch1 > 1: batch z is scaled by scale_b[z * s_scale_b] (0: one scale for every batch) - the
     * q / k / v projections of one attention share their input (one scale_a) but carry a scale per frozen weight */
    int64_t s_scale_b;
    /* ABI 8, fp8 operands only: a MIXED-PRECISION K TAIL in the same launch,
     *     C = act(alpha * (scale_a * scale_b * A B^T + A2k B2k^T) + bias + bias2) + beta * R
     * with A2k [M, K2] and B2k [N, K2] in bf16 (row strides lda2k / ldb2k, batch1 strides sA2k / sB2k, in elements; K2 a multiple
     * of 16, 16-byte aligned rows; NULL: none).  This is the LoRA branch of a frozen projection under the fp8 forward:
     * y = x8 W8^T (e4m3 MFMA) + h U^T (bf16 MFMA, h = s x D^T) - `training_utils/pipeline.py:94-115` - without a second launch and
     * without the read-modify-write of y. */
    const void* A2k;
    const void* B2k;
    int64_t K2, lda2k, ldb2k, sA2k, sB2k;
    /* ABI 8, epi2 = 1 / 2 on the pipelined kernel only (else COMAT_EINVAL): the GEGLU epilogue ALSO emits q8 [M, N / 2] (leading
     * dimension ldq8) = the e4m3 bytes of value * gelu(gate) under *q_scale, and folds its abs-max into *q_amax - what
     * comat_fp8_quantize_scaled would make of C2, for the `ff.net.2` product that consumes it (delayed scaling, see the fp8 section).
     * With q8 given C2 may be NULL: the bf16 copy is then never written. */
    void* q8;
    const float* q_scale;
    uint32_t* q_amax;
    int64_t ldq8;
} comat_gemm_params;
int comat_gemm(const comat_gemm_params* p, void* stream);

/* Split-K workspace (comat_gemm, comat_gemm_segments, comat_conv2d).  Problems with few output tiles and a long
 * contraction are cut along k; the partial tiles are combined INSIDE the launch by the last-arriving workgroup of
 * each tile, in slice order (bit-reproducible; no reduce launch).  Layout of `ws`:
 *   [0, COMAT_WS_COUNTER_BYTES)  uint32 ticket counters, one per output tile.  The caller zeroes this region ONCE
 *                                 (before the first call that receives the buffer); every launch restores the zeros.
 *   [COMAT_WS_COUNTER_BYTES, ws_bytes)  fp32 partial tiles.
 * One workspace serves any number of calls on ONE stream; calls that may overlap (different streams) need a
 * workspace each.  comat_gemm_workspace_bytes() returns the size that lets a problem use its full planned split (a
 * smaller buffer only lowers the split count).  It does NOT include the scratch of the two-launch forms of the second epilogue
 * (epi2 = 2 or 3 on a problem the pipelined kernel declines: M * N * 2 bytes behind the counters, see comat_gemm_params::epi2):
 * a caller that relies on those forms adds it. */
#define COMAT_WS_COUNTER_BYTES (256 * 1024)
int64_t comat_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t batch, int32_t in_dtype);

/* K-segmented GEMM:  C = act(alpha * sum_s A_s[M, K_s] B_s[N, K_s]^T + bias + bias2) + beta * R   (1 <= nseg <= 8).
 * Every A_s / B_s is k-contiguous (row-major [rows, K_s] with leading dimension lda / ldb); M, N, the dtypes, the
 * epilogue and the workspace come from `p` (its A, B, K, lda, ldb, trans*, batch2 fields are ignored / must be 0).
 * p->batch1 > 1 runs that many independent problems in one launch (q/k/v projections of one activation): C and R
 * advance by p->sC1 / p->sR1 elements, bias (if any) is [batch1, N], each segment's operands by sA / sB.
 * One launch replaces the chains  y = x W^T + b;  y += (x D^T) U^T  (LoRALinearLayer added to a frozen nn.Linear,
 * training_utils/pipeline.py:95-115) and  dx = sum_i g_i W_i + u D  (the data-gradient of q/k/v projections that
 * share one input plus their low-rank branches). */
typedef struct {
    const void* A; const void* B;
    int64_t K, lda, ldb;
    int64_t sA, sB;   /* element stride of A_s / B_s between batch items (p->batch1 items; 0 = shared operand) */
} comat_gemm_segment;
int comat_gemm_segments(const comat_gemm_params* p, const comat_gemm_segment* segs, int32_t nseg, void* stream);

/* Grouped k-major products:  C_p[M_p, N_p] += A_p^T B_p  for nprob INDEPENDENT problems, fp32 accumulation in place.
 *   A_p is stored [K_p, M_p] (lda = element stride between k-rows), B_p is stored [K_p, N_p], both bf16; C_p is fp32
 *   row-major with leading dimension ldc.  M_p, N_p multiples of 8 (>= 8); any K_p >= 1; lda, ldb multiples of 8, ldc of 4;
 *   operands 16-byte aligned.  The C_p of one call must not overlap each other (the problems run concurrently); two calls
 *   on one stream are ordered.  A violated requirement is COMAT_EINVAL before anything is launched.
 * These are the LoRA weight gradients of a backward pass - dU = g^T h and dD = u^T x contract over the token axis of two
 * row-major token matrices - which the reference leaves to autograd's addmm, one small launch per factor
 * (training_utils/pipeline.py:84-115: LoRALinearLayer on to_q / to_k / to_v / to_out.0 of every Attention; ~720 factors
 * gradients per SD1.5 step).  Nothing reads them before the optimizer, so the caller queues them and hands them over in
 * groups: one launch per <= 48 problems fills the chip, and the split-K combines (in-launch, fixed slice order:
 * bit-reproducible for a given grouping) overlap across problems.  `ws` as for comat_gemm (zeroed ticket counters at its
 * head); without a workspace no problem is split. */
typedef struct {
    const void* A; const void* B; void* C;
    int64_t M, N, K;
    int64_t lda, ldb, ldc;
} comat_tt_problem;
int comat_gemm_tt_grouped(const comat_tt_problem* probs, int32_t nprob, int32_t in_dtype, void* ws, int64_t ws_bytes,
                          void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * conv2d as implicit GEMM on channels-last tensors.
 *   X: [B, Hin, Win, Cin], W: [Cout, KH, KW, Cin] (K-contiguous), Y: [B, Hout, Wout, Cout].
 *   mode 0 (forward gather):    src = dst*stride + k - pad   (in the `ups`-times nearest-upsampled input)
 *   mode 1 (transposed gather): src = (dst + k - pad)/stride, taken only when divisible  (dgrad of a strided conv)
 *   The data-gradient of a stride-1 conv is mode 0 with the tap-flipped, channel-transposed weight.
 *   Epilogue as in comat_gemm (bias [Cout], bias2 [B, Cout] = per-sample time-embedding add, residual R).
 * Replaces: cuDNN conv2d of ResnetBlock2D / Downsample2D / Upsample2D / conv_in / conv_out in the UNet call
 * (TrainableSDPipeline.py:144-150), the discriminator UNet (training_utils/gan_sdxl.py:72-88,112-131) and the
 * VAE decoder (TrainableSDPipeline.py:220).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const void* X; const void* W; void* Y;
    const float* bias; const float* bias2; const void* R;
    int32_t B, Hin, Win, Cin, Hout, Wout, Cout;
    int32_t KH, KW, stride, pad, mode, ups;
    float alpha, beta;
    int32_t act;
    int32_t in_dtype, out_dtype, r_dtype;
    void* ws;           /* optional caller-owned split-K workspace (layout: see comat_gemm) */
    int64_t ws_bytes;
    const float* scale_a;  /* in_dtype == COMAT_FP8_E4M3 (mode 0, Cin % 64 == 0): per-tensor scales of X and W, as in */
    const float* scale_b;  /* comat_gemm_params */
} comat_conv_params;
int comat_conv2d(const comat_conv_params* p, void* stream);

/* Weight gradient of comat_conv2d mode 0 (additions to ABI 8: nothing existing changes its signature, comat_abi_version()
 * stays 8):
 *     dW[co, kh, kw, ci] += sum over (b, oy, ox) of dY[b, oy, ox, co] * Xu[b, oy * stride + kh - pad, ox * stride + kw - pad, ci]
 * with Xu the `ups`-times nearest-upsampled, zero-padded input.  X [B, Hin, Win, Cin] and dY [B, Hout, Wout, Cout] are dense
 * channels-last tensors of in_dtype (bf16 or fp32); dW [Cout, KH, KW, Cin] is fp32 in the kernel layout of W and is ACCUMULATED
 * in place (the caller zeroes it; as comat_gemm_tt_grouped).  Accepted: KH == KW in {1, 3}, stride in {1, 2}, ups in {1, 2}
 * (ups == 2 only with stride 1), pad >= 0, Hout / Wout = what comat_conv2d derives from them, any Cin, Cout >= 1; anything else
 * and a null operand are COMAT_EINVAL before a launch.
 * A non-finite dY element of channel co reaches dW[co] at every tap whose input pixel lies inside the image; at the padding
 * taps its product with the padding zero may or may not be formed - dW[co] may be non-finite there too, no other channel is.
 *   bf16, Cin % 8 == 0, Cout % 8 == 0, 16-byte aligned X, dY, dW: ONE launch of KH * KW k-major products (one per tap, k = output
 *     pixel) on the tile machinery of comat_gemm_tt_grouped; the X operand is gathered by the LDS-DMA (padding taps read a zero
 *     page).  The pixel axis is always cut into slices whose partial tiles are combined inside the launch in slice order
 *     (comat_last_gemm_kernel() == 6).
 *   everything else (fp32 parity mode, Cin = 4 of the decoder's conv_in, Cout = 3 of its conv_out): a plain kernel with
 *     fixed-order partial sums and a second stage (comat_last_gemm_kernel() == 7).
 * No float atomics on either path: the same inputs and the same workspace size give the same bits.  `ws` is laid out as for
 * comat_gemm (zeroed ticket counters at its head); comat_conv2d_wgrad_workspace_bytes() returns what lets a problem use its
 * planned split, a smaller buffer only lowers it, NULL means one slice.
 * Replaces: the cuDNN weight-gradient of every Conv2d of the VAE decoder once `--tune_vae` makes it trainable
 * (training_utils/pipeline.py:68 `vae.requires_grad_(args.tune_vae)`, :170-171 its parameters join the generator's optimizer;
 * the backward of TrainableSDPipeline.py:220). */
typedef struct {
    const void* X; const void* dY; float* dW;
    int32_t B, Hin, Win, Cin, Hout, Wout, Cout;
    int32_t KH, KW, stride, pad, ups;
    int32_t in_dtype;   /* dtype of X and dY */
    void* ws;
    int64_t ws_bytes;
} comat_conv_wgrad_params;
/* training_utils/pipeline.py:68,170-171 (weight gradients of the trainable VAE convs) */
int comat_conv2d_wgrad(const comat_conv_wgrad_params* p, void* stream);
int64_t comat_conv2d_wgrad_workspace_bytes(const comat_conv_wgrad_params* p);

/* Column sums: out[c] += sum over rows of x[row, c]  (x: [M, C] of `dtype` at leading dimension ld, out fp32 [C], accumulated;
 * additions to ABI 8).  The bias gradient of every trainable Conv2d / Linear of the VAE decoder (training_utils/pipeline.py:68,
 * 170-171; autograd's sum over the token axis).  Row chunks are summed by one block each in a fixed order and combined by a
 * second stage in chunk order: no float atomics.  ws: fp32 scratch for the partial sums (NULL or too small: fewer, longer chunks). */
int comat_colsum(const void* x, float* out, int64_t M, int32_t C, int64_t ld, int32_t dtype, float* ws, int64_t ws_bytes,
                 void* stream);
/* Per-sample column sums (addition to ABI 8): out[b, c] = sum over m < M of x[b * M + m, c]   (x: [B * M, C] of `dtype` at leading
 * dimension ld, out fp32 [B, C], WRITTEN: whatever it held is overwritten), every sample in one call.  The gradient of the `bias2`
 * operand of comat_conv2d - the time-embedding projection a ResnetBlock adds per sample, which is trained under
 * `--full_finetuning` (training_utils/pipeline.py:60-61 `unet.requires_grad_(True)`; autograd's sum over the pixels of
 * `hidden_states + temb[:, :, None, None]`).  The fixed-order two-stage sums of comat_colsum: one block per (sample, row chunk,
 * 64 columns), chunks combined in chunk order, no float atomics.  ws: fp32 scratch (NULL or too small: fewer, longer chunks).
 * COMAT_EINVAL: null operand, B < 1 or B > 65535, M < 1, C < 1, ld < C. */
int comat_colsum_batched(const void* x, float* out, int32_t B, int64_t M, int32_t C, int64_t ld, int32_t dtype, float* ws,
                         int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * GroupNorm (+ optional fused SiLU) on [B, HW, C] channels-last, G groups.  stats: [B, G, 2] fp32 (mean, rstd),
 * written by fwd and read by bwd.  ws: caller workspace of COMAT_GN_WS_DOUBLES(B, G) doubles: 4 KiB of uint32 ticket
 * counters (the caller zeroes them ONCE; the kernels re-arm them) followed by the final sums and up to 1024 per-block
 * partial slabs.  The statistics pass and their fixed-order combination (by the last-arriving block of each sample)
 * are ONE launch, the normalisation a second one; sums are bit-reproducible.  One workspace per stream.
 * The sums are taken of x - K, K = the group's first element where samples of the group show an offset of more than
 * ~10 deviations, else 0 (ordinary data is summed as plain x and x^2): a large group mean costs no accuracy.  y must
 * not alias x (the normalisation pass re-reads the samples while other blocks write y).
 * gamma/beta fp32 [C].  bwd returns dx only (norm affine parameters are frozen: training_utils/pipeline.py:68-70);
 * `add` (same layout and dtype as dx, or NULL) is added to dx: the gradient of the branch that bypasses the norm (a
 * ResnetBlock's shortcut, a transformer block's residual), which autograd would otherwise sum in a kernel of its own.
 * Replaces: torch GroupNorm + SiLU in ResnetBlock2D / Transformer2DModel / VAE decoder.
 * ---------------------------------------------------------------------------------------------------------- */
#define COMAT_GN_WS_DOUBLES(B, G) (512 + (int64_t)(B) * (G) * 2 * 1025)
int comat_groupnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, double* ws,
                        int32_t B, int64_t HW, int32_t C, int32_t G, float eps, int32_t silu, int32_t dtype,
                        void* stream);
int comat_groupnorm_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* stats,
                        void* dx, double* ws, int32_t B, int64_t HW, int32_t C, int32_t G, int32_t silu,
                        const void* add, int32_t dtype, void* stream);
/* The affine gradients of the same GroupNorm, for norms that are trained (additions to ABI 8; training_utils/pipeline.py:68,
 * 170-171: `--tune_vae` makes the decoder's GroupNorm weight and bias parameters of the generator's optimizer):
 *     dgamma[c] += sum over (b, pixel) of dz * xhat,   dbeta[c] += sum over (b, pixel) of dz      (fp32 [C], accumulated)
 * with xhat = (x - mean) * rstd from the saved `stats`, z = gamma * xhat + beta, dz = dy * silu'(z) when `silu`, else dy.  A pass
 * of its own next to comat_groupnorm_bwd (which is unchanged); partial sums per row chunk in a fixed order, combined by a second
 * stage in chunk order: no float atomics.  ws: fp32 scratch (NULL or too small: fewer, longer chunks). */
int comat_groupnorm_bwd_affine(const void* dy, const void* x, const float* gamma, const float* beta, const float* stats,
                               float* dgamma, float* dbeta, float* ws, int64_t ws_bytes, int32_t B, int64_t HW, int32_t C,
                               int32_t G, int32_t silu, int32_t dtype, void* stream);

/* LayerNorm over the last dim of [M, C]; stats [M, 2] fp32 (mean, rstd).  bwd: `add` as in comat_groupnorm_bwd. */
int comat_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, int64_t M,
                        int32_t C, float eps, int32_t dtype, void* stream);
int comat_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* stats, void* dx, int64_t M,
                        int32_t C, const void* add, int32_t dtype, void* stream);
/* The affine gradients of the same LayerNorm, for norms that are trained (addition to ABI 8; training_utils/pipeline.py:60-61:
 * `--full_finetuning` makes every parameter of the UNet, the LayerNorms of its transformer blocks included, a parameter of the
 * generator's optimizer):
 *     dgamma[c] += sum over rows of dy * xhat,   dbeta[c] += sum over rows of dy      (fp32 [C], accumulated)
 * with xhat = (x - mean) * rstd from the saved `stats` [M, 2].  A pass of its own next to comat_layernorm_bwd (which is
 * unchanged), under the contract of comat_groupnorm_bwd_affine: partial sums per row chunk in a fixed order, combined by a second
 * stage in chunk order, no float atomics; ws: fp32 scratch (NULL or too small: fewer, longer chunks).
 * COMAT_EINVAL: null operand, M < 1, C < 1. */
int comat_layernorm_bwd_affine(const void* dy, const void* x, const float* stats, float* dgamma, float* dbeta, float* ws,
                               int64_t ws_bytes, int64_t M, int32_t C, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Row softmax of attention scores.  S: [rows, cols] (s_dtype), P: [rows, cols] (p_dtype).
 *   causal != 0: row r attends keys j <= (r % q_len) + causal_offset.   key_mask: int8 [rows / rows_per_mask, cols]
 *   (1 = keep) or NULL.  P is the materialised probability map that the attention-store clones
 *   (attn_utils/tc_attn_utils.py:60-68): written once, coalesced, never copied.
 *   A masked key has probability 0 whatever its score and its row hold; a row without a visible key is all zeros; a NaN or
 *   +Inf among the VISIBLE scores of a row makes every visible probability of that row NaN.
 * bwd: dS = scale * P * (dP - sum_j dP*P).
 * ---------------------------------------------------------------------------------------------------------- */
int comat_softmax_fwd(const void* S, void* P, int64_t rows, int32_t cols, int32_t q_len, int32_t causal,
                      int32_t causal_offset, const int8_t* key_mask, int64_t rows_per_mask, int32_t s_dtype,
                      int32_t p_dtype, void* stream);
int comat_softmax_bwd(const void* P, const void* dP, void* dS, int64_t rows, int32_t cols, float scale,
                      int32_t p_dtype, int32_t dp_dtype, int32_t ds_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused (flash-style) attention for layers whose probability map is not captured: O = softmax(scale Q K^T) V per
 * (batch, head), scores never written to HBM.  Q: [B*Nq, ldq], K/V: [B*Nk, ldk/ldv], O: [B*Nq, ldo] with head h in
 * columns h*d .. (h+1)*d; lse: [B, H, Nq] fp32 log-sum-exp of the scaled scores (saved for backward), evaluated as
 * m + log(sum_j exp(s_j - m)) with m the row maximum: a NaN or +Inf score makes it NaN (not +Inf), and with it the row of O.
 * Head dim d <= 160, multiple of 8 (bf16) / 4 (fp32); leading dims and base pointers 16-byte aligned.
 * bwd: Dbuf [B, H, Nq] fp32 caller workspace; dO has the layout of O; dQ/dK/dV the layouts of Q/K/V.  ws (optional,
 * fp32, ws_bytes): when there are few keys (cross-attention to 77 text tokens) the dK/dV pass cuts its query loop
 * into ranges that write fp32 partials here and are summed in fixed order (bit-reproducible); NULL: never split.
 * Replaces the materialised softmax(QK^T)V of the reference's patched Attention.forward
 * (attn_utils/tc_attn_utils.py:126-146) for self-attention (268 MB of fp16 scores per layer per sample at 64x64).
 * ---------------------------------------------------------------------------------------------------------- */
int comat_flash_attn_fwd(const void* Q, const void* K, const void* V, void* O, float* lse, int32_t B, int32_t H,
                         int32_t Nq, int32_t Nk, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                         float scale, int32_t dtype, void* stream);
/* ABI 8 (fp8 forward, delayed scaling - see the fp8 section below): the same forward that ALSO stores q8 [B*Nq, ldq8] = the e4m3 bytes of
 * its rounded output under *q_scale (layout of O) and folds max |O| into *q_amax: what comat_fp8_quantize_scaled would make of O,
 * for the `to_out` projection that consumes it (attn_utils/tc_attn_utils.py:140-146 feeds `attn.to_out[0]`). */
int comat_flash_attn_fwd_q(const void* Q, const void* K, const void* V, void* O, float* lse, int32_t B, int32_t H,
                           int32_t Nq, int32_t Nk, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                           float scale, int32_t dtype, void* q8, int64_t ldq8, const float* q_scale, uint32_t* q_amax,
                           void* stream);
int comat_flash_attn_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO,
                         const float* lse, float* Dbuf, void* dQ, void* dK, void* dV, int32_t B, int32_t H,
                         int32_t Nq, int32_t Nk, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                         float scale, int32_t dtype, float* ws, int64_t ws_bytes, void* stream);
/* Added within ABI 8 (two new entry points, no signature changes): the same fused attention under a causal limit and a
 * key-padding mask, for the layers that carry a mask and whose probability map nobody reads.  Arguments as comat_flash_attn_fwd /
 * _bwd, then the mask in the words of comat_softmax_fwd: key j is visible to query q of batch entry b iff
 * (!causal || j <= q + causal_offset) && (key_mask == NULL || key_mask[b * Nk + j] != 0); key_mask int8 [B, Nk] (1 = keep), one
 * row per batch entry for all heads; causal_offset any int (the callers pass Nk - Nq).
 * A query without a visible key gets O = 0 and lse = +Inf; its dQ is 0 and it adds nothing to dK / dV.  A NaN or +Inf among a
 * query's VISIBLE scores makes its lse and its row of O NaN - never the all-zero row.  Masked keys receive dK = dV = 0.
 * Kernels: the one-tile forward, dQ (writes Dbuf) and dK/dV kernels; causal launches skip the key tiles beyond the last one a
 * block's queries see (forward, dQ) and the query tiles before the first that sees a block's keys (dK/dV).  Option flash_trim
 * applies; flash_tr, flash_kt, flash_merge, flash_qs and flash_xcd do not.  bwd: ws / ws_bytes are accepted for the sibling's
 * argument list and unused (the masked dK/dV pass never splits its query loop); NULL is fine.
 * Replaces the masked scores -> softmax -> PV sequence of the text paths: the causal self-attention of the CLIP text towers
 * (`text_encoder(ids, attention_mask=None)[0]`, TrainableSDPipeline.py:325-326; the towers of training_utils/pipeline.py:119,
 * 173-174) and the causal + padding-masked decoder self-attention of the BlipForConditionalGeneration forward that Blip.score
 * calls (concept_mat_utils/caption_blip.py:43-59) - three launches with fp32 score and probability maps in HBM forward, five
 * to six with fp32 dP and dS maps backward. */
int comat_flash_attn_masked_fwd(const void* Q, const void* K, const void* V, void* O, float* lse, int32_t B, int32_t H,
                                int32_t Nq, int32_t Nk, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                                float scale, int32_t dtype, int32_t causal, int32_t causal_offset, const int8_t* key_mask,
                                void* stream);
int comat_flash_attn_masked_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO,
                                const float* lse, float* Dbuf, void* dQ, void* dK, void* dV, int32_t B, int32_t H,
                                int32_t Nq, int32_t Nk, int32_t d, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                                float scale, int32_t dtype, float* ws, int64_t ws_bytes, int32_t causal,
                                int32_t causal_offset, const int8_t* key_mask, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Elementwise family (HBM-bound, 16-byte vectorised).
 * ---------------------------------------------------------------------------------------------------------- */
/* QUICK_GELU: x * sigmoid(1.702 x), the `quick_gelu` of CLIP ViT-L/14's text MLP (transformers' QuickGELUActivation,
 * activations.py); backward dx = dy * (s + 1.702 x s (1 - s)) with s = sigmoid(1.702 x). Added within ABI 8: an op code of an
 * existing entry point, no signature changes. */
enum { COMAT_UN_COPY = 0, COMAT_UN_SILU = 1, COMAT_UN_GELU = 2, COMAT_UN_AFFINE = 3, COMAT_UN_QUICK_GELU = 4 };
/* y = f(x) (AFFINE: p0*x + p1); dtype conversion allowed (COPY == cast). Any other op code: COMAT_EINVAL. */
int comat_unary(int32_t op, const void* x, void* y, int64_t n, float p0, float p1, int32_t x_dtype, int32_t y_dtype,
                void* stream);
/* dx = dy * f'(x) */
int comat_unary_bwd(int32_t op, const void* dy, const void* x, void* dx, int64_t n, int32_t dtype, void* stream);
/* out = a*x + b*y (y may be NULL) */
int comat_axpby(float a, const void* x, float b, const void* y, void* out, int64_t n, int32_t x_dtype,
                int32_t y_dtype, int32_t out_dtype, void* stream);
/* GEGLU: x [M, 2D] -> y[m, d] = x[m, d] * gelu(x[m, D + d]) */
int comat_geglu_fwd(const void* x, void* y, int64_t M, int32_t D, int32_t dtype, void* stream);
int comat_geglu_bwd(const void* dy, const void* x, void* dx, int64_t M, int32_t D, int32_t dtype, void* stream);
/* The same on the INTERLEAVED layout of the fused projection (comat_gemm_params::epi2): x, dx [M, 2 D] with value / gate
 * channels interleaved in sixteens, y, dy [M, D]; D % 16 == 0, 16-byte aligned operands.  16-byte accesses. */
int comat_geglu_il_fwd(const void* x, void* y, int64_t M, int32_t D, int32_t dtype, void* stream);
int comat_geglu_il_bwd(const void* dy, const void* x, void* dx, int64_t M, int32_t D, int32_t dtype, void* stream);
/* strided 2-D copy (channel concat / split): dst[r, c] = src[r, c] for r < rows, c < cols */
int comat_copy2d(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int64_t cols,
                 int32_t src_dtype, int32_t dst_dtype, void* stream);
/* Two strided 2-D copies of the same row count in ONE launch (ABI 6): dst_i[r, c] = src_i[r, c] for c < cols_i.  The channel
 * concat of a UNet skip connection (`torch.cat([hidden_states, res_hidden_states], dim=1)` in every up-path ResnetBlock of the 3P
 * UNet, reached from TrainableSDPipeline.py:144-150) and its backward split.  16-byte accesses: cols_i and every leading dimension
 * in whole 16-byte vectors, 16-byte aligned pointers (else COMAT_EINVAL: use comat_copy2d twice). */
int comat_copy2d_pair(const void* src0, int64_t ld_src0, void* dst0, int64_t ld_dst0, int64_t cols0, const void* src1,
                      int64_t ld_src1, void* dst1, int64_t ld_dst1, int64_t cols1, int64_t rows, int32_t dtype, void* stream);
/* out[r, c] = x[r, c] + v[c] broadcast over rows (positional embeddings) */
int comat_add_rowvec(const void* x, const void* v, void* out, int64_t rows, int64_t cols, int32_t dtype,
                     void* stream);
/* 2x2 sum pooling [B, 2H, 2W, C] -> [B, H, W, C]: adjoint of the nearest-2x upsample fused in comat_conv2d. */
int comat_sumpool2x2(const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
/* Batched transpose + cast of many small fp32 matrices in ONE launch (the per-optimizer-step refresh of the
 * transposed compute-dtype copies of the LoRA down factors, which lets every LoRA data-gradient run k-contiguous).
 * tiles: device int64 [n_tiles, 6] = (src_off, dst_off, rows, cols, r0, c0) per 32x32 tile;
 * dst[dst_off + c*rows + r] = cast(src[src_off + r*cols + c]). */
int comat_transpose_cast_tiles(const float* src, void* dst, const int64_t* tiles, int64_t n_tiles, int32_t out_dtype,
                               void* stream);
/* Merged LoRA weights of MANY projections in ONE launch (ABI 6; once per optimizer step):
 *     Wm_p[N, K] = bf16(W_p + scale * U_p[N, r] D_p[r, K]),     WmT_p[K, N] = Wm_p^T
 * i.e. the weight of the function the reference's LoRA-wrapped Linear computes, y = W x + s * up(down(x))
 * (training_utils/pipeline.py:94-115).  The trained and the no-grad calls of a step then run ONE plain GEMM per projection
 * (forward on Wm, data-gradient on WmT) instead of a rank-r product in front of a K-segmented one.
 *   problems: device int64 [n_problems, 10] = (W, U, Dt, Wm, WmT: device addresses; WmT may be 0), N, K, r, ldu, lddt:
 *             W, Wm bf16 [N, K] contiguous; WmT bf16 [K, N] contiguous; U bf16 [N, r] with leading dimension ldu;
 *             Dt = D^T bf16 [K, r] with leading dimension lddt.  N % 8 == K % 8 == 0, r % 16 == 0, ldu % 8 == lddt % 8 == 0,
 *             every address 16-byte aligned.
 *   tiles:    device int32 [n_tiles, 3] = (problem, n0, k0), one 64 x 64 output tile each (a launch may cover any subset). */
int comat_lora_merge(const int64_t* problems, const int32_t* tiles, int64_t n_tiles, float scale, void* stream);
/* The compute copies of MANY fully trained weights in ONE launch (addition to ABI 8; once per optimizer step, under
 * `--full_finetuning`: training_utils/pipeline.py:60-61 trains every UNet parameter in place, training_script.py:661-664 the
 * optimizer step after which the next forward reads the new values).  The optimizer updates a flat fp32 `master`; the products
 * read each weight in the compute dtype in two orientations, both derived here from the master:
 *     w [R, C]  = dtype(master[R, C]),     wt [C, R] = w^T       (the same bits, transposed; ONE round-to-nearest-even to bf16)
 * A Linear [N, K] is one such matrix.  A conv weight in the kernel layout [Cout, KH, KW, Cin] is one matrix PER TAP t = kh KW + kw:
 * R = Cout rows at pitch KH KW Cin from offset t Cin, C = Cin; its transpose lands at tap KH KW - 1 - t (both taps flipped) of the
 * data-gradient weight wd [Cin, KH, KW, Cout], at pitch KH KW Cout.
 * problems: device int64 [n, 8] = (src, w, wt, R, C, lds, ldw, ldt) per matrix: ELEMENT offsets into `master`, `w`, `wt` and the
 * row pitches of the three.  tiles: device int32 [n_tiles, 3] = (problem, r0, c0), one per 64 x 64 block of a problem's [R, C],
 * r0 and c0 multiples of 64; one workgroup per tile.  The host builds both tables once (comat_amd/refresh.py).
 * dtype = COMAT_BF16: `w` and `wt` are bf16 buffers, both written.  dtype = COMAT_F32: the master IS the forward copy, `w` is
 * ignored (may be NULL) and only `wt` (fp32) is written.
 * A tile goes through LDS so that both copies leave in 16-byte rows; tile edges and rows that are not 16-byte aligned (base
 * address or pitch) are moved element by element.  Nothing outside a problem's [R, C] (source) / [R, C] and [C, R] (destinations)
 * is touched.  The tables are trusted: offsets and pitches must describe memory inside the three buffers.
 * COMAT_EINVAL: null master / wt / problems / tiles, null w in bf16 mode, n_tiles outside [1, 2^31), another dtype. */
int comat_weights_refresh(const float* master, void* w, void* wt, const int64_t* problems, const int32_t* tiles,
                          int64_t n_tiles, int32_t dtype, void* stream);
/* comat_weights_refresh that ALSO re-quantises the fp8-eligible weights for the fp8 forward of a fully trained model (addition
 * to ABI 8; comat_abi_version() stays 8).  `problems` and `tiles` are the tables of comat_weights_refresh, unchanged, and `w` / `wt`
 * receive exactly what that entry point writes for them, bit for bit.  slots: device int32 [n], one entry per problem row:
 * s >= 0 - the problem belongs to quantised weight s (the nine tap matrices of a 3x3 conv share one slot), -1 - not quantised.
 * After the call, in stream order, for every slot s in [0, n_slots) that a problem names:
 *     amax_s    = max |v| over all elements of all problems of the slot; v is the value of the FORWARD copy (the bf16-rounded
 *                 master in bf16 mode, the master itself in fp32 mode)
 *     scales[s] = max(amax_s, 2^-100) / 448                                                         (comat_fp8_scale's rule)
 *     q8[p.w + r p.ldw + c] = e4m3fn_rne(clamp(v * (1 / scales[s]), +-448))  for every element of those problems
 * - comat_fp8_quantize's arithmetic (fp32 reciprocal and product, hardware round-to-nearest-even), the product clamped on every
 * path, tile edges and unaligned rows included: no byte is ever the NaN pattern.  The bytes live at the forward copy's ELEMENT
 * offsets of the byte buffer `q8` (a conv's bytes are [Cout, KH, KW, Cin]).  Nothing else in `q8` or `scales` is written: not
 * the problems with slot -1, not the padding between weights, nothing outside [R, C], no scale of a slot without a problem.
 * amax_bits: device uint32 [n_slots], caller-owned scratch with a convention of its own: it need NOT be initialised - the call
 * zeroes it before its first pass, so nothing an earlier (or an aborted) call left there can reach a scale - and afterwards it
 * holds the float bits of every amax_s.  Two calls on the same stream may share it; calls on concurrent streams may not.
 * Three kernel launches per call whatever the number of weights (one that zeroes amax_bits, the tile pass, the byte pass over the same tile
 * table); no host synchronisation, no allocation, capturable.  The cross-tile maximum is an agent-scope atomic max on the uint
 * bits of a non-negative float: exact and order-independent, the same bits on every run.  Bytes leave in 8-byte rows where
 * q8 + offset and ldw allow, byte by byte at tile edges and on unaligned rows.  bf16 mode moves 4 + 2 x 2 + 2 + 1 = 11 bytes per
 * element of a quantised weight (8 for the others).
 * COMAT_EINVAL (nothing is launched): null master / wt / q8 / scales / amax_bits / problems / slots / tiles, null w in bf16 mode,
 * n_tiles outside [1, 2^31), n_slots < 1, another dtype. */
int comat_weights_refresh_q8(const float* master, void* w, void* wt, uint8_t* q8, float* scales, uint32_t* amax_bits,
                             const int64_t* problems, const int32_t* slots, const int32_t* tiles, int64_t n_tiles,
                             int32_t n_slots, int32_t dtype, void* stream);
/* NCHW <-> NHWC permutation of small boundary tensors (latents, images). to_nhwc != 0: [B,C,H,W] -> [B,H,W,C]. */
int comat_permute_nchw_nhwc(const void* x, void* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t to_nhwc,
                            int32_t x_dtype, int32_t y_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Classifier-free guidance + DDPM ancestral step, fused (fp32, tiny):
 *   eps = e_u + s (e_c - e_u);   x_prev = cx * x + ce * eps + sigma * z
 * with cx, ce the closed-form coefficients of DDPMScheduler.step.  eps2 holds [uncond; cond].
 * Replaces TrainableSDPipeline.py:155-157,166.  bwd: dx = cx*g, de_u = ce*(1-s)*g, de_c = ce*s*g.
 * ---------------------------------------------------------------------------------------------------------- */
int comat_cfg_ddpm_fwd(const float* x, const void* eps2, const float* z, float* x_prev, int64_t n, float s,
                       float cx, float ce, float sigma, int32_t eps_dtype, void* stream);
int comat_cfg_ddpm_bwd(const float* g, float* dx, void* deps2, int64_t n, float s, float cx, float ce,
                       int32_t eps_dtype, void* stream);
/* The same step with RESCALED guidance (`guidance_rescale` = phi > 0: `rescale_noise_cfg`, Lin et al. arXiv 2305.08891 s. 3.4).
 * Additions to ABI 8: nothing existing changes its signature, comat_abi_version() stays 8.
 * Sample b is the contiguous run of per_sample values [b * per_sample, (b + 1) * per_sample) of each half of eps2 (n = batch *
 * per_sample, per_sample % 4 == 0, 16-byte aligned fp32 operands, 8-byte aligned bf16 ones):
 *   e = e_u + s (e_c - e_u);   r_b = std_b(e_c) / std_b(e);   k_b = phi r_b + (1 - phi);   x_prev = cx x + ce k_b e + sigma z
 * stats: fp32 [batch, 4] = (mean, sum of squared deviations) of e_c, then of e, per sample: written by fwd, read by bwd (with
 * the eps2 of the forward).  With g = dL/dx_prev, d = ce g, D_b = sum_i d_i e_i:
 *   dx = cx g;   de = k_b d - D_b phi r_b (e - mu_e) / V_e;   de_c' = D_b phi r_b (e_c - mu_c) / V_c;
 *   de_u = (1 - s) de;   de_c = s de + de_c'.
 * ONE launch each, one block per sample, sums in a fixed order (no atomics: the same bits on every run and graph replay), no
 * workspace.  phi = 0 gives the bits of comat_cfg_ddpm_fwd / _bwd; a sample of zero variance gives non-finite values (as the
 * reference does).  z and dx may be NULL.  Replaces TrainableSDPipeline.py:155-161 (guidance, rescale) and :166 (scheduler step). */
int comat_cfg_rescale_ddpm_fwd(const float* x, const void* eps2, const float* z, float* x_prev, int64_t n, float s,
                               float cx, float ce, float sigma, float phi, int32_t batch, int64_t per_sample,
                               float* stats, int32_t eps_dtype, void* stream);
/* backward of the step above, TrainableSDPipeline.py:155-161 */
int comat_cfg_rescale_ddpm_bwd(const float* g, const void* eps2, const float* stats, float* dx, void* deps2, int64_t n,
                               float s, float cx, float ce, float phi, int32_t batch, int64_t per_sample,
                               int32_t eps_dtype, void* stream);
/* The step of the sampler's other modes (`early_exit`, `double_laststep`, `fast_training`, guidance off).  Additions to ABI 8.
 * The rescaled step above with three more degrees of freedom:
 *   halves = 2: eps holds [uncond; cond], e = e_u + s (e_c - e_u).  halves = 1: guidance is off (guidance_scale <= 1,
 *               TrainableSDPipeline.py:70,135,155), eps is the prediction itself, e = eps, s is ignored and phi must be 0
 *               (the reference skips the rescale without guidance, :159), else COMAT_EINVAL.
 *   x0 = px x + pe (k_b e), the scheduler's `pred_original_sample` (px = 1 / sqrt(abar_t), pe = -sqrt(1 - abar_t) /
 *               sqrt(abar_t)): what `early_exit` returns (:168,175-177), next to x_prev = cx x + ce (k_b e) + sigma z.  Either
 *               output may be NULL, not both; each is two rounded products and a sum, and x_prev has the bits of
 *               comat_cfg_ddpm_fwd (phi = 0, halves = 2) / comat_cfg_rescale_ddpm_fwd (phi > 0) on the same operands.
 *   phi >= 0 with batch, per_sample, stats as above (n = batch * per_sample, per_sample % 4 == 0 and the alignment of the
 *               rescaled kernels, for every phi).  phi = 0: k_b = 1, stats may be NULL, no per-sample pass runs.  The
 *               statistics are computed once and serve both outputs.
 * bwd: g_prev = dL/dx_prev, g_x0 = dL/dx0, either may be NULL, not both.  With d = ce g_prev + pe g_x0:
 *   dx = cx g_prev + px g_x0;   de, de_c' as above with d in place of ce g;   halves = 1: deps = d.
 * dx or deps may be NULL, not both; without deps (an untrained step) eps and stats are not read.  ONE launch each, sums in a
 * fixed order, no atomics, no workspace.  z may be NULL.  Replaces TrainableSDPipeline.py:155-168 and, after the loop, :203-213. */
int comat_ddpm_step2_fwd(const float* x, const void* eps, const float* z, float* x_prev, float* x0, int64_t n,
                         int32_t halves, float s, float cx, float ce, float sigma, float px, float pe, float phi,
                         int32_t batch, int64_t per_sample, float* stats, int32_t eps_dtype, void* stream);
/* backward of the step above, TrainableSDPipeline.py:155-168 */
int comat_ddpm_step2_bwd(const float* g_prev, const float* g_x0, const void* eps, const float* stats, float* dx, void* deps,
                         int64_t n, int32_t halves, float s, float cx, float ce, float px, float pe, float phi,
                         int32_t batch, int64_t per_sample, int32_t eps_dtype, void* stream);
/* Re-noising in front of the extra trained UNet call of `double_laststep` (scheduler.add_noise + torch.cat + cast,
 * TrainableSDPipeline.py:191-195) in ONE launch: noisy[n] = sa x + sb noise in fp32 (sa = sqrt(abar_t), sb = sqrt(1 - abar_t))
 * and xin = `copies` (1 or 2) stacked copies of noisy in xin_dtype, the UNet input.  No backward: nothing in front of it
 * carries a gradient in that mode (every loop step runs without grad, :133,138,163). */
int comat_add_noise_fwd(const float* x, const float* noise, float* noisy, void* xin, int64_t n, float sa, float sb,
                        int32_t copies, int32_t xin_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Denoising fine-tune (noise-prediction MSE), additions to ABI 8: nothing existing changes its signature,
 * comat_abi_version() stays 8.  The reference's SDXL recipe starts from a UNet that diffusers' train_text_to_image_sdxl.py
 * tuned for 100 steps (reference README.md:78-80, loaded through --sdxl_unet_path, training_utils/pipeline.py:27-28); the
 * three entry points below replace the elementwise body of that script's training loop.  csrc/denoise.hip; plain vector
 * stores, no float atomics, no ticket counters, no workspace; every sum runs in ONE order, so equal operands give equal bits.
 * ---------------------------------------------------------------------------------------------------------- */
/* Everything between the VAE encoder (or a stored latent) and the UNet call, in ONE launch - replacing
 * `latent_dist.sample() * scaling_factor`, `noise_scheduler.add_noise(model_input, noise, timesteps)`, the cast to the weight
 * dtype, the timestep's sinusoid (`get_timestep_embedding`) and `compute_snr` + the min-SNR weight of that loop body.
 *   source, exactly one of
 *     moments [B * P, 2 C] (moments_dtype; columns (mean | logvar) - AutoencoderKL.encode's DiagonalGaussianDistribution
 *       parameters) with z fp32 [B * P, C] or NULL:   x0 = scaling * (mean + expf(0.5f * clamp(logvar, -30, 20)) * z),
 *       every operation rounded to fp32 on its own (no fused multiply-add); z == NULL: x0 = scaling * mean, one rounding;
 *     latents fp32 [B * P, C], already scaled (moments == NULL, z == NULL):   x0 = latents;
 *   noisy = fma(sa, x0, sb * noise) with (sa, sb) = sab[tc_b]: the product sb * noise rounded to fp32, then one fused
 *     multiply-add - the bits comat_add_noise_fwd (copies 1) writes for the same sa, sb;  noise fp32 [B * P, C];
 *   xin [B * P, C] = cast(noisy) to xin_dtype;   x0_out fp32 [B * P, C] = x0 (may be NULL);
 *   temb fp32 [B, C0] = sinus[tc_b, :];   w fp32 [B] = wtab[tc_b];
 *   t int32 [B] ON THE DEVICE (nothing of the step is read on the host);  tc_b = min(max(t_b, 0), T - 1): no access leaves the
 *     tables.  oob (int32 [1], zeroed by the caller; may be NULL): 1 is stored when some t_b lies outside [0, T), and nothing
 *     else is ever stored there.
 * The tables are built once by the host: sab fp32 [T, 2] = (sqrt(abar_t), sqrt(1 - abar_t)) rounded to fp32, sinus fp32
 * [T, C0] the timestep embedding of t, wtab fp32 [T] the loss weight (1, or min(snr, gamma) / snr).  The one expf is the only
 * transcendental evaluated on the device.  clamp keeps a NaN logvar (NaN is carried).  B samples of P pixels, C latent
 * channels.  16-byte (fp32) / 8-byte (bf16) accesses where C % 4 == 0 and every base is 16-byte aligned, element accesses
 * otherwise - the same bits.  COMAT_EINVAL: neither or both of moments / latents; z with latents; a null noise, t, sab, sinus,
 * wtab, xin, temb or w; B, P, C, C0 or T <= 0; B > 65535; P * C beyond 2^31 - 1; moments_dtype (with moments) or xin_dtype
 * other than fp32 / bf16. */
int comat_denoise_prepare(const void* moments, const float* z, const float* latents, const float* noise, const int32_t* t,
                          const float* sab, const float* sinus, const float* wtab, void* xin, float* x0_out, float* temb,
                          float* w, int32_t* oob, float scaling, int32_t T, int32_t B, int64_t P, int32_t C, int32_t C0,
                          int32_t moments_dtype, int32_t xin_dtype, void* stream);
/* The loss of that loop body, `F.mse_loss(model_pred.float(), target.float(), reduction="mean")` and, under --snr_gamma, its
 * per-sample weighted form (`mse_loss(..., "none").mean(dim=1..) * mse_loss_weights`, `.mean()`):
 *   per_sample[b] = (1 / n) sum_i (pred[b, i] - target[b, i])^2,   loss[0] = (1 / B) sum_b w_b per_sample[b]   (w NULL: w_b = 1)
 * pred [B, n] of pred_dtype, target fp32 [B, n], w fp32 [B] or NULL, per_sample fp32 [B], loss fp32 [1].  Two launches.  One
 * block of 1 024 lanes per sample, and ONE summation order that depends on n alone (not on B, nor on the alignment): each
 * term is (pred - target)^2 evaluated in fp64 and rounded ONCE to fp32; element i belongs to lane (i / 4) mod 1024, a lane adds
 * its terms to 0 in ascending i (fp32), the 64 lanes of a wave are summed by the xor butterfly 32, 16, .. 1, the 16 wave sums
 * are added to 0 in wave order, and the sum is divided by (float)n.  The second launch adds w_b * per_sample[b] (product
 * rounded, then the sum) to 0 in index order and divides by (float)B.  A non-finite pred element makes per_sample[b] and loss
 * non-finite and no other sample's per_sample.  COMAT_EINVAL: a null pred, target, per_sample or loss; B or n <= 0; B > 65535;
 * another pred_dtype. */
int comat_mse_fwd(const void* pred, const float* target, const float* w, float* per_sample, float* loss, int32_t B, int64_t n,
                  int32_t pred_dtype, void* stream);
/* Its gradient, one launch:   dpred[b, i] = c_b * (pred[b, i] - target[b, i]),   c_b = g w_b 2 / (B n)
 * c_b is evaluated in fp64 as ((g * w_b) * 2) / ((double)B * n) and rounded once to fp32; the difference and the product are
 * fp32; dpred [B, n] is of pred_dtype (one more rounding in bf16).  g: a DEVICE scalar (the gradient arriving at loss[0]), NULL
 * means 1; w NULL: w_b = 1.  A non-finite pred element, g or w_b makes the gradient elements that depend on it non-finite and
 * no others.  COMAT_EINVAL: a null pred, target or dpred; B or n <= 0; B > 65535; another pred_dtype. */
int comat_mse_bwd(const void* pred, const float* target, const float* w, const float* g, void* dpred, int32_t B, int64_t n,
                  int32_t pred_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Image path between VAE and BLIP (training_script.py:606-611, concept_mat_utils/caption_blip.py:33-36,45):
 * separable resampling with precomputed sparse taps (crop + antialiased bicubic + per-channel affine in one
 * pass); the same kernel with transposed tap tables is its adjoint.
 *   in: [B, Hin, Win, C], out: [B, Hout, Wout, C];  ystart[Hout], ywt[Hout, KT], xstart[Wout], xwt[Wout, KT];
 *   out = scale[c] * sum_ty sum_tx ywt*xwt*in[ystart+ty, xstart+tx, c] + shift[c]
 * ---------------------------------------------------------------------------------------------------------- */
int comat_resample2d(const void* in, void* out, int32_t B, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                     int32_t C, const int32_t* ystart, const float* ywt, const int32_t* xstart, const float* xwt,
                     int32_t KT, const float* scale, const float* shift, int32_t in_dtype, int32_t out_dtype,
                     void* stream);
/* ViT patch embedding gather: img [B, H, W, C] -> patches [B*(H/P)*(W/P), P*P*C] (fwd) and its adjoint (bwd). */
int comat_patchify(const void* img, void* patches, int32_t B, int32_t H, int32_t W, int32_t C, int32_t P,
                   int32_t inverse, int32_t dtype, void* stream);
/* rows of a table: out[i, :] = table[ids[i], :] */
int comat_embedding(const int64_t* ids, const void* table, void* out, int64_t n, int32_t dim, int64_t vocab,
                    int32_t dtype, void* stream);
/* The embeddings of a text tower that is trained in full (additions to ABI 8, comat_abi_version() stays 8; `--tune_text_encoder`:
 * training_utils/pipeline.py:69,173-174 put every parameter of the tower, its two tables included, into the optimizer, and
 * training_script.py:304-305 keeps them fp32).
 * Forward, replacing `inputs_embeds + position_embeddings` of transformers' CLIPTextEmbeddings as training_script.py:569-573 runs it:
 *   out[i, :] = cast(tok[clamp(ids[i]), :] + pos[i mod L, :]),  i < n
 * tok [vocab, dim] and pos [npos, dim] are the fp32 MASTER tables (no compute-dtype copy exists), the sum is fp32, rounded once to
 * out_dtype; clamp is comat_embedding's, 0 <= id <= vocab - 1; L <= npos.  16-byte accesses where dim % 8 == 0 and the bases allow. */
int comat_embed_fwd(const int64_t* ids, const float* tok, const float* pos, void* out, int64_t n, int32_t L, int32_t dim,
                    int64_t vocab, int32_t npos, int32_t out_dtype, void* stream);
/* Its gradient (the `index_put_(accumulate=True)` of torch's embedding backward under training_script.py:653), deterministic:
 *   dtable[v, :] += sum over {i < n : clamp(ids[i]) = v} of dy[i, :]
 * dtable fp32 [vocab, dim], accumulated (it may hold an earlier micro-step's sum); dy [n, dim] of dy_dtype.  No atomics, ONE order:
 * the rows of one id are added to 0 in ascending i in fp32 and that sum is added once to dtable's row, so two runs - and a
 * sequential fp32 restatement - give the same bits however often a row repeats (Stable Diffusion pads with the end token).  Rows
 * named by no id are not written.  The position table takes the same call with ids[i] = i mod L.  n <= COMAT_EMBED_GRAD_MAX_N
 * (the occurrence list of one id lives in LDS); a larger n is COMAT_EINVAL before any launch.  Any dim > 0. */
#define COMAT_EMBED_GRAD_MAX_N 4096
int comat_embed_grad(const int64_t* ids, const void* dy, float* dtable, int64_t n, int32_t dim, int64_t vocab,
                     int32_t dy_dtype, void* stream);
/* The pooled output of a text tower with a projection (SDXL's second encoder, `pipeline.text_encoder_2`), replacing
 * `final_layer_norm(last_hidden_state)[arange(B), eos_pos]` of transformers' CLIPTextTransformer.forward (modeling_clip.py:559-581
 * of transformers 5.x; the reference reads it as `text_encoder_2(...)[0]`, training_script.py:516,523 through encode_prompt):
 *   out[b, :] = LayerNorm(h[b * L + pos[b], :]; gamma, beta, eps),  b < B
 * Only B of the B * L rows are normalised, in one launch.  ids int64 [B, L]; h [B * L, C], the LAST layer's output before the final
 * norm; out [B, C] of h's dtype (fp32 or bf16); pos int64 [B] receives the chosen positions and may be NULL.  The position rule is
 * transformers': eos_id == 2 (the configs that shipped with the wrong end token) takes the first position of the largest id,
 * `input_ids.argmax(-1)`; any other eos_id >= 0 the first position whose id equals it, 0 when there is none
 * (`(ids == eos).int().argmax(-1)`).  Ids are compared as given, not clamped.  out[b] carries the bits comat_layernorm_fwd writes for
 * that row under the same pointers' alignment (the kernels share the row routines; a row's result depends on no other row): 16-byte
 * accesses where C % (16 / sizeof T) == 0, C / (16 / sizeof T) <= 256 and the bases are 16-byte aligned, scalar ones otherwise.  Plain
 * vector stores, no atomics, no workspace.  COMAT_EINVAL for a null pointer, B, L or C <= 0, eos_id < 0 or another dtype. */
int comat_eos_pool(const int64_t* ids, const void* h, const float* gamma, const float* beta, void* out, int64_t* pos, int64_t B,
                   int32_t L, int32_t C, int64_t eos_id, float eps, int32_t dtype, void* stream);
/* Decoded image tokens to bytes: the last operator of validation sampling (training_script.py:472 reads the pipeline's `.images`,
 * :489 stacks them as NHWC uint8).  The arithmetic is diffusers' VaeImageProcessor.postprocess followed by numpy_to_pil -
 * `(x / 2 + 0.5).clamp(0, 1)`, then `(... * 255).round().astype("uint8")` - per element, every step rounded to fp32:
 *   v = denorm ? x * 0.5f + 0.5f : x;   v = min(max(v, 0), 1);   p = v * 255.0f;   byte = rint(p)   (round half to even)
 * The multiply by 255 is NOT folded into the affine: fma(x, 127.5, 127.5) gives other bytes.  NaN gives 0, +Inf 255, -Inf 0.
 * x: dense channels-last tokens [B * H * W, C], fp32 or bf16, C in 1 .. 4.  Pixel (y, x, c) of image b goes to byte
 *   (pad + (b / cols) * (H + pad) + y) * out_pitch + (pad + (b % cols) * (W + pad) + x) * C + c
 * of `out`: cols = 1, pad = 0, out_pitch = W * C is the dense [B, H, W, C] batch; anything else places the images on a contact
 * sheet whose other bytes are not touched.  bad (int32 [B], zeroed by the caller; may be NULL): bad[b] = 1 is stored when image b
 * holds a non-finite element, and nothing else is ever stored there (plain vector stores of one value).  Where a 16-byte chunk of
 * the source row and its 4 (fp32) or 8 (bf16) destination bytes are both aligned, a lane loads the chunk and stores its bytes at
 * once; row heads, row tails and rows whose two sides are not aligned alike go element by element, with the same bits.  No LDS, no
 * atomics, no workspace.  COMAT_EINVAL for a null x or out, B, H or W <= 0, C outside 1 .. 4, another dtype, cols < 1, pad < 0 or
 * an out_pitch smaller than the widest row written, (pad + (min(B, cols) - 1) * (W + pad) + W) * C bytes. */
int comat_image_u8(const void* x, uint8_t* out, int32_t* bad, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype,
                   int32_t denorm, int64_t out_pitch, int32_t cols, int32_t pad, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Losses.
 * ---------------------------------------------------------------------------------------------------------- */
/* Token cross-entropy with ignore_index and label smoothing (BLIP decoder LM loss, caption_blip.py:51-58).
 * logits [T, V]; labels int64 [T] (already shifted by the caller); logp[T] = log-prob of the label ("token-level
 * concept score", 0 where ignored); loss_sum_cnt[2] = {sum of per-token losses, number of valid tokens}.  row_lse[t] =
 * m + log(sum_v exp(z_v - m)), m the row maximum: a NaN or +Inf logit makes it NaN.  A valid row with a non-finite loss counts and
 * reaches the sum; the logits of an ignored row reach neither loss, count nor any gradient (its own gradient is 0). */
int comat_cross_entropy_fwd(const void* logits, const int64_t* labels, float* logp, float* row_lse,
                            float* row_loss /* [T] workspace */, float* loss_sum_cnt, int64_t T, int32_t V, int64_t ld,
                            int32_t ignore_index, float label_smoothing, int32_t dtype, void* stream);
/* dlogits = (g_up[0] / loss_sum_cnt[1]) * (softmax - smoothed one-hot) on valid rows, 0 elsewhere.  The upstream
 * gradient and the valid-token count are DEVICE scalars: no host synchronisation in the middle of backward. */
int comat_cross_entropy_bwd(const void* logits, const int64_t* labels, const float* row_lse, void* dlogits,
                            int64_t T, int32_t V, int64_t ld, int32_t ignore_index, float label_smoothing,
                            const float* g_up, const float* loss_sum_cnt, int32_t dtype, void* stream);
/* Discriminator head (training_utils/gan_sdxl.py:32-35,83-88,124-131): pred = x[p, 0:4] . w + b per pixel,
 * BCE-with-logits against target[p / pix_per_sample], mean over pixels.  x: [P, 4] channels-last UNet output.
 * fwd writes loss[0]; bwd writes dx [P,4] and accumulates dw[4], db[1] (fp32, caller zeroes). */
int comat_disc_head_fwd(const void* x, const float* w, const float* b, const float* target, float* loss,
                        float* ws /* >= 512 floats */, int64_t P, int64_t pix_per_sample, int32_t dtype, void* stream);
/* g_up: upstream gradient, a DEVICE scalar.  dwb: [5] = {dw[0..3], db}, accumulated (caller zeroes) or NULL;
 * ws: >= 512*5 floats.  All reductions of this family are two-stage with a fixed order (bit-reproducible). */
int comat_disc_head_bwd(const void* x, const float* w, const float* b, const float* target, const float* g_up,
                        void* dx, float* dwb, float* ws, int64_t P, int64_t pix_per_sample, int32_t dtype,
                        void* stream);
/* Discriminator conv head, `--gan_unet_lastlayer_cls` (additions to ABI 8: nothing existing changes its signature,
 * comat_abi_version() stays 8; training_utils/gan_sdxl.py:27-30,81-82,122-123; checkpoint training_script.py:196-200,426): the
 * discriminator UNet's conv_out is a trainable nn.Conv2d(C, 1, 3, padding=1) and its output IS the logit map.
 *   x [B*H*W, C] channels-last tokens in the compute dtype (the output of conv_norm_out + SiLU), 16-byte aligned, C % 8 == 0,
 *   8 <= C <= 1024;  w fp32 [9, C] tap-major, tap = ky * 3 + kx (the Conv2d weight [1, C, 3, 3] permuted by the host);
 *   b fp32 [1];  target fp32 [B];  z fp32 [B*H*W] logits, written by fwd and read by bwd (the conv is not recomputed).
 * fwd:  z[p] = b + sum_tap sum_c x[nbr(p, tap), c] * w[tap, c]  (zero padding 1, stride 1, fp32 accumulation);
 *       loss[0] = mean over the B*H*W pixels of BCE-with-logits(z[p], target[sample(p)]).
 * bwd:  g_up is a DEVICE scalar;  dz[p] = g_up / (B*H*W) * (sigmoid(z[p]) - target);
 *       dx[q, c] = sum_tap dz[q - off(tap)] * w[tap, c] (in-bounds taps only), in the compute dtype, 16-byte aligned;
 *       dwb[tap * C + c] += sum_q x[q, c] * dz[q - off(tap)],  dwb[9 C] += sum_p dz[p]  (fp32 [9 C + 1], caller zeroes).
 *       dwb may be NULL (generator side: the head is frozen), dx may be NULL; both NULL is COMAT_EINVAL.
 * ws: comat_disc_convhead_workspace_bytes(B, H, W, C) bytes, caller-owned, one per stream.  Every cross-block sum goes
 * through partial slabs in it and a second stage of fixed order (parallel over the 9 C + 1 columns): no float atomics,
 * the same bits on every run.  Both entry points are capturable. */
int64_t comat_disc_convhead_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C);
/* training_utils/gan_sdxl.py:72-88,112-131 with gan_unet_lastlayer_cls */
int comat_disc_convhead_fwd(const void* x, const float* w, const float* b, const float* target, float* z, float* loss,
                            float* ws, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
/* backward of the above; the trainable conv of training_utils/gan_sdxl.py:27-30 (checkpoint: training_script.py:196-200,426).
 * As for comat_conv2d_wgrad: under a tap that pairs a non-finite x element with a pixel outside the image the product with the
 * padding zero may be formed - dw[tap, c] of that channel may be non-finite at every tap, no other channel is. */
int comat_disc_convhead_bwd(const void* x, const float* w, const float* z, const float* target, const float* g_up,
                            void* dx, float* dwb, float* ws, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype,
                            void* stream);

/* Attribute-concentration losses on one captured cross-attention map (attn_utils/tc_loss_utils.py:104-167).
 *   amap: [heads, res*res, L] probabilities of ONE sample and ONE layer; mask: [n_obj, res*res] fp32 {0,1};
 *   tok_idx: int32 [n_tok] token positions, tok_obj: int32 [n_tok] owning object.
 * Stage 1 (HBM-bound strided gather, one pass over the map):
 *   num[h, t] = sum_px A[h,px,tok_t] * mask[obj_t, px];  den[h, t] = sum_px A[h,px,tok_t];
 *   avg[t, px] += (1/heads) * A[h,px,tok_t]   (head-mean map per token, accumulated across layers by the caller)
 * The (tiny) remaining reductions are host-side torch on [heads, n_tok] and [n_tok, res*res] tensors.
 * bwd: dA[h,px,tok_t] = sum over the listed t of g_num[h,t]*mask + g_den[h,t] + g_avg[t,px]/heads, zero elsewhere: the
 * kernel writes EVERY element of dA (no zero-fill by the caller).
 * Both passes move the map as one coalesced stream staged through LDS (16-byte accesses) and pick / place the token
 * columns there. */
int comat_attnmap_gather_fwd(const void* amap, const float* mask, const int32_t* tok_idx, const int32_t* tok_obj,
                             float* num, float* den, float* avg,
                             float* ws /* (ceil(npix/128)*2 + npix) * heads * n_tok floats */,
                             int32_t heads, int32_t npix, int32_t L, int32_t n_tok, int32_t dtype, void* stream);
int comat_attnmap_gather_bwd(const float* g_num, const float* g_den, const float* g_avg, const float* mask,
                             const int32_t* tok_idx, const int32_t* tok_obj, void* damap, int32_t heads,
                             int32_t npix, int32_t L, int32_t n_tok, int32_t dtype, void* stream);

/* Attribute concentration on the device (StepConfig.attrcon_on_device; additions to ABI 8): the whole batch per launch, the
 * ragged per-sample shapes read from tables in device memory, so the host neither synchronises nor builds index tensors.
 *
 * comat_mask_resize_any: torchvision Resize(antialias=True) on a bool mask followed by `> 0` (tc_loss_utils.py:88-98).  The
 * triangle taps are non-negative, so out = 1 iff a source pixel inside the window of positive-weight taps is set: a logical OR,
 * no floating point.  masks: uint8 [n, H, W]; ylo, yhi, xlo, xhi: int32 [res], the half-open source range of the positive
 * taps of every output row / column; out: fp32 {0, 1} [n, res * res].  One launch; none for n = 0.  W <= 32768.
 *
 * Tables of the gather family: n_obj, n_tok int32 [bs]; tok_idx (token column), tok_obj (owning object) int32 [bs, TOK];
 * inv_len fp32 [bs, TOK] (1 / tokens of the owning object); masks fp32 {0, 1} [bs, OBJ, npix].  OBJ, TOK: the batch's
 * maxima (rows are padded).  A sample with n_obj = 0 is skipped: nothing is divided by it.  n_tok is clamped into [0, TOK].
 * Table values outside their range are neither refused nor followed out of bounds: a token whose column tok_idx[t] lies outside
 * [0, L) has the value 0 in gather_fwd (num = den = 0, nothing added to avg: the token loss then carries 0 / 0) and gets no
 * gradient in gather_bwd; both gathers clamp tok_obj[t] into [0, OBJ - 1] where they pick the token's mask row.  (The loss
 * call counts a token towards object i only where tok_obj[t] == i.)
 *
 * comat_attrcon_gather_fwd, one map [bs * heads, npix, L]: num, den [bs, heads, TOK] are WRITTEN for t < n_tok
 *   (num = sum_px A mask[obj_t], den = sum_px A at column tok_idx[t]); avg [bs, TOK, npix] += the head-mean of that column.
 * comat_attrcon_loss, one (timestep, layer) of M maps: num, den [M, bs, heads, TOK], avg summed over the M maps;
 *   out[0] = (1 / bs) sum_b (1 / n_obj) sum_m sum_t inv_len[t] (1 - mean_h(num / den))^2
 *   out[1] = (1 / bs) sum_b (1 / n_obj) sum_i mean_px bce(sum_{t in i} avg[t] / M, mask[i])
 *   with bce = (t - 1) max(log(1 - p), -100) - t max(log p, -100); a NaN probability is carried.  The same call writes the
 *   derivatives of out[0] to g_num, g_den [M, bs, heads, TOK] and of out[1] to g_avg [bs, TOK, npix] (elements of tokens
 *   beyond n_tok are left alone); the derivative of a clamped logarithm is 0.
 * comat_attrcon_gather_bwd, one map: damap [bs * heads, npix, L], EVERY element written:
 *   go[0] (g_num mask + g_den) + go[1] g_avg / heads summed over the tokens that name the column, zero elsewhere and in the
 *   whole slice of a sample with n_obj = 0.  go: two fp32 device scalars, the upstream gradients of out[0] and out[1].
 * ws: comat_attrcon_workspace_floats(M, bs, heads, npix, TOK) floats, shared by the calls of one (timestep, layer).
 * No floating-point atomics; every sum has a fixed order: the same inputs give the same bits. */
int comat_mask_resize_any(const uint8_t* masks, const int32_t* ylo, const int32_t* yhi, const int32_t* xlo,
                          const int32_t* xhi, float* out, int32_t n, int32_t H, int32_t W, int32_t res, void* stream);
int64_t comat_attrcon_workspace_floats(int32_t M, int32_t bs, int32_t heads, int32_t npix, int32_t TOK);
int comat_attrcon_gather_fwd(const void* amap, const float* masks, const int32_t* n_obj, const int32_t* n_tok,
                             const int32_t* tok_idx, const int32_t* tok_obj, float* num, float* den, float* avg, float* ws,
                             int32_t bs, int32_t heads, int32_t npix, int32_t L, int32_t OBJ, int32_t TOK, int32_t dtype,
                             void* stream);
int comat_attrcon_loss(const float* num, const float* den, const float* avg, const float* masks, const int32_t* n_obj,
                       const int32_t* n_tok, const int32_t* tok_obj, const float* inv_len, float* g_num, float* g_den,
                       float* g_avg, float* out, float* ws, int32_t M, int32_t bs, int32_t heads, int32_t npix, int32_t OBJ,
                       int32_t TOK, void* stream);
int comat_attrcon_gather_bwd(const float* g_num, const float* g_den, const float* g_avg, const float* masks,
                             const int32_t* n_obj, const int32_t* n_tok, const int32_t* tok_idx, const int32_t* tok_obj,
                             const float* go, void* damap, int32_t bs, int32_t heads, int32_t npix, int32_t L, int32_t OBJ,
                             int32_t TOK, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimizer tail on the flat fp32 LoRA buffers (training_script.py:661-664,692-694).
 * ---------------------------------------------------------------------------------------------------------- */
/* out[0] += sum(x^2)  (caller zeroes out); ws: >= 1024 floats.  Fixed summation order: every data-parallel rank gets
 * the bit-identical norm (and clip factor) from the all-reduced gradient. */
int comat_sumsq(const float* x, int64_t n, float* out, float* ws, void* stream);
/* Norm (and normalisation) of the gradient that reaches the decoded image - the `record_grad` hook of training_script.py:644-651
 * (addition to ABI 8): norm_out[0] = |g|_2 (fp32, fixed summation order; g: n values of `dtype`, fp32 or bf16) and, when
 * target > 0, g_out_i = g_i * (target / |g|_2) with the norm read from device memory (the host never sees it).  g_out may
 * alias g; target = 0 only measures (g_out may be NULL).  |g|_2 = 0: g_out = 0 (a zero gradient stays zero, no 0 * inf); a NaN
 * norm is no zero norm: every g_out_i is NaN.
 * ws: >= 1024 floats.  Two launches. */
int comat_grad_norm_scale(const void* g, void* g_out, int64_t n, int32_t dtype, float* norm_out, float target, float* ws,
                          void* stream);
/* AdamW with the global-norm clip folded in: g' = s g * min(1, max_norm / (s sqrt(*gnorm_sq) + 1e-6)), s = grad_scale:
 * the gradient buffer (and *gnorm_sq, the sum of ITS squares) may hold the SUM over data-parallel ranks, grad_scale =
 * 1 / world makes it the mean (DDP semantics, training_script.py:659) without another pass over the buffer.  A non-finite
 * *gnorm_sq skips the update entirely (p, m, v untouched): the inf/NaN check of a mixed-precision optimizer step.
 * Step count t of the bias correction: `step` (host value, >= 1) when step_dev is NULL; otherwise *step_dev + 1 with
 * the count of APPLIED updates kept in device memory — advanced by comat_adamw_tick after the adamw launches of one
 * optimizer step, and only when the update was applied (so a skipped step does not run the bias correction ahead of
 * the moments, and a captured hipGraph of the whole step replays with the right count). */
int comat_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                float eps, float weight_decay, int32_t step, const int32_t* step_dev, const float* gnorm_sq,
                float max_norm, float grad_scale, void* stream);
/* counters[0] += 1 if *gnorm_sq is finite (update applied), else counters[1] += 1 (update skipped). */
int comat_adamw_tick(int32_t* counters, const float* gnorm_sq, void* stream);

/* Learning-rate schedules, `--lr_scheduler` / `--lr_warmup_steps` / `--max_train_steps` (training_script.py:290-295: the scheduler
 * is built by get_scheduler; :664 `lr_scheduler.step()`; :667 `logs["lr"] = get_last_lr()[0]`).  Additions to ABI 8: nothing
 * existing changes its signature, comat_abi_version() stays 8.
 * The learning rate is a pure function of the count of APPLIED updates, evaluated on the device in double:
 *     clock = stride * counters[0]                                          (64-bit)
 *     lr    = (float)(base_lr * lambda_kind(clock; warmup, total, num_cycles, power, lr_end))
 * with lambda_kind the multiplier of transformers.optimization (= diffusers.optimization) for that name, in its order of
 * operations.  A skipped update leaves counters[0], and so the rate, where it was - accelerate's AcceleratedScheduler does
 * not step after a skipped optimizer step either.  stride: accelerate without split_batches steps the scheduler
 * num_processes times per optimizer step; 1 otherwise.
 * The struct is passed to the kernels BY VALUE: a captured hipGraph bakes the schedule and reads only the counter and the
 * learning-rate word, both at fixed device addresses.
 * COMAT_EINVAL: unknown kind, stride < 1, warmup < 0, total < 1 for linear / cosine / cosine_with_restarts / polynomial,
 * and for polynomial base_lr <= lr_end (the host library raises there).  polynomial with total == warmup is evaluated as
 * written: every clock but clock == total has a value, and there the multiplier is 0 / 0 (the host library raises
 * ZeroDivisionError at that step) and the rate NaN - comat_amd.step.lr_schedule refuses that configuration up front. */
enum { COMAT_LR_CONSTANT = 0, COMAT_LR_CONSTANT_WITH_WARMUP = 1, COMAT_LR_LINEAR = 2, COMAT_LR_COSINE = 3,
       COMAT_LR_COSINE_WITH_RESTARTS = 4, COMAT_LR_POLYNOMIAL = 5 };
typedef struct {
    int64_t kind;       /* COMAT_LR_* */
    int64_t stride;     /* scheduler steps per applied update */
    int64_t warmup;     /* --lr_warmup_steps */
    int64_t total;      /* --max_train_steps (unused by the two constant kinds) */
    double base_lr;     /* --learning_rate */
    double num_cycles;  /* cosine: 0.5, cosine_with_restarts: 1 (get_scheduler's defaults) */
    double power;       /* polynomial: 1.0 */
    double lr_end;      /* polynomial: 1e-7 */
} comat_lr_schedule;
/* lr_out[0] = the rate at the current counters[0] (one thread).  Launched when an optimizer is built and after its state is loaded. */
int comat_lr_schedule_eval(const comat_lr_schedule* sched, const int32_t* counters, float* lr_out, void* stream);
/* comat_adamw_tick, then lr_out[0] = the rate of the NEXT update from the new count (training_script.py:664; the word is what
 * :667 logs).  A skipped update writes neither counters[0] nor lr_out.  One launch. */
int comat_adamw_tick_lr(int32_t* counters, const float* gnorm_sq, const comat_lr_schedule* sched, float* lr_out, void* stream);
/* comat_adamw with the learning rate read from device memory (*lr_dev) and the step count always from *step_dev (both
 * required).  Per element the arithmetic of comat_adamw in the same order: with *lr_dev holding a given float, p, m, v come out
 * bit-identical to comat_adamw called with that float.  16-byte accesses when p, g, m, v are all 16-byte aligned (the n % 4
 * last elements one by one), 4-byte accesses otherwise. */
int comat_adamw_lr(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2,
                   float eps, float weight_decay, const int32_t* step_dev, const float* gnorm_sq, float max_norm,
                   float grad_scale, void* stream);

/* Gradient accumulation, `--gradient_accumulation_steps` N (training_script.py:556,680 `accelerator.accumulate`; used as
 * accelerate documents it: zero_grad AFTER the optimizer step).  Additions to ABI 8.  The state is one device word, `window`
 * (int32 [1]): the index 0 .. N - 1 of the current micro-step inside its window.  A launch CLOSES the window iff
 * window[0] == accum_steps - 1 (accelerate's `sync_gradients`).  Every kernel reads the word when it executes, so one captured
 * hipGraph serves every micro-step.  COMAT_EINVAL: null required pointers, n < 1, accum_steps < 1. */
/* optimizer.zero_grad() of training_script.py:658,689, in the documented place: g[0..n) = 0 iff window[0] == 0, otherwise nothing is
 * written (every block leaves after one uniform load).  16-byte stores when g is 16-byte aligned (the n % 4 last elements one by
 * one), 4-byte stores otherwise. */
int comat_accum_zero(float* g, int64_t n, const int32_t* window, void* stream);
/* comat_adamw_lr under `if accelerator.sync_gradients` (training_script.py:661-664,692-694): when the launch closes, per element the
 * arithmetic of comat_adamw_lr in the same order, bit-identical, the skip on a non-finite *gnorm_sq included; otherwise p, m, v are
 * not written. */
int comat_adamw_window(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2,
                       float eps, float weight_decay, const int32_t* step_dev, const float* gnorm_sq, float max_norm,
                       float grad_scale, const int32_t* window, int32_t accum_steps, void* stream);
/* The bookkeeping of one micro-step (one thread, one launch), after the comat_adamw_window launches:
 *   train_loss[0] = (window[0] == 0 ? 0 : train_loss[0]) + *step_loss / (float)accum_steps     (fp32, in that order; :655)
 *   closing:  comat_adamw_tick_lr (sched non-NULL; lr_out required) or comat_adamw_tick (sched NULL) - a non-finite *gnorm_sq counts
 *             a skipped update and moves neither the count nor the rate (:664 under sync_gradients);
 *             train_loss[1] = train_loss[0] (the value :702 logs); window[0] = 0
 *   else:     window[0] += 1; counters, lr_out and train_loss[1] untouched.
 * step_loss and train_loss (fp32 [1], fp32 [2]) may both be NULL (the discriminator's optimizer); exactly one of them is refused,
 * and so is what comat_adamw_tick_lr refuses in a schedule. */
int comat_window_tick(int32_t* window, int32_t accum_steps, int32_t* counters, const float* gnorm_sq,
                      const comat_lr_schedule* sched, float* lr_out, const float* step_loss, float* train_loss, void* stream);

/* 8-bit blockwise optimizer state, `--use_8bit_adam` (training_script.py:216-223 makes bnb.optim.AdamW8bit the optimizer class;
 * :258-264 the generator's optimizer, :269-275 the discriminator's).  Additions to ABI 8.  bitsandbytes is not linked or ported: the
 * algorithm is restated from its published form (comat_amd/optim8.py; deviations: INTEGRATION.md).
 * A moment is stored as one CODE byte per element and one fp32 SCALE per block of 256 consecutive elements of the flat buffer (the
 * last block may be partial): value = table[code] * scale, scale = the block's max |value|.  Two tables of 256 ascending fp32 values
 * in [-1, 1]: signed (first moment; zero is code 127) and unsigned (second moment; zero is code 0) - optim8.dynamic_map.
 * Every fp32 array must be 16-byte aligned and every code array 4-byte aligned (COMAT_EINVAL otherwise, as for null pointers, n < 1,
 * is_signed not 0 / 1): accesses are 16 bytes per fp32 operand and one word of four codes, the n % 4 last elements one by one.
 * No atomics and no order-dependent arithmetic: equal inputs give equal bits on every launch and every rank. */
/* Copies a table (256 floats) to HOST memory: with comat_last_error / comat_build_id the one entry point whose pointer is not a
 * device pointer; needs no GPU. */
int comat_q8_map(int32_t is_signed, float* host_out256);
/* absmax[b] = the exact max |x| over block b; codes[i] = index of a table entry nearest to x[i] / absmax[b] (at an exact tie either
 * neighbour).  A block whose abs-max is 0 gets the zero code and absmax 0: no division by zero reaches a code. */
int comat_q8_quantize_blockwise(const float* x, uint8_t* codes, float* absmax, int64_t n, int32_t is_signed, void* stream);
/* x[i] = table[codes[i]] * absmax[i / 256], one fp32 product. */
int comat_q8_dequantize_blockwise(const uint8_t* codes, const float* absmax, float* x, int64_t n, int32_t is_signed, void* stream);
/* comat_adamw_window on 8-bit moments (m8 signed, v8 unsigned); window == NULL: every launch closes (the form comat_adamw_lr has).
 * The uniform early exits of comat_adamw_window (a window that does not close, a non-finite *gnorm_sq) come before any store; the
 * clip factor is that kernel's.  Per element: m, v dequantised; the element arithmetic of comat_adamw_lr, same roundings - p moves
 * from the fresh fp32 m', v', never from the requantised ones, so from equal p, g and dequantised moments p comes out bit-identical
 * to comat_adamw_lr's; then the block's new scales max |m'|, max v' and the nearest codes under them. */
int comat_adamw8_window(float* p, const float* g, uint8_t* m8, uint8_t* v8, float* absmax_m, float* absmax_v, int64_t n,
                        const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, const int32_t* step_dev,
                        const float* gnorm_sq, float max_norm, float grad_scale, const int32_t* window /* nullable */,
                        int32_t accum_steps, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Per-tensor fp8 (OCP e4m3fn) quantisation: the operand format of the fp8-forward configuration (BASELINE.json
 * configs[4]: "fp8 MFMA UNet forward with bf16 backward"; the reference itself trains in fp16 autocast,
 * training_script.py:449-456 - fp8 is this project's MI355X target, restated on the CPU by oracle/fp8.py).
 *   comat_fp8_scale:    *scale = max(max_i |x_i|, 2^-100) / 448      (one launch; ws: 8 bytes the caller zeroed once).  ABI 8:
 *                       amax_bits (may be NULL) = the site's running maximum below, which receives the tensor's abs-max too
 *   comat_fp8_quantize: y_i = e4m3fn(x_i * (1 / *scale)), round to nearest even, saturating; y: n bytes
 * x: n elements of `dtype` (fp32 or bf16), 16-byte aligned.  Feed y and scale to comat_gemm / comat_conv2d with
 * in_dtype = COMAT_FP8_E4M3.
 *
 * DELAYED SCALING (ABI 8).  A quantisation SITE (the input of one frozen layer) owns two device words: `scale` (fp32) and
 * `amax_bits` (the float bits of a running abs-max, zeroed once).  During an optimizer step every tensor that passes the site
 * is quantised under the scale that is already there and folds its own abs-max into amax_bits; once per optimizer step
 * comat_fp8_scales_update turns every running maximum that saw a tensor into next step's scale and re-arms it.  One launch per
 * tensor, no reduction anybody waits for - and none at all where the producer of the tensor emits the bytes itself:
 *   comat_fp8_quantize_scaled: y_i = e4m3fn(x_i * (1 / *scale)); *amax_bits = max(*amax_bits, bits(max_i |x_i|))
 *   comat_fp8_scales_update:   for i < n with amax_bits[i] != 0: scale[i] = max(float(amax_bits[i]), 2^-100) / 448, amax_bits[i] = 0
 *       A site whose abs-max is NOT FINITE (+Inf or NaN: an overflowed or poisoned activation, a step whose update the optimizer
 *       skips) is treated as having seen no tensor: scale[i] is kept and only amax_bits[i] is cleared.
 *   comat_fp8_scales_update_hist: the RECIPE form of comat_fp8_scales_update (which it replaces once a recipe is set; with
 *       hist_len = 1, margin = 1 it writes the same scale words, bit for bit): an abs-max HISTORY window of hist_len (1..16) steps
 *       per site (hist [n, hist_len], ring position count[i] % hist_len), a MARGIN >= 1 on the scale, and step-level clip
 *       accounting.  For i < n, b = amax_bits[i]; b == 0 (site unseen this step): nothing changes, clip_now[i] = 0.  float(b) not
 *       finite (+Inf, NaN): the site is treated as unseen too - scale, hist, count, clip_steps and worst untouched, clip_now[i] = 0,
 *       amax_bits[i] = 0 - so that no Inf scale lives for hist_len steps and no NaN stays in the window for good.  Otherwise,
 *       with a = float(b), in fp32 and in this order:
 *         s_a = max(a, 2^-100) / 448
 *         clip_now[i] = account && scale[i] > 0 && s_a > scale[i]; then also clip_steps[i] += 1, worst[i] = max(worst[i], s_a / scale[i])
 *         hist[i, count[i] % hist_len] = a; count[i] += 1
 *         scale[i] = max(max over the first min(count[i], hist_len) slots, 2^-100) * margin / 448; amax_bits[i] = 0
 *       The clip test compares SCALES: fp32 division is monotone, so a step whose abs-max does not exceed margin x the window
 *       maximum is never flagged.  clip_steps / worst / clip_now: all three or none (NULL).  No workspace, no float atomics.
 *   comat_layernorm_fwd_q / comat_groupnorm_fwd_q: the normalisation of comat_layernorm_fwd / comat_groupnorm_fwd that ALSO
 *       stores q8 = the e4m3 bytes of its (rounded) output y under *scale and folds max |y| into *amax_bits: the bits of
 *       comat_fp8_quantize_scaled(y), one launch and one read of y less.  Only the vectorised forms (comat_*_fwd_q_ok -> 1);
 *       other shapes return COMAT_EUNSUPPORTED and the caller runs the two calls.
 * (The reference has no fp8 path: nothing to cite; arithmetic restated by oracle/fp8.py.)
 * ---------------------------------------------------------------------------------------------------------- */
int comat_fp8_scale(const void* x, int64_t n, int32_t dtype, float* scale, void* ws, uint32_t* amax_bits, void* stream);
int comat_fp8_quantize(const void* x, int64_t n, int32_t dtype, const float* scale, void* y, void* stream);
int comat_fp8_quantize_scaled(const void* x, int64_t n, int32_t dtype, const float* scale, void* y, uint32_t* amax_bits,
                              void* stream);
int comat_fp8_scales_update(uint32_t* amax_bits, float* scale, int32_t n, void* stream);
int comat_fp8_scales_update_hist(uint32_t* amax_bits, float* scale, float* hist /*[n, hist_len]*/, int32_t* count /*[n]*/,
                                 int32_t* clip_steps /*[n] or NULL*/, float* worst /*[n] or NULL*/, int32_t* clip_now /*[n] or NULL*/,
                                 int32_t n, int32_t hist_len, float margin, int32_t account, void* stream);
int comat_layernorm_fwd_q_ok(int32_t C, int32_t dtype);
int comat_layernorm_fwd_q(const void* x, const float* gamma, const float* beta, void* y, float* stats, int64_t M, int32_t C,
                          float eps, int32_t dtype, void* q8, const float* scale, uint32_t* amax_bits, void* stream);
int comat_groupnorm_fwd_q_ok(int32_t B, int64_t HW, int32_t C, int32_t G, int32_t dtype);
int comat_groupnorm_fwd_q(const void* x, const float* gamma, const float* beta, void* y, float* stats, double* ws, int32_t B,
                          int64_t HW, int32_t C, int32_t G, float eps, int32_t silu, int32_t dtype, void* q8, const float* scale,
                          uint32_t* amax_bits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COMAT_HIP_H */
