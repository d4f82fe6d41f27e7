// wgrad.hip — the weight-gradient entry points of layers that are trained in full (include/comat_hip.h: comat_conv2d_wgrad,
// comat_colsum, comat_groupnorm_bwd_affine): the VAE decoder under `--tune_vae`; comat_layernorm_bwd_affine and
// comat_colsum_batched: the UNet under `--full_finetuning`.  The pipelined conv weight gradient lives in
// gemm2.hip (it shares the k-major tile machinery); here are its contract, the general kernel for everything that one declines
// (fp32 parity mode, the 4-channel conv_in, the 3-channel conv_out) and the two column-reduction kernels.
// Every sum of this file is two-stage with a fixed order, in the spirit of convhead_bwd_kernel (loss.hip): a block sums one
// chunk of rows per column (threads of one column in LDS, in lane order), a second kernel adds the chunks in chunk order.
#include "gemm_shared.h"
#include "conv_wgrad_decode.h"

int comat_gemm2_try_conv_wgrad(const comat_conv_wgrad_params* p, void* stream);
int64_t comat_gemm2_conv_wgrad_ws_bytes(const comat_conv_wgrad_params* p);

namespace {

constexpr int MAX_CHUNKS = 1024;

// out[i] += sum_c part[c * n + i] in chunk order; i < n0 goes to out0, the rest to out1[i - n0]
__global__ __launch_bounds__(256) void partials_add_kernel(const float* __restrict__ part, int nchunks, int64_t n, float* out0,
                                                           int64_t n0, float* out1) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int c = 0; c < nchunks; ++c) s += part[(int64_t)c * n + i];
    if (i < n0) out0[i] += s;
    else out1[i - n0] += s;
}

// out[i] = sum_c part[c * n + i] in chunk order (the written form: comat_colsum_batched)
__global__ __launch_bounds__(256) void partials_set_kernel(const float* __restrict__ part, int nchunks, int64_t n, float* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int c = 0; c < nchunks; ++c) s += part[(int64_t)c * n + i];
    out[i] = s;
}

// chunks of `rows` rows for a reduction with n outputs per chunk: about `want` rows each, as many as the scratch holds
int plan_chunks(int64_t rows, int64_t want, int64_t n, const float* ws, int64_t ws_bytes) {
    int64_t c = cdiv64(rows, want);
    if (c > MAX_CHUNKS) c = MAX_CHUNKS;
    const int64_t cap = ws ? ws_bytes / (n * 4) : 0;
    if (c > cap) c = cap;
    return c < 2 ? 1 : (int)c;
}

// the 256 per-thread sums of a block -> column sums: thread t < cl adds lanes t, t + cl, ... in that order
__device__ __forceinline__ float fold_lanes(float v, float* sred, int cl) {
    __syncthreads();
    sred[threadIdx.x] = v;
    __syncthreads();
    float s = 0.f;
    if ((int)threadIdx.x < cl)
        for (int j = threadIdx.x; j < 256; j += cl) s += sred[j];
    return s;
}

// ---- conv weight gradient, general ------------------------------------------------------------------------------------
// block (x) = (co, tap, chunk of `cl` input channels), block (y) = chunk of pixels; thread = (channel lane, pixel lane).
// cl = a power of two <= 64: consecutive lanes read consecutive channels of one X row, dY[p, co] is a broadcast.
template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_general_kernel(const T* __restrict__ dY, const T* __restrict__ X, float* out,
                                                                 ConvWgradGeom g, int Cout, int taps, int64_t K, int64_t per, int cl,
                                                                 int ci_chunks, int direct) {
    __shared__ float sred[256];
    int bx = blockIdx.x;
    const int cc = bx % ci_chunks;
    bx /= ci_chunks;
    const int tap = bx % taps, co = bx / taps;
    const int ci = cc * cl + (threadIdx.x % cl), pl = threadIdx.x / cl, npl = 256 / cl;
    const int64_t k0 = (int64_t)blockIdx.y * per, k1 = k0 + per < K ? k0 + per : K;
    float acc = 0.f;
    if (ci < g.Cin)
        for (int64_t p = k0 + pl; p < k1; p += npl) {
            const int64_t off = conv_wgrad_src(g, p, tap);
            if (off != CONV_WGRAD_ZERO) acc += ldf(dY + p * Cout + co) * ldf(X + off + ci);
        }
    const float s = fold_lanes(acc, sred, cl);
    if ((int)threadIdx.x < cl && ci < g.Cin) {
        const int64_t o = ((int64_t)co * taps + tap) * g.Cin + ci;
        if (direct) out[o] += s;
        else out[(int64_t)blockIdx.y * ((int64_t)Cout * taps * g.Cin) + o] = s;
    }
}

// ---- column sums ------------------------------------------------------------------------------------------------------
// block (x) = 64 columns, block (y) = chunk of rows; thread = (column lane, one of 4 row lanes)
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, float* out, int64_t M, int C, int64_t ld, int64_t per,
                                                     int direct) {
    __shared__ float sred[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < M ? r0 + per : M;
    float acc = 0.f;
    if (c < C)
        for (int64_t row = r0 + rl; row < r1; row += 4) acc += ldf(x + row * ld + c);
    const float s = fold_lanes(acc, sred, 64);
    if (threadIdx.x < 64 && c < C) {
        if (direct) out[c] += s;
        else out[(int64_t)blockIdx.y * C + c] = s;
    }
}

// per-sample column sums: as colsum_kernel with block (z) = sample b, rows b * M .. b * M + M - 1; WRITES out[b, c] (direct) or
// the partial slab [chunk, b, c]
template <typename T>
__global__ __launch_bounds__(256) void colsum_batched_kernel(const T* __restrict__ x, float* out, int64_t M, int C, int64_t ld,
                                                             int64_t per) {
    __shared__ float sred[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < M ? r0 + per : M;
    const T* xb = x + (int64_t)blockIdx.z * M * ld;
    float acc = 0.f;
    if (c < C)
        for (int64_t row = r0 + rl; row < r1; row += 4) acc += ldf(xb + row * ld + c);
    const float s = fold_lanes(acc, sred, 64);
    if (threadIdx.x < 64 && c < C) out[((int64_t)blockIdx.y * gridDim.z + blockIdx.z) * C + c] = s;
}

// ---- LayerNorm affine gradients ---------------------------------------------------------------------------------------
// as colsum over the M rows, two sums per column: dy * xhat and dy, xhat from the row's saved (mean, rstd)
template <typename T>
__global__ __launch_bounds__(256) void ln_affine_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ stats,
                                                        float* out0, float* out1, int64_t M, int C, int64_t per, int direct) {
    __shared__ float sred[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < M ? r0 + per : M;
    float ag = 0.f, ab = 0.f;
    if (c < C)
        for (int64_t row = r0 + rl; row < r1; row += 4) {
            const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
            const float d = ldf(dy + row * C + c);
            ag += d * ((ldf(x + row * C + c) - mean) * rstd);
            ab += d;
        }
    const float sg = fold_lanes(ag, sred, 64);
    const float sb = fold_lanes(ab, sred, 64);
    if (threadIdx.x < 64 && c < C) {
        if (direct) {
            out0[c] += sg;
            out1[c] += sb;
        } else {
            out0[(int64_t)blockIdx.y * 2 * C + c] = sg;
            out0[(int64_t)blockIdx.y * 2 * C + C + c] = sb;
        }
    }
}

// ---- GroupNorm affine gradients ---------------------------------------------------------------------------------------
// as colsum over the B * HW rows, two sums per column: dz * xhat and dz
template <typename T>
__global__ __launch_bounds__(256) void gn_affine_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ stats, float* out0,
                                                        float* out1, int64_t M, int64_t HW, int C, int G, int silu, int64_t per,
                                                        int direct) {
    __shared__ float sred[256];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < M ? r0 + per : M;
    float ag = 0.f, ab = 0.f;
    if (c < C) {
        const int grp = c / (C / G);
        const float gm = gamma[c], bt = beta[c];
        for (int64_t row = r0 + rl; row < r1; row += 4) {
            const int64_t b = row / HW;
            const float mean = stats[(b * G + grp) * 2], rstd = stats[(b * G + grp) * 2 + 1];
            const float xh = (ldf(x + row * C + c) - mean) * rstd;
            float dz = ldf(dy + row * C + c);
            if (silu) dz *= silu_grad_f(gm * xh + bt);
            ag += dz * xh;
            ab += dz;
        }
    }
    const float sg = fold_lanes(ag, sred, 64);
    const float sb = fold_lanes(ab, sred, 64);
    if (threadIdx.x < 64 && c < C) {
        if (direct) {
            out0[c] += sg;
            out1[c] += sb;
        } else {
            out0[(int64_t)blockIdx.y * 2 * C + c] = sg;
            out0[(int64_t)blockIdx.y * 2 * C + C + c] = sb;
        }
    }
}

int conv_wgrad_check(const comat_conv_wgrad_params* p, const char* who) {
    COMAT_REQUIRE(p != nullptr, "%s: null parameter block", who);
    COMAT_REQUIRE(p->X && p->dY && p->dW, "%s: null operand", who);
    COMAT_REQUIRE(dtype_ok(p->in_dtype), "%s: operands must be bf16 or fp32", who);
    COMAT_REQUIRE(p->KH == p->KW && (p->KH == 1 || p->KH == 3), "%s: KH == KW in {1, 3} (got %d x %d)", who, p->KH, p->KW);
    COMAT_REQUIRE(p->stride == 1 || p->stride == 2, "%s: stride in {1, 2} (got %d)", who, p->stride);
    COMAT_REQUIRE(p->ups == 1 || (p->ups == 2 && p->stride == 1), "%s: ups in {1, 2}, ups == 2 only with stride 1 (got ups %d, stride %d)",
                  who, p->ups, p->stride);
    COMAT_REQUIRE(p->B >= 1 && p->Hin >= 1 && p->Win >= 1 && p->Cin >= 1 && p->Cout >= 1 && p->pad >= 0 && p->Hout >= 1 && p->Wout >= 1,
                  "%s: sizes must be positive", who);
    COMAT_REQUIRE((int64_t)p->Hin * p->ups + 2 * p->pad >= p->KH && (int64_t)p->Win * p->ups + 2 * p->pad >= p->KW &&
                      p->Hout == (p->Hin * p->ups + 2 * p->pad - p->KH) / p->stride + 1 &&
                      p->Wout == (p->Win * p->ups + 2 * p->pad - p->KW) / p->stride + 1,
                  "%s: Hout x Wout = %d x %d is not the output of this convolution", who, p->Hout, p->Wout);
    COMAT_REQUIRE((int64_t)p->B * p->Hout * p->Wout < (1ll << 31) && (int64_t)p->Cout * p->KH * p->KW * (p->Cin + 63) < (1ll << 31),
                  "%s: problem too large", who);
    return COMAT_OK;
}

}  // namespace

extern "C" int64_t comat_conv2d_wgrad_workspace_bytes(const comat_conv_wgrad_params* p) {
    if (!p || conv_wgrad_check(p, "comat_conv2d_wgrad_workspace_bytes") != COMAT_OK) return 0;
    if (p->in_dtype == COMAT_BF16 && p->Cin % 8 == 0 && p->Cout % 8 == 0) return comat_gemm2_conv_wgrad_ws_bytes(p);
    const int64_t K = (int64_t)p->B * p->Hout * p->Wout, nout = (int64_t)p->Cout * p->KH * p->KW * p->Cin;
    int64_t c = cdiv64(K, 4096);
    if (c > MAX_CHUNKS) c = MAX_CHUNKS;
    return c > 1 ? COMAT_WS_COUNTER_BYTES + c * nout * 4 : 0;
}

extern "C" int comat_conv2d_wgrad(const comat_conv_wgrad_params* p, void* stream) {
    const int rc = conv_wgrad_check(p, "comat_conv2d_wgrad");
    if (rc != COMAT_OK) return rc;
    if (comat_gemm2_try_conv_wgrad(p, stream)) {
        comat_note_gemm_kernel(6);
        return comat_check_launch("comat_conv2d_wgrad");
    }
    const int taps = p->KH * p->KW;
    const int64_t K = (int64_t)p->B * p->Hout * p->Wout, nout = (int64_t)p->Cout * taps * p->Cin;
    int cl = 1;
    while (cl < 64 && cl < p->Cin) cl *= 2;
    const int ci_chunks = (int)cdiv64(p->Cin, cl);
    // the partial sums live behind the ticket counters of the workspace (the pipelined kernels own those)
    float* part = p->ws ? (float*)p->ws + WS_COUNTERS : nullptr;
    const int nch = plan_chunks(K, 4096, nout, part, p->ws_bytes - COMAT_WS_COUNTER_BYTES);
    const int64_t per = cdiv64(K, nch);
    const ConvWgradGeom g = {p->B, p->Hin, p->Win, p->Cin, p->Hout, p->Wout, p->KW, p->stride, p->pad, p->ups};
    const dim3 grid((unsigned)((int64_t)p->Cout * taps * ci_chunks), (unsigned)nch);
    float* out = nch == 1 ? p->dW : part;
    if (p->in_dtype == COMAT_F32)
        hipLaunchKernelGGL(conv_wgrad_general_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)p->dY,
                           (const float*)p->X, out, g, p->Cout, taps, K, per, cl, ci_chunks, nch == 1);
    else
        hipLaunchKernelGGL(conv_wgrad_general_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)p->dY,
                           (const bf16_t*)p->X, out, g, p->Cout, taps, K, per, cl, ci_chunks, nch == 1);
    if (nch > 1)
        hipLaunchKernelGGL(partials_add_kernel, dim3((unsigned)cdiv64(nout, 256)), dim3(256), 0, (hipStream_t)stream, part, nch, nout,
                           p->dW, nout, (float*)nullptr);
    comat_note_gemm_kernel(7);
    return comat_check_launch("comat_conv2d_wgrad");
}

extern "C" int comat_colsum(const void* x, float* out, int64_t M, int32_t C, int64_t ld, int32_t dtype, float* ws, int64_t ws_bytes,
                            void* stream) {
    COMAT_REQUIRE(x && out, "comat_colsum: null operand");
    COMAT_REQUIRE(dtype_ok(dtype), "comat_colsum: x must be bf16 or fp32");
    COMAT_REQUIRE(M >= 1 && C >= 1 && ld >= C, "comat_colsum: M, C >= 1 and ld >= C (got M %lld, C %d, ld %lld)", (long long)M, C,
                  (long long)ld);
    const int nch = plan_chunks(M, 1024, C, ws, ws_bytes);
    const int64_t per = cdiv64(M, nch);
    const dim3 grid((unsigned)cdiv64(C, 64), (unsigned)nch);
    float* o = nch == 1 ? out : ws;
    if (dtype == COMAT_F32)
        hipLaunchKernelGGL(colsum_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, o, M, C, ld, per, nch == 1);
    else
        hipLaunchKernelGGL(colsum_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, o, M, C, ld, per, nch == 1);
    if (nch > 1)
        hipLaunchKernelGGL(partials_add_kernel, dim3((unsigned)cdiv64(C, 256)), dim3(256), 0, (hipStream_t)stream, ws, nch, (int64_t)C, out,
                           (int64_t)C, (float*)nullptr);
    return comat_check_launch("comat_colsum");
}

extern "C" int comat_groupnorm_bwd_affine(const void* dy, const void* x, const float* gamma, const float* beta, const float* stats,
                                          float* dgamma, float* dbeta, float* ws, int64_t ws_bytes, int32_t B, int64_t HW, int32_t C,
                                          int32_t G, int32_t silu, int32_t dtype, void* stream) {
    COMAT_REQUIRE(dy && x && gamma && beta && stats && dgamma && dbeta, "comat_groupnorm_bwd_affine: null operand");
    COMAT_REQUIRE(dtype_ok(dtype), "comat_groupnorm_bwd_affine: dy, x must be bf16 or fp32");
    COMAT_REQUIRE(B >= 1 && HW >= 1 && C >= 1 && G >= 1 && C % G == 0, "comat_groupnorm_bwd_affine: B, HW >= 1 and G must divide C");
    const int64_t M = (int64_t)B * HW;
    const int nch = plan_chunks(M, 1024, 2 * (int64_t)C, ws, ws_bytes);
    const int64_t per = cdiv64(M, nch);
    const dim3 grid((unsigned)cdiv64(C, 64), (unsigned)nch);
    float* o0 = nch == 1 ? dgamma : ws;
    if (dtype == COMAT_F32)
        hipLaunchKernelGGL(gn_affine_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)dy, (const float*)x, gamma, beta,
                           stats, o0, dbeta, M, HW, C, G, silu, per, nch == 1);
    else
        hipLaunchKernelGGL(gn_affine_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)x, gamma,
                           beta, stats, o0, dbeta, M, HW, C, G, silu, per, nch == 1);
    if (nch > 1)
        hipLaunchKernelGGL(partials_add_kernel, dim3((unsigned)cdiv64(2 * (int64_t)C, 256)), dim3(256), 0, (hipStream_t)stream, ws, nch,
                           2 * (int64_t)C, dgamma, (int64_t)C, dbeta);
    return comat_check_launch("comat_groupnorm_bwd_affine");
}

extern "C" int comat_layernorm_bwd_affine(const void* dy, const void* x, const float* stats, float* dgamma, float* dbeta, float* ws,
                                          int64_t ws_bytes, int64_t M, int32_t C, int32_t dtype, void* stream) {
    COMAT_REQUIRE(dy && x && stats && dgamma && dbeta, "comat_layernorm_bwd_affine: null operand");
    COMAT_REQUIRE(dtype_ok(dtype), "comat_layernorm_bwd_affine: dy, x must be bf16 or fp32");
    COMAT_REQUIRE(M >= 1 && C >= 1, "comat_layernorm_bwd_affine: M, C >= 1 (got M %lld, C %d)", (long long)M, C);
    // 256 rows per chunk: the UNet's norms are short and wide (8192 x 320 ... 128 x 1280) and a chunk is one block per 64 columns
    const int nch = plan_chunks(M, 256, 2 * (int64_t)C, ws, ws_bytes);
    const int64_t per = cdiv64(M, nch);
    const dim3 grid((unsigned)cdiv64(C, 64), (unsigned)nch);
    float* o0 = nch == 1 ? dgamma : ws;
    if (dtype == COMAT_F32)
        hipLaunchKernelGGL(ln_affine_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)dy, (const float*)x, stats, o0,
                           dbeta, M, C, per, nch == 1);
    else
        hipLaunchKernelGGL(ln_affine_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)x, stats,
                           o0, dbeta, M, C, per, nch == 1);
    if (nch > 1)
        hipLaunchKernelGGL(partials_add_kernel, dim3((unsigned)cdiv64(2 * (int64_t)C, 256)), dim3(256), 0, (hipStream_t)stream, ws, nch,
                           2 * (int64_t)C, dgamma, (int64_t)C, dbeta);
    return comat_check_launch("comat_layernorm_bwd_affine");
}

extern "C" int comat_colsum_batched(const void* x, float* out, int32_t B, int64_t M, int32_t C, int64_t ld, int32_t dtype, float* ws,
                                    int64_t ws_bytes, void* stream) {
    COMAT_REQUIRE(x && out, "comat_colsum_batched: null operand");
    COMAT_REQUIRE(dtype_ok(dtype), "comat_colsum_batched: x must be bf16 or fp32");
    COMAT_REQUIRE(B >= 1 && B <= 65535 && M >= 1 && C >= 1 && ld >= C,
                  "comat_colsum_batched: 1 <= B <= 65535, M, C >= 1 and ld >= C (got B %d, M %lld, C %d, ld %lld)", B, (long long)M, C,
                  (long long)ld);
    const int64_t n = (int64_t)B * C;
    const int nch = plan_chunks(M, 256, n, ws, ws_bytes);
    const int64_t per = cdiv64(M, nch);
    const dim3 grid((unsigned)cdiv64(C, 64), (unsigned)nch, (unsigned)B);
    float* o = nch == 1 ? out : ws;
    if (dtype == COMAT_F32)
        hipLaunchKernelGGL(colsum_batched_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, o, M, C, ld, per);
    else
        hipLaunchKernelGGL(colsum_batched_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, o, M, C, ld, per);
    if (nch > 1)
        hipLaunchKernelGGL(partials_set_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, ws, nch, n, out);
    return comat_check_launch("comat_colsum_batched");
}
