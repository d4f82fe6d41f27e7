// denoise.hip — the elementwise body of a noise-prediction fine-tune step: latent + noise + timestep -> UNet input
// (comat_denoise_prepare) and the MSE against the noise (comat_mse_fwd / _bwd).  Definitions: include/comat_hip.h.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int RT = 1024;  // lanes of the one block per sample of the MSE reduction (as eltwise.hip's rescaled guidance)

// four consecutive elements, one access: 16 bytes of fp32, 8 bytes of bf16
__device__ __forceinline__ void ld4(const float* p, float* v) {
    const float4 a = *(const float4*)p;
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
}
__device__ __forceinline__ void ld4(const bf16_t* p, float* v) {
    const uint2 u = *(const uint2*)p;
    v[0] = __uint_as_float(u.x << 16), v[1] = __uint_as_float(u.x & 0xffff0000u);
    v[2] = __uint_as_float(u.y << 16), v[3] = __uint_as_float(u.y & 0xffff0000u);
}
__device__ __forceinline__ void st4(float* p, const float* v) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void st4(bf16_t* p, const float* v) {
    uint2 u;
    u.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
    u.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
    *(uint2*)p = u;
}

// x0 of one element on the moments path: every operation its own fp32 rounding (the header's order); the clamp keeps a NaN
__device__ __forceinline__ float posterior(float mean, float logvar, float z, bool has_z, float scaling) {
#pragma clang fp contract(off)
    if (!has_z) return scaling * mean;
    const float lv = logvar < -30.0f ? -30.0f : (logvar > 20.0f ? 20.0f : logvar);
    const float sd = expf(0.5f * lv);
    return scaling * (mean + sd * z);
}
// comat_add_noise_fwd's rounding, read off its kernel's code: the product sb * noise rounded, then ONE fused multiply-add
__device__ __forceinline__ float noised(float sa, float x0, float sb, float nz) { return fmaf(sa, x0, __fmul_rn(sb, nz)); }

// grid (x, B): block row b is sample b; its blocks stride over the sample's P * C elements (VEC = 4: in fours, C % 4 == 0 keeps a
// four inside one pixel's channels).  Block x == 0 of a row also copies the sample's table rows.
template <typename TM, typename TX, int VEC>
__global__ __launch_bounds__(NT) void denoise_prepare_kernel(const TM* __restrict__ moments, const float* __restrict__ z,
                                                             const float* __restrict__ latents, const float* __restrict__ noise,
                                                             const int32_t* __restrict__ t, const float* __restrict__ sab,
                                                             const float* __restrict__ sinus, const float* __restrict__ wtab,
                                                             TX* __restrict__ xin, float* __restrict__ x0_out,
                                                             float* __restrict__ temb, float* __restrict__ w,
                                                             int32_t* __restrict__ oob, float scaling, int T, int64_t P, int C,
                                                             int C0) {
    const int b = blockIdx.y;
    const int tb = t[b];
    const int tc = tb < 0 ? 0 : (tb >= T ? T - 1 : tb);
    const float sa = sab[2 * tc], sb = sab[2 * tc + 1];
    const int64_t n = P * C, base = (int64_t)b * n;
    const bool has_z = z != nullptr;
    if (blockIdx.x == 0) {
        for (int j = threadIdx.x; j < C0; j += NT) temb[(int64_t)b * C0 + j] = sinus[(int64_t)tc * C0 + j];
        if (threadIdx.x == 0) {
            w[b] = wtab[tc];
            if (oob && tb != tc) oob[0] = 1;
        }
    }
    const int64_t items = n / VEC;
    for (int64_t it = (int64_t)blockIdx.x * NT + threadIdx.x; it < items; it += (int64_t)gridDim.x * NT) {
        const int64_t e = it * VEC, i = base + e;
        float x0[VEC], nz[VEC], o[VEC];
        if (moments) {
            const int64_t p = e / C;
            const int c = (int)(e - p * C);
            const TM* m = moments + ((int64_t)b * P + p) * 2 * C + c;
            float mean[VEC], lv[VEC], zz[VEC];
            if constexpr (VEC == 4) {
                ld4(m, mean);
                if (has_z) ld4(m + C, lv), ld4(z + i, zz);
            } else {
                mean[0] = ldf<TM>(m);
                if (has_z) lv[0] = ldf<TM>(m + C), zz[0] = z[i];
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) x0[k] = posterior(mean[k], has_z ? lv[k] : 0.f, has_z ? zz[k] : 0.f, has_z, scaling);
        } else {
            if constexpr (VEC == 4) ld4(latents + i, x0); else x0[0] = latents[i];
        }
        if constexpr (VEC == 4) ld4(noise + i, nz); else nz[0] = noise[i];
#pragma unroll
        for (int k = 0; k < VEC; ++k) o[k] = noised(sa, x0[k], sb, nz[k]);
        if constexpr (VEC == 4) {
            st4(xin + i, o);
            if (x0_out) st4(x0_out + i, x0);
        } else {
            stf<TX>(xin + i, o[0]);
            if (x0_out) x0_out[i] = x0[0];
        }
    }
}

// (pred - target)^2 with ONE rounding: difference and square in fp64 (the difference of two fp32 values is exact there unless
// their exponents lie more than 29 apart), rounded to fp32
__device__ __forceinline__ float sq_err(float p, float q) {
    const double d = (double)p - (double)q;
    return (float)(d * d);
}

// One block per sample.  Element i belongs to lane (i / 4) mod RT - the owner of its four whether the four is one access (VEC) or
// four; a lane adds its terms in ascending i, a wave's lanes meet in the butterfly, lane 0 of wave 0 adds the wave sums in order.
template <typename T, bool VEC>
__global__ __launch_bounds__(RT) void mse_fwd_kernel(const T* __restrict__ pred, const float* __restrict__ target,
                                                     float* __restrict__ per_sample, int64_t n) {
#pragma clang fp contract(off)
    __shared__ float sbuf[RT / 64];
    const int64_t base = (int64_t)blockIdx.x * n;
    const T* p = pred + base;
    const float* q = target + base;
    float acc = 0.f;
    for (int64_t i = (int64_t)threadIdx.x * 4; i < n; i += RT * 4) {
        if (VEC) {  // n % 4 == 0: the four is whole
            float a[4], c[4];
            ld4(p + i, a);
            ld4(q + i, c);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += sq_err(a[k], c[k]);
        } else {
            for (int k = 0; k < 4 && i + k < n; ++k) acc += sq_err(ldf<T>(p + i + k), q[i + k]);
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sbuf[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
#pragma unroll
        for (int wv = 0; wv < RT / 64; ++wv) s += sbuf[wv];
        per_sample[blockIdx.x] = s / (float)n;
    }
}

// loss = (1 / B) sum_b w_b per_sample[b] in index order: B is a batch size, one lane walks it
__global__ void mse_mean_kernel(const float* __restrict__ per_sample, const float* __restrict__ w, float* __restrict__ loss,
                                int B) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += w ? w[b] * per_sample[b] : per_sample[b];
    loss[0] = s / (float)B;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void mse_bwd_kernel(const T* __restrict__ pred, const float* __restrict__ target,
                                                     const float* __restrict__ w, const float* __restrict__ g,
                                                     T* __restrict__ dpred, int B, int64_t n) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const double gw = (double)(g ? g[0] : 1.0f) * (double)(w ? w[b] : 1.0f);
    const float c = (float)((gw * 2.0) / ((double)B * (double)n));
    const int64_t base = (int64_t)b * n;
    const int64_t items = VEC ? n / 4 : n;
    for (int64_t it = (int64_t)blockIdx.x * NT + threadIdx.x; it < items; it += (int64_t)gridDim.x * NT) {
        if (VEC) {
            const int64_t i = base + it * 4;
            float a[4], q[4], o[4];
            ld4(pred + i, a);
            ld4(target + i, q);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = c * (a[k] - q[k]);
            st4(dpred + i, o);
        } else {
            const int64_t i = base + it;
            stf<T>(dpred + i, c * (ldf<T>(pred + i) - target[i]));
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int comat_denoise_prepare(const void* moments, const float* z, const float* latents, const float* noise,
                                     const int32_t* t, const float* sab, const float* sinus, const float* wtab, void* xin,
                                     float* x0_out, float* temb, float* w, int32_t* oob, float scaling, int32_t T, int32_t B,
                                     int64_t P, int32_t C, int32_t C0, int32_t moments_dtype, int32_t xin_dtype, void* stream) {
    COMAT_REQUIRE((moments != nullptr) != (latents != nullptr),
                  "comat_denoise_prepare: exactly one of moments and latents (got %s)", moments ? "both" : "neither");
    COMAT_REQUIRE(!(latents && z), "comat_denoise_prepare: z goes with moments, not with latents");
    COMAT_REQUIRE(noise && t && sab && sinus && wtab && xin && temb && w, "comat_denoise_prepare: null pointer");
    COMAT_REQUIRE(B > 0 && P > 0 && C > 0 && C0 > 0 && T > 0,
                  "comat_denoise_prepare: bad shape (B %d, P %lld, C %d, C0 %d, T %d must be positive)", B, (long long)P, C, C0, T);
    COMAT_REQUIRE(B <= 65535, "comat_denoise_prepare: B = %d, at most 65535 samples a launch", B);
    COMAT_REQUIRE(P <= INT32_MAX / C, "comat_denoise_prepare: bad shape (P * C beyond 2^31 - 1)");
    COMAT_REQUIRE(dtype_ok(xin_dtype) && (!moments || dtype_ok(moments_dtype)), "comat_denoise_prepare: bad dtype");
    const bool vec = C % 4 == 0 && aligned16(moments) && aligned16(z) && aligned16(latents) && aligned16(noise) && aligned16(xin) &&
                     aligned16(x0_out);
    const int64_t items = P * C / (vec ? 4 : 1);
    const dim3 grid(grid_1d(items, NT, 1024), (unsigned)B), block(NT);
#define COMAT_PREPARE(TM, TX, VEC)                                                                                            \
    hipLaunchKernelGGL((denoise_prepare_kernel<TM, TX, VEC>), grid, block, 0, ST, (const TM*)moments, z, latents, noise, t, sab, \
                       sinus, wtab, (TX*)xin, x0_out, temb, w, oob, scaling, T, P, C, C0)
#define COMAT_PREPARE_X(TM)                                                              \
    do {                                                                                 \
        if (xin_dtype == COMAT_BF16) {                                                   \
            if (vec) COMAT_PREPARE(TM, bf16_t, 4); else COMAT_PREPARE(TM, bf16_t, 1);    \
        } else {                                                                         \
            if (vec) COMAT_PREPARE(TM, float, 4); else COMAT_PREPARE(TM, float, 1);      \
        }                                                                                \
    } while (0)
    if (moments && moments_dtype == COMAT_BF16) COMAT_PREPARE_X(bf16_t); else COMAT_PREPARE_X(float);
#undef COMAT_PREPARE_X
#undef COMAT_PREPARE
    return comat_check_launch("comat_denoise_prepare");
}

extern "C" int comat_mse_fwd(const void* pred, const float* target, const float* w, float* per_sample, float* loss, int32_t B,
                             int64_t n, int32_t pred_dtype, void* stream) {
    COMAT_REQUIRE(pred && target && per_sample && loss, "comat_mse_fwd: null pointer");
    COMAT_REQUIRE(B > 0 && n > 0, "comat_mse_fwd: bad shape (B %d, n %lld must be positive)", B, (long long)n);
    COMAT_REQUIRE(B <= 65535, "comat_mse_fwd: B = %d, at most 65535 samples a launch", B);
    COMAT_REQUIRE(dtype_ok(pred_dtype), "comat_mse_fwd: bad dtype");
    const bool vec = n % 4 == 0 && aligned16(pred) && aligned16(target);
#define COMAT_MSE_FWD(T, VEC) \
    hipLaunchKernelGGL((mse_fwd_kernel<T, VEC>), dim3(B), dim3(RT), 0, ST, (const T*)pred, target, per_sample, n)
    if (pred_dtype == COMAT_BF16) {
        if (vec) COMAT_MSE_FWD(bf16_t, true); else COMAT_MSE_FWD(bf16_t, false);
    } else {
        if (vec) COMAT_MSE_FWD(float, true); else COMAT_MSE_FWD(float, false);
    }
#undef COMAT_MSE_FWD
    hipLaunchKernelGGL(mse_mean_kernel, dim3(1), dim3(64), 0, ST, per_sample, w, loss, B);
    return comat_check_launch("comat_mse_fwd");
}

extern "C" int comat_mse_bwd(const void* pred, const float* target, const float* w, const float* g, void* dpred, int32_t B,
                             int64_t n, int32_t pred_dtype, void* stream) {
    COMAT_REQUIRE(pred && target && dpred, "comat_mse_bwd: null pointer");
    COMAT_REQUIRE(B > 0 && n > 0, "comat_mse_bwd: bad shape (B %d, n %lld must be positive)", B, (long long)n);
    COMAT_REQUIRE(B <= 65535, "comat_mse_bwd: B = %d, at most 65535 samples a launch", B);
    COMAT_REQUIRE(dtype_ok(pred_dtype), "comat_mse_bwd: bad dtype");
    const bool vec = n % 4 == 0 && aligned16(pred) && aligned16(target) && aligned16(dpred);
    const dim3 grid(grid_1d(vec ? n / 4 : n, NT, 1024), (unsigned)B), block(NT);
#define COMAT_MSE_BWD(T, VEC) \
    hipLaunchKernelGGL((mse_bwd_kernel<T, VEC>), grid, block, 0, ST, (const T*)pred, target, w, g, (T*)dpred, B, n)
    if (pred_dtype == COMAT_BF16) {
        if (vec) COMAT_MSE_BWD(bf16_t, true); else COMAT_MSE_BWD(bf16_t, false);
    } else {
        if (vec) COMAT_MSE_BWD(float, true); else COMAT_MSE_BWD(float, false);
    }
#undef COMAT_MSE_BWD
    return comat_check_launch("comat_mse_bwd");
}
