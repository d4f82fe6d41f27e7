// eltwise.hip — HBM-bound elementwise / data-movement kernels of the CoMat step (grid-stride, runtime dtype).
#include "common.h"

namespace {

constexpr int NT = 256;
#define GRID_STRIDE(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < (n); i += (int64_t)gridDim.x * NT)

__global__ __launch_bounds__(NT) void unary_kernel(int op, const void* __restrict__ x, void* __restrict__ y, int64_t n,
                                                   float p0, float p1, int xdt, int ydt) {
    GRID_STRIDE(i, n) {
        float v = ld_dt(x, i, xdt);
        if (op == COMAT_UN_SILU) v = silu_f(v);
        else if (op == COMAT_UN_GELU) v = gelu_f(v);
        else if (op == COMAT_UN_AFFINE) v = p0 * v + p1;
        else if (op == COMAT_UN_QUICK_GELU) v = quick_gelu_f(v);
        st_dt(y, i, v, ydt);
    }
}

__global__ __launch_bounds__(NT) void unary_bwd_kernel(int op, const void* __restrict__ dy, const void* __restrict__ x,
                                                       void* __restrict__ dx, int64_t n, int dt) {
    GRID_STRIDE(i, n) {
        const float v = ld_dt(x, i, dt);
        float g = ld_dt(dy, i, dt);
        if (op == COMAT_UN_SILU) g *= silu_grad_f(v);
        else if (op == COMAT_UN_GELU) g *= gelu_grad_f(v);
        else if (op == COMAT_UN_QUICK_GELU) g *= quick_gelu_grad_f(v);
        st_dt(dx, i, g, dt);
    }
}

__global__ __launch_bounds__(NT) void axpby_kernel(float a, const void* __restrict__ x, float b,
                                                   const void* __restrict__ y, void* __restrict__ out, int64_t n,
                                                   int xdt, int ydt, int odt) {
    GRID_STRIDE(i, n) {
        float v = a * ld_dt(x, i, xdt);
        if (y) v += b * ld_dt(y, i, ydt);
        st_dt(out, i, v, odt);
    }
}

__global__ __launch_bounds__(NT) void geglu_fwd_kernel(const void* __restrict__ x, void* __restrict__ y, int64_t M,
                                                       int D, int dt) {
    const int64_t n = M * D;
    GRID_STRIDE(i, n) {
        const int64_t m = i / D;
        const int d = (int)(i - m * D);
        const float a = ld_dt(x, m * 2 * D + d, dt), g = ld_dt(x, m * 2 * D + D + d, dt);
        st_dt(y, i, a * gelu_f(g), dt);
    }
}

__global__ __launch_bounds__(NT) void geglu_bwd_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                                       void* __restrict__ dx, int64_t M, int D, int dt) {
    const int64_t n = M * D;
    GRID_STRIDE(i, n) {
        const int64_t m = i / D;
        const int d = (int)(i - m * D);
        const float a = ld_dt(x, m * 2 * D + d, dt), g = ld_dt(x, m * 2 * D + D + d, dt);
        const float go = ld_dt(dy, i, dt);
        st_dt(dx, m * 2 * D + d, go * gelu_f(g), dt);
        st_dt(dx, m * 2 * D + D + d, go * a * gelu_grad_f(g), dt);
    }
}

// GEGLU on the INTERLEAVED layout of the fused projection (comat_gemm, epi2): every 32 columns of x [M, 2 D] hold 16 value
// channels followed by their 16 gate channels, so that one lane of the GEMM epilogue owns both halves of 8 channels.
// Work item = 8 channels of one row: 16-byte accesses (bf16), 2 x 16 (fp32).
template <typename T> struct V8;
template <> struct V8<bf16_t> {
    uint4 u;
    __device__ __forceinline__ void load(const bf16_t* p) { u = *(const uint4*)p; }
    __device__ __forceinline__ void store(bf16_t* p) const { *(uint4*)p = u; }
    __device__ __forceinline__ float get(int e) const { return bf16_to_f32(((const bf16_t*)&u)[e]); }
    __device__ __forceinline__ void set(int e, float v) { ((bf16_t*)&u)[e] = f32_to_bf16(v); }
};
template <> struct V8<float> {
    float v[8];  // (one array: indexing past a float4 member into its neighbour was undefined behaviour - ADVICE r4)
    __device__ __forceinline__ void load(const float* p) {
        const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    __device__ __forceinline__ void store(float* p) const {
        *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    __device__ __forceinline__ float get(int e) const { return v[e]; }
    __device__ __forceinline__ void set(int e, float x) { v[e] = x; }
};

template <typename T>
__global__ __launch_bounds__(NT) void geglu_il_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t M, int D) {
    const int D8 = D / 8;
    const int64_t n = M * D8;
    GRID_STRIDE(i, n) {
        const int64_t m = i / D8;
        const int c8 = (int)(i - m * D8);           // channels 8 c8 .. + 8
        const int col = (c8 >> 1) * 32 + (c8 & 1) * 8;  // their value columns; the gate columns are 16 further
        V8<T> a, g, o;
        a.load(x + m * 2 * D + col);
        g.load(x + m * 2 * D + col + 16);
#pragma unroll
        for (int e = 0; e < 8; ++e) o.set(e, a.get(e) * gelu_f(g.get(e)));
        o.store(y + m * D + c8 * 8);
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void geglu_il_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, T* __restrict__ dx,
                                                          int64_t M, int D) {
    const int D8 = D / 8;
    const int64_t n = M * D8;
    GRID_STRIDE(i, n) {
        const int64_t m = i / D8;
        const int c8 = (int)(i - m * D8);
        const int col = (c8 >> 1) * 32 + (c8 & 1) * 8;
        V8<T> a, g, go, da, dg;
        a.load(x + m * 2 * D + col);
        g.load(x + m * 2 * D + col + 16);
        go.load(dy + m * D + c8 * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            da.set(e, go.get(e) * gelu_f(g.get(e)));
            dg.set(e, go.get(e) * a.get(e) * gelu_grad_f(g.get(e)));
        }
        da.store(dx + m * 2 * D + col);
        dg.store(dx + m * 2 * D + col + 16);
    }
}

__global__ __launch_bounds__(NT) void copy2d_kernel(const void* __restrict__ src, int64_t lds_, void* __restrict__ dst,
                                                    int64_t ldd, int64_t rows, int64_t cols, int sdt, int ddt) {
    const int64_t n = rows * cols;
    GRID_STRIDE(i, n) {
        const int64_t r = i / cols, c = i - r * cols;
        st_dt(dst, r * ldd + c, ld_dt(src, r * lds_ + c, sdt), ddt);
    }
}

// two strided 2-D copies in ONE launch, 16 bytes per thread and step: the channel concat of a skip connection (out[:, :Ca] = a,
// out[:, Ca:] = b) and its backward split - twice per up-path ResnetBlock and direction (336 two-copy pairs per C2 step)
struct Copy2dPair {
    const char* src[2];
    char* dst[2];
    int64_t lds[2], ldd[2];  // bytes between rows
    int vpr[2];              // 16-byte vectors per row
};
__global__ __launch_bounds__(NT) void copy2d_pair_kernel(Copy2dPair p, int64_t rows) {
    const int vt = p.vpr[0] + p.vpr[1];
    const int64_t n = rows * vt;
    GRID_STRIDE(i, n) {
        const int64_t r = i / vt;
        int v = (int)(i - r * vt);
        const int w = v >= p.vpr[0] ? 1 : 0;
        v -= w * p.vpr[0];
        *(uint4*)(p.dst[w] + r * p.ldd[w] + (int64_t)v * 16) = *(const uint4*)(p.src[w] + r * p.lds[w] + (int64_t)v * 16);
    }
}

__global__ __launch_bounds__(NT) void add_rowvec_kernel(const void* __restrict__ x, const void* __restrict__ v,
                                                        void* __restrict__ out, int64_t rows, int64_t cols, int dt) {
    const int64_t n = rows * cols;
    GRID_STRIDE(i, n) { st_dt(out, i, ld_dt(x, i, dt) + ld_dt(v, i % cols, dt), dt); }
}

__global__ __launch_bounds__(NT) void sumpool2x2_kernel(const void* __restrict__ x, void* __restrict__ y, int B, int H,
                                                        int W, int C, int dt) {
    const int64_t n = (int64_t)B * H * W * C;
    GRID_STRIDE(i, n) {
        const int c = (int)(i % C);
        int64_t t = i / C;
        const int w = (int)(t % W);
        t /= W;
        const int h = (int)(t % H);
        const int64_t b = t / H;
        const int64_t W2 = 2 * (int64_t)W;
        const int64_t base = ((b * 2 * H + 2 * h) * W2 + 2 * w) * C + c;
        const float v = ld_dt(x, base, dt) + ld_dt(x, base + C, dt) + ld_dt(x, base + W2 * C, dt) +
                        ld_dt(x, base + W2 * C + C, dt);
        st_dt(y, i, v, dt);
    }
}

__global__ __launch_bounds__(NT) void permute_kernel(const void* __restrict__ x, void* __restrict__ y, int B, int C,
                                                     int H, int W, int to_nhwc, int xdt, int ydt) {
    const int64_t n = (int64_t)B * C * H * W;
    GRID_STRIDE(i, n) {  // i indexes the OUTPUT
        if (to_nhwc) {
            const int c = (int)(i % C);
            int64_t t = i / C;
            const int w = (int)(t % W);
            t /= W;
            const int h = (int)(t % H);
            const int64_t b = t / H;
            st_dt(y, i, ld_dt(x, ((b * C + c) * H + h) * W + w, xdt), ydt);
        } else {
            const int w = (int)(i % W);
            int64_t t = i / W;
            const int h = (int)(t % H);
            t /= H;
            const int c = (int)(t % C);
            const int64_t b = t / C;
            st_dt(y, i, ld_dt(x, ((b * H + h) * W + w) * C + c, xdt), ydt);
        }
    }
}

__global__ __launch_bounds__(NT) void cfg_ddpm_fwd_kernel(const float* __restrict__ x, const void* __restrict__ eps2,
                                                          const float* __restrict__ z, float* __restrict__ xp,
                                                          int64_t n, float s, float cx, float ce, float sigma,
                                                          int edt) {
    GRID_STRIDE(i, n) {
        const float eu = ld_dt(eps2, i, edt), ec = ld_dt(eps2, n + i, edt);
        const float eps = eu + s * (ec - eu);
        float v = cx * x[i] + ce * eps;
        if (z) v += sigma * z[i];
        xp[i] = v;
    }
}

__global__ __launch_bounds__(NT) void cfg_ddpm_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx,
                                                          void* __restrict__ deps2, int64_t n, float s, float cx,
                                                          float ce, int edt) {
    GRID_STRIDE(i, n) {
        const float gi = g[i];
        if (dx) dx[i] = cx * gi;
        st_dt(deps2, i, ce * (1.0f - s) * gi, edt);
        st_dt(deps2, n + i, ce * s * gi, edt);
    }
}

// ---- rescaled guidance + DDPM step (comat_cfg_rescale_ddpm_fwd / _bwd) --------------------------------------------
// One block of 1 024 lanes per sample: the op sits between two UNet calls (latency, not bandwidth: <= 0.5 MB per operand), so
// it is ONE launch - per-sample statistics, then the apply pass, which reads the two predictions again from L2 (the block
// itself has just pulled them in).  Keeping the guided noise of a 65 536-value sample in registers between the passes was
// tried: 64 values per lane next to the loads in flight do not fit the 128 registers of a 1 024-lane block, the compiler
// spilled 44-80 of them to scratch memory - slower than the L2 hit it was meant to save.
constexpr int RT = 1024;  // lanes per block

template <typename T> __device__ __forceinline__ void ld4(const T* p, float* v);
template <> __device__ __forceinline__ void ld4<float>(const float* p, float* v) {
    const float4 a = *(const float4*)p;
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
template <> __device__ __forceinline__ void ld4<bf16_t>(const bf16_t* p, float* v) {
    const uint2 u = *(const uint2*)p;
    v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
    v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
}
template <typename T> __device__ __forceinline__ void st4(T* p, const float* v);
template <> __device__ __forceinline__ void st4<float>(float* p, const float* v) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void st4<bf16_t>(bf16_t* p, const float* v) {
    uint2 u;
    u.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
    u.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
    *(uint2*)p = u;
}

// cx * x + ce * eps as cfg_ddpm_fwd_kernel computes it: the compiler pairs its two products into ONE packed multiply and adds
// them (two rounded products, no fused multiply-add); in the surroundings of the rescaled kernel it would contract one of them
// into the sum, and phi = 0 would no longer give the bits of the plain step.  (tests/test_cfg_rescale.py compares the two.)
__device__ __forceinline__ float ddpm_mix(float cx, float x, float ce, float eps) {
#pragma clang fp contract(off)
    return cx * x + ce * eps;
}

// block-wide sums of NV values per lane for blockDim.x == RT (16 waves), in a fixed order: butterfly inside a wave, then every
// lane adds the 16 wave results in wave order.  sbuf: >= 16 * NV floats.  All lanes get the same bits.
template <int NV> __device__ __forceinline__ void block_sum_rt(float* v, float* sbuf) {
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = wave_sum(v[j]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) sbuf[(threadIdx.x >> 6) * NV + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < RT / 64; ++w) a += sbuf[w * NV + j];
        v[j] = a;
    }
}

template <typename T>
__global__ __launch_bounds__(RT) void cfg_rescale_ddpm_fwd_kernel(const float* __restrict__ x, const T* __restrict__ eps2,
                                                                  const float* __restrict__ z, float* __restrict__ xp,
                                                                  int64_t n, int64_t P, float s, float cx, float ce,
                                                                  float sigma, float phi, float* __restrict__ stats) {
    __shared__ float sbuf[(RT / 64) * 4];
    const int64_t base = (int64_t)blockIdx.x * P;
    const T* eu = eps2 + base;
    const T* ec = eps2 + n + base;
    // one-pass sums of (v - shift), (v - shift)^2 with the sample's first value as the shift: no cancellation when the
    // predictions carry a mean offset
    const float su = ldf<T>(eu), kt = ldf<T>(ec);
    const float kc = su + s * (kt - su);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = (int64_t)threadIdx.x * 4; i < P; i += RT * 4) {
        float u[4], t[4];
        ld4<T>(eu + i, u);
        ld4<T>(ec + i, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ev = u[j] + s * (t[j] - u[j]);
            const float dt_ = t[j] - kt, dc = ev - kc;
            acc[0] += dt_; acc[1] += dt_ * dt_; acc[2] += dc; acc[3] += dc * dc;
        }
    }
    block_sum_rt<4>(acc, sbuf);
    const float inv_p = 1.0f / (float)P;
    const float mu_t = kt + acc[0] * inv_p, V_t = acc[1] - acc[0] * acc[0] * inv_p;
    const float mu_c = kc + acc[2] * inv_p, V_c = acc[3] - acc[2] * acc[2] * inv_p;
    const float r = sqrtf(V_t / V_c);  // std(e_c) / std(e): the n - 1 of torch.std cancels; V_c == 0 -> non-finite, not clamped
    const float k = phi * r + (1.0f - phi);
    if (threadIdx.x == 0) {
        float* st = stats + (int64_t)blockIdx.x * 4;
        st[0] = mu_t; st[1] = V_t; st[2] = mu_c; st[3] = V_c;
    }
    // apply: the operations of cfg_ddpm_fwd_kernel with eps = k * e (phi = 0: k == 1, the same bits)
    for (int64_t i = (int64_t)threadIdx.x * 4; i < P; i += RT * 4) {
        float u[4], t[4], xv[4], zv[4], o[4];
        ld4<T>(eu + i, u);
        ld4<T>(ec + i, t);
        ld4<float>(x + base + i, xv);
        if (z) ld4<float>(z + base + i, zv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ev = u[j] + s * (t[j] - u[j]);
            float v = ddpm_mix(cx, xv[j], ce, k * ev);
            if (z) v += sigma * zv[j];
            o[j] = v;
        }
        st4<float>(xp + base + i, o);
    }
}

template <typename T>
__global__ __launch_bounds__(RT) void cfg_rescale_ddpm_bwd_kernel(const float* __restrict__ g, const T* __restrict__ eps2,
                                                                  const float* __restrict__ stats, float* __restrict__ dx,
                                                                  T* __restrict__ deps2, int64_t n, int64_t P, float s,
                                                                  float cx, float ce, float phi) {
    __shared__ float sbuf[RT / 64];
    const int64_t base = (int64_t)blockIdx.x * P;
    const T* eu = eps2 + base;
    const T* ec = eps2 + n + base;
    const float* st = stats + (int64_t)blockIdx.x * 4;
    const float mu_t = st[0], V_t = st[1], mu_c = st[2], V_c = st[3];
    const float r = sqrtf(V_t / V_c);
    const float k = phi * r + (1.0f - phi);
    float D = 0.f;  // sum_i (ce g_i) e_i = dL/dk
    for (int64_t i = (int64_t)threadIdx.x * 4; i < P; i += RT * 4) {
        float u[4], t[4], gv[4];
        ld4<T>(eu + i, u);
        ld4<T>(ec + i, t);
        ld4<float>(g + base + i, gv);
#pragma unroll
        for (int j = 0; j < 4; ++j) D += (ce * gv[j]) * (u[j] + s * (t[j] - u[j]));
    }
    block_sum_rt<1>(&D, sbuf);
    const float w = D * phi * r;
    const float A = w / V_c, Bt = w / V_t;
    // the coefficients of cfg_ddpm_bwd_kernel, formed the same way (phi = 0: k == 1 and A == Bt == 0, the same bits)
    const float c1 = ce * (1.0f - s), c2 = ce * s;
    for (int64_t i = (int64_t)threadIdx.x * 4; i < P; i += RT * 4) {
        float u[4], t[4], gv[4], du[4], dc[4];
        ld4<T>(eu + i, u);
        ld4<T>(ec + i, t);
        ld4<float>(g + base + i, gv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ev = u[j] + s * (t[j] - u[j]);
            const float q = A * (ev - mu_c);  // what the statistics of e take out of de
            du[j] = k * (c1 * gv[j]) - (1.0f - s) * q;
            dc[j] = k * (c2 * gv[j]) - s * q + Bt * (t[j] - mu_t);
        }
        st4<T>(deps2 + base + i, du);
        st4<T>(deps2 + n + base + i, dc);
        if (dx) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = cx * gv[j];
            st4<float>(dx + base + i, o);
        }
    }
}

// ---- guidance on or off + DDPM step with x_prev and / or x0 (comat_ddpm_step2_fwd / _bwd) ------------------------------------
// The rescaled kernels above with three more degrees of freedom: HALVES = 1 (eps is the prediction itself), a second output
// x0 = px x + pe k e next to x_prev, and phi == 0 without a statistics pass.  phi > 0: one block per sample, as above.  phi == 0:
// nothing is per sample, the blocks share the n values in vectors of 4.  Every vector [i, i + 4) lies below `hi` because
// per_sample (and with it n) is a multiple of 4.
struct Span {
    int64_t lo, hi, stride;
};
__device__ __forceinline__ Span step2_span(bool per_sample_blocks, int64_t n, int64_t P) {
    Span r;
    if (per_sample_blocks) {
        r.lo = (int64_t)blockIdx.x * P + (int64_t)threadIdx.x * 4;
        r.hi = ((int64_t)blockIdx.x + 1) * P;
        r.stride = (int64_t)RT * 4;
    } else {
        r.lo = ((int64_t)blockIdx.x * RT + threadIdx.x) * 4;
        r.hi = n;
        r.stride = (int64_t)gridDim.x * RT * 4;
    }
    return r;
}

template <typename T, int HALVES>
__global__ __launch_bounds__(RT) void ddpm_step2_fwd_kernel(const float* __restrict__ x, const T* __restrict__ eps,
                                                            const float* __restrict__ z, float* __restrict__ xp,
                                                            float* __restrict__ x0, int64_t n, int64_t P, float s, float cx,
                                                            float ce, float sigma, float px, float pe, float phi,
                                                            float* __restrict__ stats) {
    __shared__ float sbuf[(RT / 64) * 4];
    const T* eu = eps;
    const T* ec = eps + (HALVES == 2 ? n : 0);
    float k = 1.0f;
    if (HALVES == 2 && phi > 0.f) {  // the statistics pass of cfg_rescale_ddpm_fwd_kernel, operation for operation
        const int64_t base = (int64_t)blockIdx.x * P;
        const float su = ldf<T>(eu + base), kt = ldf<T>(ec + base);
        const float kc = su + s * (kt - su);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int64_t i = (int64_t)threadIdx.x * 4; i < P; i += RT * 4) {
            float u[4], t[4];
            ld4<T>(eu + base + i, u);
            ld4<T>(ec + base + i, t);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float ev = u[j] + s * (t[j] - u[j]);
                const float dt_ = t[j] - kt, dc = ev - kc;
                acc[0] += dt_; acc[1] += dt_ * dt_; acc[2] += dc; acc[3] += dc * dc;
            }
        }
        block_sum_rt<4>(acc, sbuf);
        const float inv_p = 1.0f / (float)P;
        const float mu_t = kt + acc[0] * inv_p, V_t = acc[1] - acc[0] * acc[0] * inv_p;
        const float mu_c = kc + acc[2] * inv_p, V_c = acc[3] - acc[2] * acc[2] * inv_p;
        const float r = sqrtf(V_t / V_c);
        k = phi * r + (1.0f - phi);
        if (threadIdx.x == 0) {
            float* st = stats + (int64_t)blockIdx.x * 4;
            st[0] = mu_t; st[1] = V_t; st[2] = mu_c; st[3] = V_c;
        }
    }
    const Span sp = step2_span(HALVES == 2 && phi > 0.f, n, P);
    for (int64_t i = sp.lo; i < sp.hi; i += sp.stride) {
        float u[4], t[4], xv[4], zv[4], o[4], q[4];
        ld4<T>(eu + i, u);
        if (HALVES == 2) ld4<T>(ec + i, t);
        ld4<float>(x + i, xv);
        if (z && xp) ld4<float>(z + i, zv);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ev = HALVES == 2 ? u[j] + s * (t[j] - u[j]) : u[j];
            const float ke = k * ev;  // one scaled noise for both outputs
            float v = ddpm_mix(cx, xv[j], ce, ke);
            if (z && xp) v += sigma * zv[j];
            o[j] = v;
            q[j] = ddpm_mix(px, xv[j], pe, ke);
        }
        if (xp) st4<float>(xp + i, o);
        if (x0) st4<float>(x0 + i, q);
    }
}

// the gradients of the two outputs, 4 values each; one that is not there (NULL) counts as zero
__device__ __forceinline__ void ld4_or_zero(const float* p, int64_t i, float* v) {
    if (p) {
        ld4<float>(p + i, v);
    } else {
        v[0] = v[1] = v[2] = v[3] = 0.f;
    }
}

template <typename T, int HALVES>
__global__ __launch_bounds__(RT) void ddpm_step2_bwd_kernel(const float* __restrict__ gp, const float* __restrict__ gx,
                                                            const T* __restrict__ eps, const float* __restrict__ stats,
                                                            float* __restrict__ dx, T* __restrict__ deps, int64_t n, int64_t P,
                                                            float s, float cx, float ce, float px, float pe, float phi) {
    __shared__ float sbuf[RT / 64];
    const bool rescaled = HALVES == 2 && phi > 0.f && deps != nullptr;
    const T* eu = eps;
    const T* ec = eps + (HALVES == 2 ? n : 0);
    float k = 1.0f, A = 0.f, Bt = 0.f, mu_t = 0.f, mu_c = 0.f;
    if (rescaled) {
        const int64_t base = (int64_t)blockIdx.x * P;
        const float* st = stats + (int64_t)blockIdx.x * 4;
        mu_t = st[0];
        mu_c = st[2];
        const float V_t = st[1], V_c = st[3];
        const float r = sqrtf(V_t / V_c);
        k = phi * r + (1.0f - phi);
        float D = 0.f;  // sum_i d_i e_i = dL/dk
        for (int64_t i = (int64_t)threadIdx.x * 4; i < P; i += RT * 4) {
            float u[4], t[4], a[4], b[4];
            ld4<T>(eu + base + i, u);
            ld4<T>(ec + base + i, t);
            ld4_or_zero(gp, base + i, a);
            ld4_or_zero(gx, base + i, b);
#pragma unroll
            for (int j = 0; j < 4; ++j) D += ddpm_mix(ce, a[j], pe, b[j]) * (u[j] + s * (t[j] - u[j]));
        }
        block_sum_rt<1>(&D, sbuf);
        const float w = D * phi * r;
        A = w / V_c;
        Bt = w / V_t;
    }
    const Span sp = step2_span(rescaled, n, P);
    for (int64_t i = sp.lo; i < sp.hi; i += sp.stride) {
        float u[4], t[4], a[4], b[4], du[4], dc[4], o[4];
        ld4_or_zero(gp, i, a);
        ld4_or_zero(gx, i, b);
        if (rescaled) {
            ld4<T>(eu + i, u);
            ld4<T>(ec + i, t);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = ddpm_mix(ce, a[j], pe, b[j]);  // d = ce g_prev + pe g_x0: two rounded products and a sum
            o[j] = ddpm_mix(cx, a[j], px, b[j]);
            if (HALVES == 1) {
                du[j] = d;
            } else if (rescaled) {
                const float ev = u[j] + s * (t[j] - u[j]);
                const float de = k * d - A * (ev - mu_c);
                du[j] = (1.0f - s) * de;
                dc[j] = s * de + Bt * (t[j] - mu_t);
            } else {
                du[j] = (1.0f - s) * d;
                dc[j] = s * d;
            }
        }
        if (deps) {
            st4<T>(deps + i, du);
            if (HALVES == 2) st4<T>(deps + n + i, dc);
        }
        if (dx) st4<float>(dx + i, o);
    }
}

// re-noising in front of the extra trained call of `double_laststep`: noisy = sa x + sb noise in fp32 and `copies` stacked
// copies of it in the compute dtype (the UNet input) in one pass
__global__ __launch_bounds__(NT) void add_noise_fwd_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                           float* __restrict__ noisy, void* __restrict__ xin, int64_t n,
                                                           float sa, float sb, int copies, int xdt) {
    GRID_STRIDE(i, n) {
        const float v = sa * x[i] + sb * noise[i];
        noisy[i] = v;
        st_dt(xin, i, v, xdt);
        if (copies == 2) st_dt(xin, n + i, v, xdt);
    }
}

// Batched transpose + cast of many small matrices in one launch: block b handles the 32x32 tile described by
// tiles[b] = (src_off, dst_off, rows, cols, r0, c0): dst[dst_off + c*rows + r] = src[src_off + r*cols + c].
__global__ __launch_bounds__(NT) void transpose_tiles_kernel(const float* __restrict__ src, void* __restrict__ dst,
                                                             const int64_t* __restrict__ tiles, int out_dt) {
    __shared__ float tile[32][33];
    const int64_t* d = tiles + (int64_t)blockIdx.x * 6;
    const int64_t so = d[0], dof = d[1], rows = d[2], cols = d[3], r0 = d[4], c0 = d[5];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int j = 0; j < 32; j += NT / 32) {
        const int64_t r = r0 + ty + j, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + j][tx] = src[so + r * cols + c];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 32; j += NT / 32) {
        const int64_t c = c0 + ty + j, r = r0 + tx;
        if (r < rows && c < cols) st_dt(dst, dof + c * rows + r, tile[tx][ty + j], out_dt);
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int comat_unary(int32_t op, const void* x, void* y, int64_t n, float p0, float p1, int32_t x_dtype,
                           int32_t y_dtype, void* stream) {
    COMAT_REQUIRE(x && y && n > 0, "comat_unary: bad args");
    COMAT_REQUIRE(op >= 0 && op <= COMAT_UN_QUICK_GELU, "comat_unary: bad op %d", op);
    COMAT_REQUIRE(dtype_ok(x_dtype) && dtype_ok(y_dtype), "comat_unary: bad dtype");
    hipLaunchKernelGGL(unary_kernel, dim3(grid_1d(n, NT)), dim3(NT), 0, ST, op, x, y, n, p0, p1, x_dtype, y_dtype);
    return comat_check_launch("comat_unary");
}

extern "C" int comat_unary_bwd(int32_t op, const void* dy, const void* x, void* dx, int64_t n, int32_t dtype,
                               void* stream) {
    COMAT_REQUIRE(dy && x && dx && n > 0, "comat_unary_bwd: bad args");
    COMAT_REQUIRE(op == COMAT_UN_SILU || op == COMAT_UN_GELU || op == COMAT_UN_QUICK_GELU, "comat_unary_bwd: bad op %d", op);
    COMAT_REQUIRE(dtype_ok(dtype), "comat_unary_bwd: bad dtype");
    hipLaunchKernelGGL(unary_bwd_kernel, dim3(grid_1d(n, NT)), dim3(NT), 0, ST, op, dy, x, dx, n, dtype);
    return comat_check_launch("comat_unary_bwd");
}

extern "C" int comat_axpby(float a, const void* x, float b, const void* y, void* out, int64_t n, int32_t x_dtype,
                           int32_t y_dtype, int32_t out_dtype, void* stream) {
    COMAT_REQUIRE(x && out && n > 0, "comat_axpby: bad args");
    COMAT_REQUIRE(dtype_ok(x_dtype) && dtype_ok(out_dtype) && (!y || dtype_ok(y_dtype)), "comat_axpby: bad dtype");
    hipLaunchKernelGGL(axpby_kernel, dim3(grid_1d(n, NT)), dim3(NT), 0, ST, a, x, b, y, out, n, x_dtype, y_dtype,
                       out_dtype);
    return comat_check_launch("comat_axpby");
}

extern "C" int comat_geglu_fwd(const void* x, void* y, int64_t M, int32_t D, int32_t dtype, void* stream) {
    COMAT_REQUIRE(x && y && M > 0 && D > 0 && dtype_ok(dtype), "comat_geglu_fwd: bad args");
    hipLaunchKernelGGL(geglu_fwd_kernel, dim3(grid_1d(M * D, NT)), dim3(NT), 0, ST, x, y, M, D, dtype);
    return comat_check_launch("comat_geglu_fwd");
}

extern "C" int comat_geglu_il_fwd(const void* x, void* y, int64_t M, int32_t D, int32_t dtype, void* stream) {
    COMAT_REQUIRE(x && y && M > 0 && D > 0 && D % 16 == 0 && dtype_ok(dtype), "comat_geglu_il_fwd: bad args (D must be a multiple of 16)");
    COMAT_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "comat_geglu_il_fwd: operands must be 16-byte aligned");
    const int g = grid_1d(M * (D / 8), NT, 1 << 20);
    if (dtype == COMAT_BF16) hipLaunchKernelGGL(geglu_il_fwd_kernel<bf16_t>, dim3(g), dim3(NT), 0, ST, (const bf16_t*)x, (bf16_t*)y, M, D);
    else hipLaunchKernelGGL(geglu_il_fwd_kernel<float>, dim3(g), dim3(NT), 0, ST, (const float*)x, (float*)y, M, D);
    return comat_check_launch("comat_geglu_il_fwd");
}

extern "C" int comat_geglu_il_bwd(const void* dy, const void* x, void* dx, int64_t M, int32_t D, int32_t dtype, void* stream) {
    COMAT_REQUIRE(dy && x && dx && M > 0 && D > 0 && D % 16 == 0 && dtype_ok(dtype), "comat_geglu_il_bwd: bad args (D must be a multiple of 16)");
    COMAT_REQUIRE((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0, "comat_geglu_il_bwd: operands must be 16-byte aligned");
    const int g = grid_1d(M * (D / 8), NT, 1 << 20);
    if (dtype == COMAT_BF16)
        hipLaunchKernelGGL(geglu_il_bwd_kernel<bf16_t>, dim3(g), dim3(NT), 0, ST, (const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)dx, M, D);
    else hipLaunchKernelGGL(geglu_il_bwd_kernel<float>, dim3(g), dim3(NT), 0, ST, (const float*)dy, (const float*)x, (float*)dx, M, D);
    return comat_check_launch("comat_geglu_il_bwd");
}

extern "C" int comat_geglu_bwd(const void* dy, const void* x, void* dx, int64_t M, int32_t D, int32_t dtype,
                               void* stream) {
    COMAT_REQUIRE(dy && x && dx && M > 0 && D > 0 && dtype_ok(dtype), "comat_geglu_bwd: bad args");
    hipLaunchKernelGGL(geglu_bwd_kernel, dim3(grid_1d(M * D, NT)), dim3(NT), 0, ST, dy, x, dx, M, D, dtype);
    return comat_check_launch("comat_geglu_bwd");
}

extern "C" int comat_copy2d(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int64_t cols,
                            int32_t src_dtype, int32_t dst_dtype, void* stream) {
    COMAT_REQUIRE(src && dst && rows > 0 && cols > 0 && ld_src >= cols && ld_dst >= cols, "comat_copy2d: bad args");
    COMAT_REQUIRE(dtype_ok(src_dtype) && dtype_ok(dst_dtype), "comat_copy2d: bad dtype");
    hipLaunchKernelGGL(copy2d_kernel, dim3(grid_1d(rows * cols, NT)), dim3(NT), 0, ST, src, ld_src, dst, ld_dst, rows,
                       cols, src_dtype, dst_dtype);
    return comat_check_launch("comat_copy2d");
}

extern "C" int comat_copy2d_pair(const void* src0, int64_t ld_src0, void* dst0, int64_t ld_dst0, int64_t cols0, const void* src1,
                                 int64_t ld_src1, void* dst1, int64_t ld_dst1, int64_t cols1, int64_t rows, int32_t dtype,
                                 void* stream) {
    COMAT_REQUIRE(src0 && dst0 && src1 && dst1 && rows > 0 && cols0 > 0 && cols1 > 0, "comat_copy2d_pair: bad args");
    COMAT_REQUIRE(dtype_ok(dtype), "comat_copy2d_pair: bad dtype");
    const int eb = dtype == COMAT_F32 ? 4 : 2, epv = 16 / eb;
    COMAT_REQUIRE(ld_src0 >= cols0 && ld_dst0 >= cols0 && ld_src1 >= cols1 && ld_dst1 >= cols1, "comat_copy2d_pair: leading dimension too small");
    COMAT_REQUIRE(cols0 % epv == 0 && cols1 % epv == 0 && ld_src0 % epv == 0 && ld_dst0 % epv == 0 && ld_src1 % epv == 0 &&
                      ld_dst1 % epv == 0 && (((uintptr_t)src0 | (uintptr_t)dst0 | (uintptr_t)src1 | (uintptr_t)dst1) & 15) == 0 &&
                      (cols0 + cols1) / epv < (1 << 30),
                  "comat_copy2d_pair: 16-byte rows only (columns and leading dimensions in whole 16-byte vectors, aligned pointers)");
    Copy2dPair p;
    p.src[0] = (const char*)src0; p.src[1] = (const char*)src1; p.dst[0] = (char*)dst0; p.dst[1] = (char*)dst1;
    p.lds[0] = ld_src0 * eb; p.lds[1] = ld_src1 * eb; p.ldd[0] = ld_dst0 * eb; p.ldd[1] = ld_dst1 * eb;
    p.vpr[0] = (int)(cols0 / epv); p.vpr[1] = (int)(cols1 / epv);
    hipLaunchKernelGGL(copy2d_pair_kernel, dim3(grid_1d(rows * (p.vpr[0] + p.vpr[1]), NT, 1 << 16)), dim3(NT), 0, ST, p, rows);
    return comat_check_launch("comat_copy2d_pair");
}

extern "C" int comat_add_rowvec(const void* x, const void* v, void* out, int64_t rows, int64_t cols, int32_t dtype,
                                void* stream) {
    COMAT_REQUIRE(x && v && out && rows > 0 && cols > 0 && dtype_ok(dtype), "comat_add_rowvec: bad args");
    hipLaunchKernelGGL(add_rowvec_kernel, dim3(grid_1d(rows * cols, NT)), dim3(NT), 0, ST, x, v, out, rows, cols,
                       dtype);
    return comat_check_launch("comat_add_rowvec");
}

extern "C" int comat_sumpool2x2(const void* x, void* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t dtype,
                                void* stream) {
    COMAT_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && C > 0 && dtype_ok(dtype), "comat_sumpool2x2: bad args");
    hipLaunchKernelGGL(sumpool2x2_kernel, dim3(grid_1d((int64_t)B * H * W * C, NT)), dim3(NT), 0, ST, x, y, B, H, W, C,
                       dtype);
    return comat_check_launch("comat_sumpool2x2");
}

extern "C" int comat_permute_nchw_nhwc(const void* x, void* y, int32_t B, int32_t C, int32_t H, int32_t W,
                                       int32_t to_nhwc, int32_t x_dtype, int32_t y_dtype, void* stream) {
    COMAT_REQUIRE(x && y && B > 0 && C > 0 && H > 0 && W > 0, "comat_permute_nchw_nhwc: bad args");
    COMAT_REQUIRE(dtype_ok(x_dtype) && dtype_ok(y_dtype), "comat_permute_nchw_nhwc: bad dtype");
    hipLaunchKernelGGL(permute_kernel, dim3(grid_1d((int64_t)B * C * H * W, NT)), dim3(NT), 0, ST, x, y, B, C, H, W,
                       to_nhwc, x_dtype, y_dtype);
    return comat_check_launch("comat_permute_nchw_nhwc");
}

extern "C" int comat_cfg_ddpm_fwd(const float* x, const void* eps2, const float* z, float* x_prev, int64_t n, float s,
                                  float cx, float ce, float sigma, int32_t eps_dtype, void* stream) {
    COMAT_REQUIRE(x && eps2 && x_prev && n > 0 && dtype_ok(eps_dtype), "comat_cfg_ddpm_fwd: bad args");
    hipLaunchKernelGGL(cfg_ddpm_fwd_kernel, dim3(grid_1d(n, NT)), dim3(NT), 0, ST, x, eps2, z, x_prev, n, s, cx, ce,
                       sigma, eps_dtype);
    return comat_check_launch("comat_cfg_ddpm_fwd");
}

extern "C" int comat_cfg_ddpm_bwd(const float* g, float* dx, void* deps2, int64_t n, float s, float cx, float ce,
                                  int32_t eps_dtype, void* stream) {
    COMAT_REQUIRE(g && deps2 && n > 0 && dtype_ok(eps_dtype), "comat_cfg_ddpm_bwd: bad args");
    hipLaunchKernelGGL(cfg_ddpm_bwd_kernel, dim3(grid_1d(n, NT)), dim3(NT), 0, ST, g, dx, deps2, n, s, cx, ce,
                       eps_dtype);
    return comat_check_launch("comat_cfg_ddpm_bwd");
}

static int rescale_args_ok(const char* who, int64_t n, int32_t batch, int64_t per_sample, const void* stats, int32_t eps_dtype,
                           uintptr_t f32_ptrs, const void* eps2, const void* deps2) {
    COMAT_REQUIRE(n > 0 && batch > 0 && per_sample > 0 && dtype_ok(eps_dtype), "%s: bad args", who);
    COMAT_REQUIRE((int64_t)batch * per_sample == n, "%s: batch (%d) * per_sample (%lld) != n (%lld)", who, batch,
                  (long long)per_sample, (long long)n);
    COMAT_REQUIRE(stats, "%s: null statistics buffer (fp32 [batch, 4])", who);
    const uintptr_t emask = eps_dtype == COMAT_F32 ? 15 : 7;
    COMAT_REQUIRE(per_sample % 4 == 0 && (f32_ptrs & 15) == 0 && (((uintptr_t)eps2 | (uintptr_t)deps2) & emask) == 0,
                  "%s: per_sample must be a multiple of 4 and the operands aligned to 4 values", who);
    return COMAT_OK;
}

extern "C" int comat_cfg_rescale_ddpm_fwd(const float* x, const void* eps2, const float* z, float* x_prev, int64_t n, float s,
                                          float cx, float ce, float sigma, float phi, int32_t batch, int64_t per_sample,
                                          float* stats, int32_t eps_dtype, void* stream) {
    COMAT_REQUIRE(x && eps2 && x_prev, "comat_cfg_rescale_ddpm_fwd: null operand");
    if (rescale_args_ok("comat_cfg_rescale_ddpm_fwd", n, batch, per_sample, stats, eps_dtype,
                        (uintptr_t)x | (uintptr_t)z | (uintptr_t)x_prev, eps2, nullptr) != COMAT_OK)
        return COMAT_EINVAL;
    if (eps_dtype == COMAT_BF16)
        hipLaunchKernelGGL(cfg_rescale_ddpm_fwd_kernel<bf16_t>, dim3(batch), dim3(RT), 0, ST, x, (const bf16_t*)eps2, z, x_prev, n,
                           per_sample, s, cx, ce, sigma, phi, stats);
    else
        hipLaunchKernelGGL(cfg_rescale_ddpm_fwd_kernel<float>, dim3(batch), dim3(RT), 0, ST, x, (const float*)eps2, z, x_prev, n,
                           per_sample, s, cx, ce, sigma, phi, stats);
    return comat_check_launch("comat_cfg_rescale_ddpm_fwd");
}

extern "C" int comat_cfg_rescale_ddpm_bwd(const float* g, const void* eps2, const float* stats, float* dx, void* deps2,
                                          int64_t n, float s, float cx, float ce, float phi, int32_t batch,
                                          int64_t per_sample, int32_t eps_dtype, void* stream) {
    COMAT_REQUIRE(g && eps2 && deps2, "comat_cfg_rescale_ddpm_bwd: null operand");
    if (rescale_args_ok("comat_cfg_rescale_ddpm_bwd", n, batch, per_sample, stats, eps_dtype, (uintptr_t)g | (uintptr_t)dx,
                        eps2, deps2) != COMAT_OK)
        return COMAT_EINVAL;
    if (eps_dtype == COMAT_BF16)
        hipLaunchKernelGGL(cfg_rescale_ddpm_bwd_kernel<bf16_t>, dim3(batch), dim3(RT), 0, ST, g, (const bf16_t*)eps2, stats, dx,
                           (bf16_t*)deps2, n, per_sample, s, cx, ce, phi);
    else
        hipLaunchKernelGGL(cfg_rescale_ddpm_bwd_kernel<float>, dim3(batch), dim3(RT), 0, ST, g, (const float*)eps2, stats, dx,
                           (float*)deps2, n, per_sample, s, cx, ce, phi);
    return comat_check_launch("comat_cfg_rescale_ddpm_bwd");
}

static int step2_args_ok(const char* who, int64_t n, int32_t halves, float phi, int32_t batch, int64_t per_sample,
                         bool needs_stats, const void* stats, int32_t eps_dtype, uintptr_t f32_ptrs, const void* eps,
                         const void* deps) {
    COMAT_REQUIRE(n > 0 && batch > 0 && per_sample > 0 && dtype_ok(eps_dtype), "%s: bad args", who);
    COMAT_REQUIRE(halves == 1 || halves == 2, "%s: halves must be 1 or 2, got %d", who, halves);
    COMAT_REQUIRE(phi >= 0.f, "%s: phi must be >= 0", who);
    COMAT_REQUIRE(halves == 2 || phi == 0.f, "%s: halves = 1 (guidance off) takes no rescale: phi must be 0", who);
    COMAT_REQUIRE((int64_t)batch * per_sample == n, "%s: batch (%d) * per_sample (%lld) != n (%lld)", who, batch,
                  (long long)per_sample, (long long)n);
    COMAT_REQUIRE(!needs_stats || stats, "%s: null statistics buffer (fp32 [batch, 4]) with phi > 0", who);
    const uintptr_t emask = eps_dtype == COMAT_F32 ? 15 : 7;
    COMAT_REQUIRE(per_sample % 4 == 0 && (f32_ptrs & 15) == 0 && (((uintptr_t)eps | (uintptr_t)deps) & emask) == 0,
                  "%s: per_sample must be a multiple of 4 and the operands aligned to 4 values", who);
    return COMAT_OK;
}

// phi > 0: one block per sample; phi == 0: the blocks share the n / 4 vectors
static unsigned step2_grid(bool per_sample_blocks, int32_t batch, int64_t n) {
    if (per_sample_blocks) return (unsigned)batch;
    const int64_t b = (n / 4 + RT - 1) / RT;
    return (unsigned)(b < 1024 ? b : 1024);
}

extern "C" int comat_ddpm_step2_fwd(const float* x, const void* eps, const float* z, float* x_prev, float* x0, int64_t n,
                                    int32_t halves, float s, float cx, float ce, float sigma, float px, float pe, float phi,
                                    int32_t batch, int64_t per_sample, float* stats, int32_t eps_dtype, void* stream) {
    COMAT_REQUIRE(x && eps, "comat_ddpm_step2_fwd: null operand");
    COMAT_REQUIRE(x_prev || x0, "comat_ddpm_step2_fwd: both outputs (x_prev, x0) are null");
    if (step2_args_ok("comat_ddpm_step2_fwd", n, halves, phi, batch, per_sample, phi > 0.f, stats, eps_dtype,
                      (uintptr_t)x | (uintptr_t)z | (uintptr_t)x_prev | (uintptr_t)x0, eps, nullptr) != COMAT_OK)
        return COMAT_EINVAL;
    const dim3 grid(step2_grid(phi > 0.f, batch, n));
#define COMAT_STEP2_FWD(T, H)                                                                                             \
    hipLaunchKernelGGL((ddpm_step2_fwd_kernel<T, H>), grid, dim3(RT), 0, ST, x, (const T*)eps, z, x_prev, x0, n, per_sample, s, \
                       cx, ce, sigma, px, pe, phi, stats)
    if (eps_dtype == COMAT_BF16) {
        if (halves == 2) COMAT_STEP2_FWD(bf16_t, 2); else COMAT_STEP2_FWD(bf16_t, 1);
    } else {
        if (halves == 2) COMAT_STEP2_FWD(float, 2); else COMAT_STEP2_FWD(float, 1);
    }
#undef COMAT_STEP2_FWD
    return comat_check_launch("comat_ddpm_step2_fwd");
}

extern "C" int comat_ddpm_step2_bwd(const float* g_prev, const float* g_x0, const void* eps, const float* stats, float* dx,
                                    void* deps, int64_t n, int32_t halves, float s, float cx, float ce, float px, float pe,
                                    float phi, int32_t batch, int64_t per_sample, int32_t eps_dtype, void* stream) {
    COMAT_REQUIRE(g_prev || g_x0, "comat_ddpm_step2_bwd: both gradients (g_prev, g_x0) are null");
    COMAT_REQUIRE(dx || deps, "comat_ddpm_step2_bwd: both outputs (dx, deps) are null");
    const bool rescaled = phi > 0.f && deps != nullptr;  // without deps the step is affine in x: no statistics are read
    COMAT_REQUIRE(!rescaled || eps, "comat_ddpm_step2_bwd: null eps with phi > 0");
    if (step2_args_ok("comat_ddpm_step2_bwd", n, halves, phi, batch, per_sample, rescaled, stats, eps_dtype,
                      (uintptr_t)g_prev | (uintptr_t)g_x0 | (uintptr_t)dx, rescaled ? eps : nullptr, deps) != COMAT_OK)
        return COMAT_EINVAL;
    const dim3 grid(step2_grid(rescaled, batch, n));
#define COMAT_STEP2_BWD(T, H)                                                                                              \
    hipLaunchKernelGGL((ddpm_step2_bwd_kernel<T, H>), grid, dim3(RT), 0, ST, g_prev, g_x0, (const T*)eps, stats, dx, (T*)deps, n, \
                       per_sample, s, cx, ce, px, pe, phi)
    if (eps_dtype == COMAT_BF16) {
        if (halves == 2) COMAT_STEP2_BWD(bf16_t, 2); else COMAT_STEP2_BWD(bf16_t, 1);
    } else {
        if (halves == 2) COMAT_STEP2_BWD(float, 2); else COMAT_STEP2_BWD(float, 1);
    }
#undef COMAT_STEP2_BWD
    return comat_check_launch("comat_ddpm_step2_bwd");
}

extern "C" int comat_add_noise_fwd(const float* x, const float* noise, float* noisy, void* xin, int64_t n, float sa, float sb,
                                   int32_t copies, int32_t xin_dtype, void* stream) {
    COMAT_REQUIRE(x && noise && noisy && xin && n > 0 && dtype_ok(xin_dtype), "comat_add_noise_fwd: bad args");
    COMAT_REQUIRE(copies == 1 || copies == 2, "comat_add_noise_fwd: copies must be 1 or 2, got %d", copies);
    hipLaunchKernelGGL(add_noise_fwd_kernel, dim3(grid_1d(n, NT)), dim3(NT), 0, ST, x, noise, noisy, xin, n, sa, sb, copies,
                       xin_dtype);
    return comat_check_launch("comat_add_noise_fwd");
}

extern "C" int comat_transpose_cast_tiles(const float* src, void* dst, const int64_t* tiles, int64_t n_tiles,
                                          int32_t out_dtype, void* stream) {
    COMAT_REQUIRE(src && dst && tiles && n_tiles > 0 && n_tiles < (1ll << 31) && dtype_ok(out_dtype),
                  "comat_transpose_cast_tiles: bad args");
    hipLaunchKernelGGL(transpose_tiles_kernel, dim3((unsigned)n_tiles), dim3(NT), 0, ST, src, dst, tiles, out_dtype);
    return comat_check_launch("comat_transpose_cast_tiles");
}
