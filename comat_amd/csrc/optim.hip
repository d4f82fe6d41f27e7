// optim.hip — optimizer tail on the flat fp32 trainable buffers: global-norm reduction and fused clip + AdamW.
// (training_script.py:661-664,692-694: clip_grad_norm_ then AdamW.step, one HBM pass over p/g/m/v.)
#include "common.h"

namespace {

constexpr int NT = 256;

// Two stages with a fixed summation order: the global gradient norm (and with it the clip factor) must come out
// bit-identical on every data-parallel rank, or the replicas drift apart; float atomics would make it order-dependent.
__global__ __launch_bounds__(NT) void sumsq_partial_kernel(const float* __restrict__ x, int64_t n,
                                                           float* __restrict__ ws) {
    __shared__ float sbuf[4];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) acc += x[i] * x[i];
    acc = block_sum_256(acc, sbuf);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}
__global__ __launch_bounds__(NT) void sumsq_final_kernel(const float* __restrict__ ws, int nparts,
                                                         float* __restrict__ out) {
    __shared__ float sbuf[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nparts; i += NT) acc += ws[i];
    acc = block_sum_256(acc, sbuf);
    if (threadIdx.x == 0) out[0] += acc;
}

// |g|_2 of the image gradient and its normalisation (training_script.py:644-651): the partial sums of stage one (one per block,
// fixed grid) are added again by EVERY block of stage two, in the same fixed order, so that each block has the norm without a
// third launch or a grid-wide wait; block 0 publishes it.
template <typename T>
__global__ __launch_bounds__(NT) void gnorm_partial_kernel(const T* __restrict__ x, int64_t n, float* __restrict__ ws) {
    __shared__ float sbuf[4];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const float v = ldf<T>(x + i);
        acc += v * v;
    }
    acc = block_sum_256(acc, sbuf);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}
template <typename T>
__global__ __launch_bounds__(NT) void gnorm_scale_kernel(const T* __restrict__ g, T* __restrict__ out, int64_t n,
                                                         const float* __restrict__ ws, int nparts,
                                                         float* __restrict__ norm_out, float target) {
    __shared__ float sbuf[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nparts; i += NT) acc += ws[i];
    const float norm = sqrtf(block_sum_256(acc, sbuf));
    if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
    if (!(target > 0.f)) return;
    // a zero gradient stays zero (0 * (target / 0) would be NaN); a NaN norm is carried into every element
    const float c = norm == 0.f ? 0.f : target / norm;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        stf<T>(out + i, ldf<T>(g + i) * c);
}

__global__ __launch_bounds__(NT) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                   float b1, float b2, float eps, float wd, float bc1, float bc2s,
                                                   const int32_t* __restrict__ step_dev,
                                                   const float* __restrict__ gnorm_sq, float max_norm, float grad_scale) {
    // grad_scale: the buffer holds the SUM of the data-parallel ranks' gradients (RCCL all-reduce SUM); 1 / world turns
    // it - and its norm - into the mean here, instead of one more pass over the buffer
    float clip = grad_scale;
    if (step_dev) {  // step count of applied updates lives on the device (see comat_adamw_tick)
        const float t = (float)(*step_dev + 1);
        bc1 = 1.0f - powf(b1, t);
        bc2s = sqrtf(1.0f - powf(b2, t));
    }
    // a non-finite gradient norm (overflow / NaN somewhere in backward) skips the update, like the GradScaler step
    // of the reference's mixed-precision run (accelerate, training_script.py:661-664): parameters and moments stay
    if (gnorm_sq && !isfinite(*gnorm_sq)) return;
    if (gnorm_sq && max_norm > 0.f) {
        const float c = max_norm / (sqrtf(*gnorm_sq) * grad_scale + 1e-6f);
        clip = c < 1.0f ? c * grad_scale : grad_scale;
    }
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const float gi = g[i] * clip;
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        float pi = p[i] * (1.0f - lr * wd);
        pi -= (lr / bc1) * mi / (sqrtf(vi) / bc2s + eps);
        p[i] = pi;
    }
}

__global__ void adamw_tick_kernel(int32_t* __restrict__ counters, const float* __restrict__ gnorm_sq) {
    if (threadIdx.x == 0) counters[isfinite(*gnorm_sq) ? 0 : 1] += 1;
}

// ---- learning-rate schedule evaluated on the device (training_script.py:290-295,664,667) ----------------------------------
// The multiplier of transformers.optimization for each `--lr_scheduler` name, term by term and in that library's order of
// operations, in double; no contraction into fused multiply-adds, so that the kinds built from one division and one product
// come out as the host library's doubles do, bit for bit.
__device__ float lr_at(const comat_lr_schedule& s, int32_t applied) {
#pragma clang fp contract(off)
    const int64_t c = s.stride * (int64_t)applied;
    const int64_t W = s.warmup, T = s.total;
    const double one = 1.0;
    double lam = 1.0;
    if (s.kind != COMAT_LR_CONSTANT) {
        const double span = (double)(T - W > 1 ? T - W : 1);
        if (c < W) {
            lam = (double)c / (double)(W > 1 ? W : 1);
        } else if (s.kind == COMAT_LR_LINEAR) {
            lam = fmax(0.0, (double)(T - c) / span);
        } else if (s.kind == COMAT_LR_COSINE) {
            const double progress = (double)(c - W) / span;
            lam = fmax(0.0, 0.5 * (one + cos(M_PI * s.num_cycles * 2.0 * progress)));
        } else if (s.kind == COMAT_LR_COSINE_WITH_RESTARTS) {
            const double progress = (double)(c - W) / span;
            lam = progress >= 1.0 ? 0.0 : fmax(0.0, 0.5 * (one + cos(M_PI * fmod(s.num_cycles * progress, 1.0))));
        } else if (s.kind == COMAT_LR_POLYNOMIAL) {
            if (c > T) {
                lam = s.lr_end / s.base_lr;
            } else {
                const double pct = one - (double)(c - W) / (double)(T - W);
                const double pw = s.power == 1.0 ? pct : pow(pct, s.power);
                lam = ((s.base_lr - s.lr_end) * pw + s.lr_end) / s.base_lr;
            }
        }
    }
    return (float)(s.base_lr * lam);
}

__global__ void lr_schedule_eval_kernel(const comat_lr_schedule s, const int32_t* __restrict__ counters,
                                        float* __restrict__ lr_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) lr_out[0] = lr_at(s, counters[0]);
}

// adamw_tick_kernel, then the learning rate of the NEXT update from the new count; a skipped update moves neither
__global__ void adamw_tick_lr_kernel(int32_t* __restrict__ counters, const float* __restrict__ gnorm_sq,
                                     const comat_lr_schedule s, float* __restrict__ lr_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (isfinite(*gnorm_sq)) {
        const int32_t applied = counters[0] + 1;
        counters[0] = applied;
        lr_out[0] = lr_at(s, applied);
    } else {
        counters[1] += 1;
    }
}

// (adamw_element, one element of adamw_kernel's loop with the roundings spelled out: common.h - optim8.hip runs it too)

// adamw_kernel with the learning rate read from device memory (the word comat_adamw_tick_lr / comat_lr_schedule_eval write).
// VEC: p, g, m, v are 16-byte aligned - four elements per lane and access; the n % 4 last elements go to block 0's first lanes.
// window (nullable; comat_adamw_window): the launch updates only when *window == accum_steps - 1, the closing micro-step of a
// gradient-accumulation window (accelerate's `sync_gradients`, training_script.py:556,680); otherwise every block leaves after
// that one uniform load and p, m, v are not written.
template <bool VEC>
__global__ __launch_bounds__(NT) void adamw_lr_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                      const float* __restrict__ lr_dev, float b1, float b2, float eps,
                                                      float wd, const int32_t* __restrict__ step_dev,
                                                      const float* __restrict__ gnorm_sq, float max_norm, float grad_scale,
                                                      const int32_t* __restrict__ window, int32_t accum_steps) {
#pragma clang fp contract(off)
    if (window && *window != accum_steps - 1) return;
    float clip = grad_scale;
    const float lr = *lr_dev;
    const float t = (float)(*step_dev + 1);
    const float bc1 = 1.0f - powf(b1, t);
    const float bc2s = sqrtf(1.0f - powf(b2, t));
    if (gnorm_sq && !isfinite(*gnorm_sq)) return;
    if (gnorm_sq && max_norm > 0.f) {
        const float c = max_norm / fmaf(sqrtf(*gnorm_sq), grad_scale, 1e-6f);
        clip = c < 1.0f ? c * grad_scale : grad_scale;
    }
    const float pw = fmaf(-lr, wd, 1.0f), lr_bc1 = lr / bc1, one_b1 = 1.0f - b1, one_b2 = 1.0f - b2;
#define COMAT_ADAMW_ELEMENT(P, G, M, V) adamw_element(P, G, M, V, clip, pw, lr_bc1, b1, b2, one_b1, one_b2, eps, bc2s)
    if (VEC) {
        const int64_t n4 = n >> 2;
        float4* p4 = reinterpret_cast<float4*>(p);
        const float4* g4 = reinterpret_cast<const float4*>(g);
        float4* m4 = reinterpret_cast<float4*>(m);
        float4* v4 = reinterpret_cast<float4*>(v);
        for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) {
            float4 pv = p4[i], mv = m4[i], vv = v4[i];
            const float4 gv = g4[i];
            COMAT_ADAMW_ELEMENT(pv.x, gv.x, mv.x, vv.x);
            COMAT_ADAMW_ELEMENT(pv.y, gv.y, mv.y, vv.y);
            COMAT_ADAMW_ELEMENT(pv.z, gv.z, mv.z, vv.z);
            COMAT_ADAMW_ELEMENT(pv.w, gv.w, mv.w, vv.w);
            m4[i] = mv;
            v4[i] = vv;
            p4[i] = pv;
        }
        const int64_t i = (n4 << 2) + threadIdx.x;
        if (blockIdx.x == 0 && i < n) COMAT_ADAMW_ELEMENT(p[i], g[i], m[i], v[i]);
    } else {
        for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
            COMAT_ADAMW_ELEMENT(p[i], g[i], m[i], v[i]);
    }
#undef COMAT_ADAMW_ELEMENT
}

// The gradient buffer is zeroed only at the first micro-step of a window (optimizer.zero_grad() after a closing step, as accelerate
// documents the loop): *window != 0 leaves every byte as it is.  VEC: g is 16-byte aligned; the n % 4 tail goes one by one.
template <bool VEC>
__global__ __launch_bounds__(NT) void accum_zero_kernel(float* __restrict__ g, int64_t n, const int32_t* __restrict__ window) {
    if (*window != 0) return;
    if (VEC) {
        const int64_t n4 = n >> 2;
        float4* g4 = reinterpret_cast<float4*>(g);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NT) g4[i] = z;
        const int64_t i = (n4 << 2) + threadIdx.x;
        if (blockIdx.x == 0 && i < n) g[i] = 0.f;
    } else {
        for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) g[i] = 0.f;
    }
}

// The bookkeeping of one micro-step, one thread: train_loss[0] gathers loss / N over the window (training_script.py:655), and at
// the closing micro-step the counters and the rate move as under adamw_tick_kernel / adamw_tick_lr_kernel (:664 under
// `sync_gradients`), train_loss[1] publishes the closed window's sum (:702) and the window restarts - also after a skipped update.
__global__ void window_tick_kernel(int32_t* __restrict__ window, int32_t accum_steps, int32_t* __restrict__ counters,
                                   const float* __restrict__ gnorm_sq, const comat_lr_schedule s, int has_sched,
                                   float* __restrict__ lr_out, const float* __restrict__ step_loss,
                                   float* __restrict__ train_loss) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int32_t w = window[0];
    if (train_loss) train_loss[0] = (w == 0 ? 0.f : train_loss[0]) + *step_loss / (float)accum_steps;
    if (w != accum_steps - 1) {
        window[0] = w + 1;
        return;
    }
    if (isfinite(*gnorm_sq)) {
        const int32_t applied = counters[0] + 1;
        counters[0] = applied;
        if (has_sched) lr_out[0] = lr_at(s, applied);
    } else {
        counters[1] += 1;
    }
    if (train_loss) train_loss[1] = train_loss[0];
    window[0] = 0;
}

// the contract's refusals, shared by the entry points that take a schedule
int lr_schedule_check(const comat_lr_schedule* s, const char* who) {
    COMAT_REQUIRE(s, "%s: null schedule", who);
    COMAT_REQUIRE(s->kind >= COMAT_LR_CONSTANT && s->kind <= COMAT_LR_POLYNOMIAL, "%s: unknown schedule kind %lld", who,
                  (long long)s->kind);
    COMAT_REQUIRE(s->stride >= 1 && s->warmup >= 0, "%s: stride must be >= 1 and warmup >= 0 (got %lld, %lld)", who,
                  (long long)s->stride, (long long)s->warmup);
    COMAT_REQUIRE(s->kind < COMAT_LR_LINEAR || s->total >= 1, "%s: this kind needs total >= 1 (got %lld)", who,
                  (long long)s->total);
    // (the host library raises at construction)
    COMAT_REQUIRE(s->kind != COMAT_LR_POLYNOMIAL || s->base_lr > s->lr_end, "%s: polynomial needs base_lr > lr_end", who);
    return COMAT_OK;
}

}  // namespace

extern "C" int comat_sumsq(const float* x, int64_t n, float* out, float* ws, void* stream) {
    COMAT_REQUIRE(x && out && ws && n > 0, "comat_sumsq: bad args");
    const int parts = grid_1d(n, NT, 1024);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(parts), dim3(NT), 0, (hipStream_t)stream, x, n, ws);
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const float*)ws, parts, out);
    return comat_check_launch("comat_sumsq");
}

extern "C" int comat_grad_norm_scale(const void* g, void* g_out, int64_t n, int32_t dtype, float* norm_out, float target,
                                     float* ws, void* stream) {
    COMAT_REQUIRE(g && norm_out && ws && n > 0 && dtype_ok(dtype), "comat_grad_norm_scale: bad args");
    COMAT_REQUIRE(target >= 0.f && (target == 0.f || g_out), "comat_grad_norm_scale: target > 0 needs g_out (target >= 0)");
    const int parts = grid_1d(n, NT, 1024);
    const int grid2 = target > 0.f ? grid_1d(n, NT) : 1;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == COMAT_BF16) {
        hipLaunchKernelGGL(gnorm_partial_kernel<bf16_t>, dim3(parts), dim3(NT), 0, st, (const bf16_t*)g, n, ws);
        hipLaunchKernelGGL(gnorm_scale_kernel<bf16_t>, dim3(grid2), dim3(NT), 0, st, (const bf16_t*)g, (bf16_t*)g_out, n,
                           (const float*)ws, parts, norm_out, target);
    } else {
        hipLaunchKernelGGL(gnorm_partial_kernel<float>, dim3(parts), dim3(NT), 0, st, (const float*)g, n, ws);
        hipLaunchKernelGGL(gnorm_scale_kernel<float>, dim3(grid2), dim3(NT), 0, st, (const float*)g, (float*)g_out, n,
                           (const float*)ws, parts, norm_out, target);
    }
    return comat_check_launch("comat_grad_norm_scale");
}

extern "C" int comat_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                           float eps, float weight_decay, int32_t step, const int32_t* step_dev,
                           const float* gnorm_sq, float max_norm, float grad_scale, void* stream) {
    COMAT_REQUIRE(p && g && m && v && n > 0 && (step >= 1 || step_dev) && grad_scale > 0.f, "comat_adamw: bad args");
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2s = sqrtf(1.0f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adamw_kernel, dim3(grid_1d(n, NT)), dim3(NT), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1,
                       beta2, eps, weight_decay, bc1, bc2s, step_dev, gnorm_sq, max_norm, grad_scale);
    return comat_check_launch("comat_adamw");
}

extern "C" int comat_adamw_tick(int32_t* counters, const float* gnorm_sq, void* stream) {
    COMAT_REQUIRE(counters && gnorm_sq, "comat_adamw_tick: null pointer");
    hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counters, gnorm_sq);
    return comat_check_launch("comat_adamw_tick");
}

extern "C" int comat_lr_schedule_eval(const comat_lr_schedule* sched, const int32_t* counters, float* lr_out, void* stream) {
    if (int rc = lr_schedule_check(sched, "comat_lr_schedule_eval")) return rc;
    COMAT_REQUIRE(counters && lr_out, "comat_lr_schedule_eval: null pointer");
    hipLaunchKernelGGL(lr_schedule_eval_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *sched, counters, lr_out);
    return comat_check_launch("comat_lr_schedule_eval");
}

extern "C" int comat_adamw_tick_lr(int32_t* counters, const float* gnorm_sq, const comat_lr_schedule* sched, float* lr_out,
                                   void* stream) {
    if (int rc = lr_schedule_check(sched, "comat_adamw_tick_lr")) return rc;
    COMAT_REQUIRE(counters && gnorm_sq && lr_out, "comat_adamw_tick_lr: null pointer");
    hipLaunchKernelGGL(adamw_tick_lr_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counters, gnorm_sq, *sched, lr_out);
    return comat_check_launch("comat_adamw_tick_lr");
}

// the launch of comat_adamw_lr (window == NULL) and of comat_adamw_window
static void launch_adamw_lr(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2,
                            float eps, float weight_decay, const int32_t* step_dev, const float* gnorm_sq, float max_norm,
                            float grad_scale, const int32_t* window, int32_t accum_steps, void* stream) {
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(adamw_lr_kernel<true>, dim3(grid_1d(n >> 2, NT)), dim3(NT), 0, (hipStream_t)stream, p, g, m, v, n,
                           lr_dev, beta1, beta2, eps, weight_decay, step_dev, gnorm_sq, max_norm, grad_scale, window, accum_steps);
    else
        hipLaunchKernelGGL(adamw_lr_kernel<false>, dim3(grid_1d(n, NT)), dim3(NT), 0, (hipStream_t)stream, p, g, m, v, n,
                           lr_dev, beta1, beta2, eps, weight_decay, step_dev, gnorm_sq, max_norm, grad_scale, window, accum_steps);
}

extern "C" int comat_adamw_lr(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1,
                              float beta2, float eps, float weight_decay, const int32_t* step_dev, const float* gnorm_sq,
                              float max_norm, float grad_scale, void* stream) {
    COMAT_REQUIRE(p && g && m && v && n > 0 && lr_dev && step_dev && grad_scale > 0.f,
                  "comat_adamw_lr: bad args (lr_dev and step_dev are required)");
    launch_adamw_lr(p, g, m, v, n, lr_dev, beta1, beta2, eps, weight_decay, step_dev, gnorm_sq, max_norm, grad_scale, nullptr, 1,
                    stream);
    return comat_check_launch("comat_adamw_lr");
}

extern "C" int comat_accum_zero(float* g, int64_t n, const int32_t* window, void* stream) {
    COMAT_REQUIRE(g && window, "comat_accum_zero: null pointer");
    COMAT_REQUIRE(n >= 1, "comat_accum_zero: n must be >= 1 (got %lld)", (long long)n);
    if (((uintptr_t)g & 15) == 0)
        hipLaunchKernelGGL(accum_zero_kernel<true>, dim3(grid_1d(n >> 2, NT)), dim3(NT), 0, (hipStream_t)stream, g, n, window);
    else
        hipLaunchKernelGGL(accum_zero_kernel<false>, dim3(grid_1d(n, NT)), dim3(NT), 0, (hipStream_t)stream, g, n, window);
    return comat_check_launch("comat_accum_zero");
}

extern "C" int comat_adamw_window(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1,
                                  float beta2, float eps, float weight_decay, const int32_t* step_dev, const float* gnorm_sq,
                                  float max_norm, float grad_scale, const int32_t* window, int32_t accum_steps, void* stream) {
    COMAT_REQUIRE(p && g && m && v && lr_dev && step_dev && window, "comat_adamw_window: null pointer");
    COMAT_REQUIRE(n >= 1 && grad_scale > 0.f, "comat_adamw_window: n must be >= 1 and grad_scale > 0 (got %lld, %g)", (long long)n,
                  (double)grad_scale);
    COMAT_REQUIRE(accum_steps >= 1, "comat_adamw_window: accum_steps must be >= 1 (got %d)", (int)accum_steps);
    launch_adamw_lr(p, g, m, v, n, lr_dev, beta1, beta2, eps, weight_decay, step_dev, gnorm_sq, max_norm, grad_scale, window,
                    accum_steps, stream);
    return comat_check_launch("comat_adamw_window");
}

extern "C" int comat_window_tick(int32_t* window, int32_t accum_steps, int32_t* counters, const float* gnorm_sq,
                                 const comat_lr_schedule* sched, float* lr_out, const float* step_loss, float* train_loss,
                                 void* stream) {
    if (sched)
        if (int rc = lr_schedule_check(sched, "comat_window_tick")) return rc;
    COMAT_REQUIRE(window && counters && gnorm_sq && (!sched || lr_out), "comat_window_tick: null pointer");
    COMAT_REQUIRE(accum_steps >= 1, "comat_window_tick: accum_steps must be >= 1 (got %d)", (int)accum_steps);
    COMAT_REQUIRE(!step_loss == !train_loss, "comat_window_tick: step_loss and train_loss go together");
    hipLaunchKernelGGL(window_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, window, accum_steps, counters, gnorm_sq,
                       sched ? *sched : comat_lr_schedule{}, sched ? 1 : 0, lr_out, step_loss, train_loss);
    return comat_check_launch("comat_window_tick");
}
