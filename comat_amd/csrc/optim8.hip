// optim8.hip — 8-bit blockwise optimizer state (`--use_8bit_adam`; training_script.py:216-223,258-275: bnb.optim.AdamW8bit for the
// generator and the discriminator): the two code books, blockwise quantise / dequantise, and AdamW on 8-bit moments in one HBM pass
// (16 + 1/16 bytes per element where the fp32 pass of optim.hip moves 28).
//
// Layout of every kernel: a quantisation block is 256 consecutive elements; ONE wave64 owns a block and each lane four consecutive
// elements of it - one 16-byte access per fp32 operand (1 KiB per wave instruction) and one 4-byte word of four codes per state.  The
// block's abs-max is a maximum over cross-lane shuffles: no LDS staging, no barrier, no atomics, nothing order-dependent.  Only the
// lane that holds the end of the buffer (n % 4 elements, or none) goes element by element.
#include "common.h"
#include <string.h>

namespace {

constexpr int NT = 256;  // four waves: four quantisation blocks per trip of the grid-stride loop
constexpr int QB = 256;  // elements per quantisation block

// row 0: unsigned (second moment), row 1: signed (first moment) - the index is `is_signed`
const float q8_map_host[2][256] = {
#include "q8_maps.inc"
};
__device__ const float q8_map_dev[2][256] = {
#include "q8_maps.inc"
};

// A table in LDS with the search tree over it.  tree[k], k = 1..255, is a complete binary tree in breadth-first order whose in-order
// sequence is the 255 midpoints of neighbouring table entries: node k of level L = floor(log2 k), position p = k - 2^L, holds
// midpoint r = (2p + 1) 2^(7-L) - 1, the mean of table[r] and table[r + 1].  A level of up to 32 nodes lies in 32 different banks.
struct Q8Table {
    float tab[256];
    float tree[256];
};
__device__ __forceinline__ void q8_table_fill(Q8Table& s, int is_signed) {  // blockDim.x == 256; the caller synchronises
    const int k = threadIdx.x;
    const float* t = q8_map_dev[is_signed];
    s.tab[k] = t[k];
    float e = 0.f;
    if (k >= 1) {
        const int L = 31 - __clz(k);
        const int r = ((2 * (k - (1 << L)) + 1) << (7 - L)) - 1;  // 0..254
        e = 0.5f * (t[r] + t[r + 1]);
    }
    s.tree[k] = e;
}
// index of a table entry nearest to y: eight steps down the tree, k stays in 1..255 while it is used as an index whatever y is (a NaN
// compares false at every step).  A y at a midpoint (up to the midpoint's fp32 rounding) takes the lower neighbour.
__device__ __forceinline__ uint32_t q8_code(const Q8Table& s, float y) {
    uint32_t k = 1;
#pragma unroll
    for (int step = 0; step < 8; ++step) k = 2 * k + (y > s.tree[k] ? 1u : 0u);
    return k - 256u;
}
// the four codes of a lane under the block's scale; a zero scale (an all-zero block) gives the zero code without a division
__device__ __forceinline__ uint32_t q8_pack4(const Q8Table& s, const float* x, float absmax) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) w |= q8_code(s, absmax > 0.f ? x[j] / absmax : 0.f) << (8 * j);
    return w;
}

// a lane's four elements: `left` = n - (index of the first); an element past the end (j >= left) is not touched and reads as zero
// (codes: as `fill`)
__device__ __forceinline__ void load4(const float* __restrict__ x, int64_t left, float* out) {
    if (left >= 4) {
        const float4 v = *reinterpret_cast<const float4*>(x);
        out[0] = v.x, out[1] = v.y, out[2] = v.z, out[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = j < left ? x[j] : 0.f;
    }
}
__device__ __forceinline__ void store4(float* __restrict__ x, int64_t left, const float* v) {
    if (left >= 4) {
        *reinterpret_cast<float4*>(x) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < left) x[j] = v[j];
    }
}
__device__ __forceinline__ uint32_t load_codes4(const uint8_t* __restrict__ c, int64_t left, uint32_t fill) {
    if (left >= 4) return *reinterpret_cast<const uint32_t*>(c);
    uint32_t w = fill;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < left) w = (w & ~(0xffu << (8 * j))) | ((uint32_t)c[j] << (8 * j));
    return w;
}
__device__ __forceinline__ void store_codes4(uint8_t* __restrict__ c, int64_t left, uint32_t w) {
    if (left >= 4) {
        *reinterpret_cast<uint32_t*>(c) = w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < left) c[j] = (uint8_t)(w >> (8 * j));
    }
}
__device__ __forceinline__ float absmax4(const float* x) {
    return fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3])));
}

__global__ __launch_bounds__(NT) void q8_quantize_kernel(const float* __restrict__ x, uint8_t* __restrict__ codes,
                                                         float* __restrict__ absmax, int64_t n, int is_signed) {
    __shared__ Q8Table s;
    q8_table_fill(s, is_signed);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t nblk = (n + QB - 1) / QB;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nblk; b += (int64_t)gridDim.x * 4) {  // wave-uniform
        const int64_t i0 = b * QB + lane * 4, left = n - i0;
        float xv[4];
        load4(x + i0, left, xv);
        const float a = wave_max(absmax4(xv));
        store_codes4(codes + i0, left, q8_pack4(s, xv, a));
        if (lane == 0) absmax[b] = a;
    }
}

__global__ __launch_bounds__(NT) void q8_dequantize_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ absmax,
                                                           float* __restrict__ x, int64_t n, int is_signed) {
    __shared__ float tab[256];
    tab[threadIdx.x] = q8_map_dev[is_signed][threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t nblk = (n + QB - 1) / QB;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nblk; b += (int64_t)gridDim.x * 4) {
        const int64_t i0 = b * QB + lane * 4, left = n - i0;
        const uint32_t w = load_codes4(codes + i0, left, 0u);
        const float a = absmax[b];
        float xv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = tab[(w >> (8 * j)) & 255u] * a;
        store4(x + i0, left, xv);
    }
}

struct AdamwCoef {
    float clip, pw, lr_bc1, b1, b2, one_b1, one_b2, eps, bc2s;
};
// one quantisation block of adamw8_kernel, one wave; FULL: every lane holds four elements (`left` is 4)
template <bool FULL>
__device__ __forceinline__ void adamw8_block(const Q8Table& sm, const Q8Table& sv, float* __restrict__ p, const float* __restrict__ g,
                                             uint8_t* __restrict__ m8, uint8_t* __restrict__ v8, float* __restrict__ absmax_m,
                                             float* __restrict__ absmax_v, int64_t left_, int lane, const AdamwCoef& c) {
#pragma clang fp contract(off)
    const int64_t left = FULL ? 4 : left_;
    float pv[4], gv[4], mv[4], vv[4];
    load4(p, left, pv);
    load4(g, left, gv);
    const uint32_t mw = load_codes4(m8, left, 0u), vw = load_codes4(v8, left, 0u);
    const float am = *absmax_m, av = *absmax_v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mv[j] = j < left ? sm.tab[(mw >> (8 * j)) & 255u] * am : 0.f;
        vv[j] = j < left ? sv.tab[(vw >> (8 * j)) & 255u] * av : 0.f;
        adamw_element(pv[j], gv[j], mv[j], vv[j], c.clip, c.pw, c.lr_bc1, c.b1, c.b2, c.one_b1, c.one_b2, c.eps, c.bc2s);
    }
    const float nm = wave_max(absmax4(mv)), nv = wave_max(absmax4(vv));
    store4(p, left, pv);
    store_codes4(m8, left, q8_pack4(sm, mv, nm));
    store_codes4(v8, left, q8_pack4(sv, vv, nv));
    if (lane == 0) {
        *absmax_m = nm;
        *absmax_v = nv;
    }
}

// comat_adamw_window on 8-bit moments.  The uniform early exits and the clip factor are those of optim.hip's adamw_lr_kernel, term
// by term, and come before any store; per element: dequantise m and v, adamw_element (common.h: the function and the roundings of
// the fp32 kernels, so p moves from the fresh fp32 moments), then the block's new abs-max of |m'| and of v' and the nearest codes.
// An element past n holds p = g = 0 on zero moments: its m' and v' are 0 and leave the maxima alone; nothing of it is stored.
__global__ __launch_bounds__(NT) void adamw8_kernel(float* __restrict__ p, const float* __restrict__ g, uint8_t* __restrict__ m8,
                                                    uint8_t* __restrict__ v8, float* __restrict__ absmax_m,
                                                    float* __restrict__ absmax_v, int64_t n, const float* __restrict__ lr_dev,
                                                    float b1, float b2, float eps, float wd, const int32_t* __restrict__ step_dev,
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
    const AdamwCoef c = {clip, fmaf(-lr, wd, 1.0f), lr / bc1, b1, b2, 1.0f - b1, 1.0f - b2, eps, bc2s};

    __shared__ Q8Table sm, sv;
    q8_table_fill(sm, 1);
    q8_table_fill(sv, 0);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t nblk = (n + QB - 1) / QB;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nblk; b += (int64_t)gridDim.x * 4) {  // wave-uniform
        const int64_t i0 = b * QB + lane * 4;
        if ((b + 1) * QB <= n)  // wave-uniform: all but the buffer's last block take the form without per-element bounds
            adamw8_block<true>(sm, sv, p + i0, g + i0, m8 + i0, v8 + i0, absmax_m + b, absmax_v + b, 4, lane, c);
        else
            adamw8_block<false>(sm, sv, p + i0, g + i0, m8 + i0, v8 + i0, absmax_m + b, absmax_v + b, n - i0, lane, c);
    }
}

inline bool aligned(const void* ptr, uintptr_t a) { return ((uintptr_t)ptr & (a - 1)) == 0; }
inline int q8_grid(int64_t n) { return grid_1d(cdiv64(n, QB), 4); }

}  // namespace

extern "C" int comat_q8_map(int32_t is_signed, float* host_out256) {
    COMAT_REQUIRE(host_out256, "comat_q8_map: null pointer");
    COMAT_REQUIRE(is_signed == 0 || is_signed == 1, "comat_q8_map: is_signed must be 0 or 1 (got %d)", (int)is_signed);
    memcpy(host_out256, q8_map_host[is_signed], sizeof(q8_map_host[0]));
    return COMAT_OK;
}

extern "C" int comat_q8_quantize_blockwise(const float* x, uint8_t* codes, float* absmax, int64_t n, int32_t is_signed,
                                           void* stream) {
    COMAT_REQUIRE(x && codes && absmax, "comat_q8_quantize_blockwise: null pointer");
    COMAT_REQUIRE(n >= 1 && (is_signed == 0 || is_signed == 1),
                  "comat_q8_quantize_blockwise: n must be >= 1 and is_signed 0 or 1 (got %lld, %d)", (long long)n, (int)is_signed);
    COMAT_REQUIRE(aligned(x, 16) && aligned(absmax, 16) && aligned(codes, 4),
                  "comat_q8_quantize_blockwise: x and absmax must be 16-byte aligned, codes 4-byte aligned");
    hipLaunchKernelGGL(q8_quantize_kernel, dim3(q8_grid(n)), dim3(NT), 0, (hipStream_t)stream, x, codes, absmax, n, (int)is_signed);
    return comat_check_launch("comat_q8_quantize_blockwise");
}

extern "C" int comat_q8_dequantize_blockwise(const uint8_t* codes, const float* absmax, float* x, int64_t n, int32_t is_signed,
                                             void* stream) {
    COMAT_REQUIRE(x && codes && absmax, "comat_q8_dequantize_blockwise: null pointer");
    COMAT_REQUIRE(n >= 1 && (is_signed == 0 || is_signed == 1),
                  "comat_q8_dequantize_blockwise: n must be >= 1 and is_signed 0 or 1 (got %lld, %d)", (long long)n, (int)is_signed);
    COMAT_REQUIRE(aligned(x, 16) && aligned(absmax, 16) && aligned(codes, 4),
                  "comat_q8_dequantize_blockwise: x and absmax must be 16-byte aligned, codes 4-byte aligned");
    hipLaunchKernelGGL(q8_dequantize_kernel, dim3(q8_grid(n)), dim3(NT), 0, (hipStream_t)stream, codes, absmax, x, n, (int)is_signed);
    return comat_check_launch("comat_q8_dequantize_blockwise");
}

extern "C" int comat_adamw8_window(float* p, const float* g, uint8_t* m8, uint8_t* v8, float* absmax_m, float* absmax_v, int64_t n,
                                   const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                   const int32_t* step_dev, const float* gnorm_sq, float max_norm, float grad_scale,
                                   const int32_t* window, int32_t accum_steps, void* stream) {
    COMAT_REQUIRE(p && g && m8 && v8 && absmax_m && absmax_v && lr_dev && step_dev, "comat_adamw8_window: null pointer");
    COMAT_REQUIRE(n >= 1 && grad_scale > 0.f, "comat_adamw8_window: n must be >= 1 and grad_scale > 0 (got %lld, %g)", (long long)n,
                  (double)grad_scale);
    COMAT_REQUIRE(accum_steps >= 1, "comat_adamw8_window: accum_steps must be >= 1 (got %d)", (int)accum_steps);
    COMAT_REQUIRE(aligned(p, 16) && aligned(g, 16) && aligned(absmax_m, 16) && aligned(absmax_v, 16) && aligned(m8, 4) && aligned(v8, 4),
                  "comat_adamw8_window: p, g and the scales must be 16-byte aligned, the codes 4-byte aligned");
    hipLaunchKernelGGL(adamw8_kernel, dim3(q8_grid(n)), dim3(NT), 0, (hipStream_t)stream, p, g, m8, v8, absmax_m, absmax_v, n, lr_dev,
                       beta1, beta2, eps, weight_decay, step_dev, gnorm_sq, max_norm, grad_scale, window, accum_steps);
    return comat_check_launch("comat_adamw8_window");
}
