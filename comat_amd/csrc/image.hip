// image.hip — image-space data movement between the VAE decoder and the BLIP captioner, plus embedding lookup.
#include "common.h"

namespace {

constexpr int NT = 256;
#define GRID_STRIDE(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < (n); i += (int64_t)gridDim.x * NT)

// Separable sparse resampling (crop + antialiased bicubic + per-channel affine in one pass).  With transposed tap
// tables the same kernel is the adjoint operator (gradient w.r.t. the source image).
__global__ __launch_bounds__(NT) void resample2d_kernel(const void* __restrict__ in, void* __restrict__ out, int B,
                                                        int Hin, int Win, int Hout, int Wout, int C,
                                                        const int32_t* __restrict__ ystart,
                                                        const float* __restrict__ ywt,
                                                        const int32_t* __restrict__ xstart,
                                                        const float* __restrict__ xwt, int KT,
                                                        const float* __restrict__ scale,
                                                        const float* __restrict__ shift, int idt, int odt) {
    const int64_t n = (int64_t)B * Hout * Wout * C;
    GRID_STRIDE(i, n) {
        const int c = (int)(i % C);
        int64_t t = i / C;
        const int ox = (int)(t % Wout);
        t /= Wout;
        const int oy = (int)(t % Hout);
        const int64_t b = t / Hout;
        const int ys = ystart[oy], xs = xstart[ox];
        float acc = 0.f;
        for (int ty = 0; ty < KT; ++ty) {
            const float wy = ywt[oy * KT + ty];
            const int sy = ys + ty;
            if (wy == 0.f || sy < 0 || sy >= Hin) continue;
            float racc = 0.f;
            for (int tx = 0; tx < KT; ++tx) {
                const float wx = xwt[ox * KT + tx];
                const int sx = xs + tx;
                if (wx == 0.f || sx < 0 || sx >= Win) continue;
                racc += wx * ld_dt(in, ((b * Hin + sy) * Win + sx) * C + c, idt);
            }
            acc += wy * racc;
        }
        const float sc = scale ? scale[c] : 1.0f, sh = shift ? shift[c] : 0.0f;
        st_dt(out, i, sc * acc + sh, odt);
    }
}

// img [B,H,W,C] <-> patches [B*(H/P)*(W/P), P*P*C] with inner order (ky, kx, c)
__global__ __launch_bounds__(NT) void patchify_kernel(const void* __restrict__ src, void* __restrict__ dst, int B, int H,
                                                      int W, int C, int P, int inverse, int dt) {
    const int64_t n = (int64_t)B * H * W * C;
    const int nW = W / P, nH = H / P;
    GRID_STRIDE(i, n) {  // i indexes the patch matrix
        const int c = (int)(i % C);
        int64_t t = i / C;
        const int kx = (int)(t % P);
        t /= P;
        const int ky = (int)(t % P);
        t /= P;
        const int pw = (int)(t % nW);
        t /= nW;
        const int ph = (int)(t % nH);
        const int64_t b = t / nH;
        const int64_t j = ((b * H + ph * P + ky) * W + pw * P + kx) * C + c;
        if (!inverse) st_dt(dst, i, ld_dt(src, j, dt), dt);
        else st_dt(dst, j, ld_dt(src, i, dt), dt);
    }
}

__global__ __launch_bounds__(NT) void embedding_kernel(const int64_t* __restrict__ ids, const void* __restrict__ table,
                                                       void* __restrict__ out, int64_t n, int dim, int64_t vocab,
                                                       int dt) {
    const int64_t total = n * dim;
    GRID_STRIDE(i, total) {
        const int64_t r = i / dim;
        const int d = (int)(i - r * dim);
        int64_t id = ids[r];
        if (id < 0) id = 0;
        if (id >= vocab) id = vocab - 1;
        st_dt(out, i, ld_dt(table, id * dim + d, dt), dt);
    }
}

__device__ __forceinline__ int64_t clamp_id(int64_t id, int64_t vocab) {  // embedding_kernel's rule
    return id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
}

// 8 consecutive elements as fp32 (16-byte loads; p + i is 16-byte aligned on this path)
__device__ __forceinline__ void ld8(const float* p, int64_t i, float* v) {
    const float4 a = *(const float4*)(p + i), b = *(const float4*)(p + i + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
__device__ __forceinline__ void ld8(const bf16_t* p, int64_t i, float* v) {
    const uint4 a = *(const uint4*)(p + i);
    const unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) v[2 * k] = __uint_as_float(w[k] << 16), v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
}
__device__ __forceinline__ void st8(float* p, int64_t i, const float* v) {
    *(float4*)(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    *(float4*)(p + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void st8(bf16_t* p, int64_t i, const float* v) {
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (unsigned)f32_to_bf16(v[2 * k]) | ((unsigned)f32_to_bf16(v[2 * k + 1]) << 16);
    *(uint4*)(p + i) = make_uint4(w[0], w[1], w[2], w[3]);
}

// out[i, :] = cast(tok[clamp(ids[i]), :] + pos[i mod L, :]): fp32 tables, one fp32 sum, one rounding.  VEC = 8: dim % 8 == 0 and
// 16-byte aligned bases (16-byte loads and stores); VEC = 1: any dim.
template <typename TO, int VEC>
__global__ __launch_bounds__(NT) void embed_fwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                                       const float* __restrict__ pos, TO* __restrict__ out, int64_t n, int L,
                                                       int dim, int64_t vocab) {
    const int per_row = dim / VEC;
    const int64_t total = n * per_row;
    GRID_STRIDE(i, total) {
        const int64_t r = i / per_row;
        const int d = (int)(i - r * per_row) * VEC;
        const int64_t id = clamp_id(ids[r], vocab);
        const int64_t p = r % L;
        if constexpr (VEC == 8) {
            float a[8], b[8];
            ld8(tok, id * dim + d, a);
            ld8(pos, p * dim + d, b);
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] += b[k];
            st8(out, r * dim + d, a);
        } else {
            stf<TO>(out + r * dim + d, tok[id * dim + d] + pos[p * dim + d]);
        }
    }
}

// dtable[v, :] += sum over {i : clamp(ids[i]) = v} of dy[i, :], without atomics and in ONE order: block (i, chunk) leaves at once
// when id(i) occurred at a smaller index; the block of the first occurrence adds the rows of all occurrences to 0 in ascending i
// (fp32) and adds that sum once to the row.  Wave 0 finds the occurrences: it walks the ids in 64s, a ballot gives every matching
// lane its place in the ordered list (LDS).  Rows named by no id are not touched.  n <= COMAT_EMBED_GRAD_MAX_N (the list).
constexpr int EG_NT = 128;
constexpr int EG_SCAN = 4;  // id chunks whose loads are issued together
constexpr int EG_ROWS = 8;  // rows of dy whose loads are issued together (the end token's row repeats hundreds of times)
template <typename TG, int VEC>
__global__ __launch_bounds__(EG_NT) void embed_grad_kernel(const int64_t* __restrict__ ids, const TG* __restrict__ dy,
                                                           float* __restrict__ dtable, int n, int dim, int64_t vocab) {
    __shared__ int s_list[COMAT_EMBED_GRAD_MAX_N];
    __shared__ int s_count;  // number of occurrences, 0: this block's id occurred before
    const int i = blockIdx.x;
    const int64_t v = clamp_id(ids[i], vocab);
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const unsigned long long lower = (1ull << lane) - 1;
        int cnt = 0;
        bool dup = false;
        for (int base = 0; base < n && !dup; base += 64 * EG_SCAN) {
            bool m[EG_SCAN];
#pragma unroll
            for (int u = 0; u < EG_SCAN; ++u) {
                const int j = base + 64 * u + lane;
                m[u] = j < n && clamp_id(ids[j], vocab) == v;
            }
#pragma unroll
            for (int u = 0; u < EG_SCAN; ++u) {
                const int b0 = base + 64 * u;
                const unsigned long long mask = __ballot(m[u]);
                if (b0 < i) {  // the lanes of indices below i
                    const unsigned long long below = i - b0 >= 64 ? ~0ull : (1ull << (i - b0)) - 1;
                    if (mask & below) {
                        dup = true;
                        break;
                    }
                }
                if (m[u]) s_list[cnt + __popcll(mask & lower)] = b0 + lane;
                cnt += __popcll(mask);
            }
        }
        if (lane == 0) s_count = dup ? 0 : cnt;
    }
    __syncthreads();
    const int cnt = s_count;
    if (cnt == 0) return;
    const int d = (blockIdx.y * EG_NT + threadIdx.x) * VEC;
    if (d >= dim) return;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    int k = 0;
    for (; k + EG_ROWS <= cnt; k += EG_ROWS) {  // EG_ROWS rows in flight, added in list order
        float r[EG_ROWS][VEC];
#pragma unroll
        for (int u = 0; u < EG_ROWS; ++u) {
            const int64_t o = (int64_t)s_list[k + u] * dim + d;
            if constexpr (VEC == 8) ld8(dy, o, r[u]); else r[u][0] = ldf<TG>(dy + o);
        }
#pragma unroll
        for (int u = 0; u < EG_ROWS; ++u)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += r[u][e];
    }
    for (; k < cnt; ++k) {
        float r[VEC];
        const int64_t o = (int64_t)s_list[k] * dim + d;
        if constexpr (VEC == 8) ld8(dy, o, r); else r[0] = ldf<TG>(dy + o);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += r[e];
    }
    const int64_t o = v * dim + d;
    if constexpr (VEC == 8) {
        float t[8];
        ld8(dtable, o, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] += acc[e];
        st8(dtable, o, t);
    } else {
        dtable[o] += acc[0];
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- decoded image tokens -> bytes (comat_image_u8) ------------------------------------------------------------------------
// One element: the byte of include/comat_hip.h, every step its own fp32 rounding (__fmul_rn / __fadd_rn: no contraction into an
// fma - the multiply by 255 folded into the affine gives other bytes).  `nonfinite` is raised by an Inf or NaN INPUT.
__device__ __forceinline__ unsigned u8_of(float x, int denorm, bool& nonfinite) {
    nonfinite |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
    float v = denorm ? __fadd_rn(__fmul_rn(x, 0.5f), 0.5f) : x;
    if (!(v >= 0.f)) v = 0.f;  // negatives, -Inf and NaN
    if (v > 1.f) v = 1.f;      // +Inf too
    return (unsigned)(int)rintf(__fmul_rn(v, 255.0f));  // round half to even; 0 .. 255
}

template <typename T> struct U8Chunk;  // E: elements of a 16-byte load = result bytes of one store
template <> struct U8Chunk<float> { static constexpr int E = 4; };
template <> struct U8Chunk<bf16_t> { static constexpr int E = 8; };

__device__ __forceinline__ void ld_chunk(const float* p, float* v) {
    const float4 a = *(const float4*)p;
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
}
__device__ __forceinline__ void ld_chunk(const bf16_t* p, float* v) { ld8(p, 0, v); }
__device__ __forceinline__ void st_chunk(uint8_t* p, const unsigned* w, float) { *(unsigned*)p = w[0]; }
__device__ __forceinline__ void st_chunk(uint8_t* p, const unsigned* w, bf16_t) { *(uint2*)p = make_uint2(w[0], w[1]); }

// Block row blockIdx.y (+ k * gridDim.y) is one image row: n = W * C consecutive source elements, n consecutive destination bytes.
// A row whose first 16-byte aligned source element meets an E-byte aligned destination byte (`head` elements in, the same count on
// both sides) is cut into slots: slot 0 the head, slots 1 .. nvec one 16-byte load and one E-byte store each, slot nvec + 1 the
// tail; any other row gives slot s its elements [s * E, s * E + E), one at a time.  Head, tail and such rows run u8_of element by
// element: the same bits.  slots = ceil(n / E) + 1 covers either cut.  No LDS, no atomics; bad[b] gets plain stores of 1.
template <typename T>
__global__ __launch_bounds__(NT) void image_u8_kernel(const T* __restrict__ x, uint8_t* __restrict__ out,
                                                      int32_t* __restrict__ bad, int rows, int H, int n, int denorm,
                                                      int64_t pitch, int cols, int pad, int64_t cell, int64_t left, int slots) {
    constexpr int E = U8Chunk<T>::E;
    const int slot = blockIdx.x * NT + threadIdx.x;
    if (slot >= slots) return;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const int b = r / H, y = r - b * H;
        const T* src = x + (int64_t)r * n;
        uint8_t* dst = out + ((int64_t)pad + (int64_t)(b / cols) * (H + pad) + y) * pitch + left + (int64_t)(b % cols) * cell;
        const uintptr_t sa = (uintptr_t)src, da = (uintptr_t)dst;
        const int hs = (int)(((16 - (sa & 15)) & 15) / sizeof(T)), hd = (int)((E - (da & (E - 1))) & (E - 1));
        const bool cut = sa % sizeof(T) == 0 && hs == hd;
        const int head = cut ? (hs < n ? hs : n) : 0;
        const int nvec = cut ? (n - head) / E : 0;
        bool nonfinite = false;
        if (cut && slot >= 1 && slot <= nvec) {
            const int i = head + (slot - 1) * E;
            float v[E];
            ld_chunk(src + i, v);
            unsigned w[E / 4];
#pragma unroll
            for (int q = 0; q < E / 4; ++q)
                w[q] = u8_of(v[4 * q], denorm, nonfinite) | (u8_of(v[4 * q + 1], denorm, nonfinite) << 8) |
                       (u8_of(v[4 * q + 2], denorm, nonfinite) << 16) | (u8_of(v[4 * q + 3], denorm, nonfinite) << 24);
            st_chunk(dst + i, w, T());
        } else {
            int lo, hi;
            if (!cut) lo = slot * E, hi = lo + E;
            else if (slot == 0) lo = 0, hi = head;
            else if (slot == nvec + 1) lo = head + nvec * E, hi = n;
            else lo = hi = 0;
            if (hi > n) hi = n;
            for (int i = lo; i < hi; ++i) dst[i] = (uint8_t)u8_of(ldf<T>(src + i), denorm, nonfinite);
        }
        if (nonfinite && bad) bad[b] = 1;
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int comat_resample2d(const void* in, void* out, int32_t B, int32_t Hin, int32_t Win, int32_t Hout,
                                int32_t Wout, int32_t C, const int32_t* ystart, const float* ywt, const int32_t* xstart,
                                const float* xwt, int32_t KT, const float* scale, const float* shift, int32_t in_dtype,
                                int32_t out_dtype, void* stream) {
    COMAT_REQUIRE(in && out && ystart && ywt && xstart && xwt, "comat_resample2d: null pointer");
    COMAT_REQUIRE(B > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && C > 0 && KT > 0, "comat_resample2d: bad shape");
    COMAT_REQUIRE(dtype_ok(in_dtype) && dtype_ok(out_dtype), "comat_resample2d: bad dtype");
    hipLaunchKernelGGL(resample2d_kernel, dim3(grid_1d((int64_t)B * Hout * Wout * C, NT)), dim3(NT), 0, ST, in, out, B,
                       Hin, Win, Hout, Wout, C, ystart, ywt, xstart, xwt, KT, scale, shift, in_dtype, out_dtype);
    return comat_check_launch("comat_resample2d");
}

extern "C" int comat_patchify(const void* img, void* patches, int32_t B, int32_t H, int32_t W, int32_t C, int32_t P,
                              int32_t inverse, int32_t dtype, void* stream) {
    COMAT_REQUIRE(img && patches, "comat_patchify: null pointer");
    COMAT_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && P > 0 && H % P == 0 && W % P == 0, "comat_patchify: bad shape");
    COMAT_REQUIRE(dtype_ok(dtype), "comat_patchify: bad dtype");
    // forward: src = img, dst = patches; inverse: src = patches, dst = img
    const void* src = inverse ? patches : img;
    void* dst = inverse ? (void*)img : patches;
    hipLaunchKernelGGL(patchify_kernel, dim3(grid_1d((int64_t)B * H * W * C, NT)), dim3(NT), 0, ST, src, dst, B, H, W, C,
                       P, inverse, dtype);
    return comat_check_launch("comat_patchify");
}

extern "C" int comat_embedding(const int64_t* ids, const void* table, void* out, int64_t n, int32_t dim, int64_t vocab,
                               int32_t dtype, void* stream) {
    COMAT_REQUIRE(ids && table && out && n > 0 && dim > 0 && vocab > 0 && dtype_ok(dtype), "comat_embedding: bad args");
    hipLaunchKernelGGL(embedding_kernel, dim3(grid_1d(n * dim, NT)), dim3(NT), 0, ST, ids, table, out, n, dim, vocab,
                       dtype);
    return comat_check_launch("comat_embedding");
}

extern "C" int comat_embed_fwd(const int64_t* ids, const float* tok, const float* pos, void* out, int64_t n, int32_t L,
                               int32_t dim, int64_t vocab, int32_t npos, int32_t out_dtype, void* stream) {
    COMAT_REQUIRE(ids && tok && pos && out, "comat_embed_fwd: null pointer");
    COMAT_REQUIRE(n > 0 && dim > 0 && vocab > 0 && L > 0 && L <= npos, "comat_embed_fwd: bad shape (n %lld, dim %d, vocab %lld, L %d, "
                  "npos %d)", (long long)n, dim, (long long)vocab, L, npos);
    COMAT_REQUIRE(dtype_ok(out_dtype), "comat_embed_fwd: bad dtype");
    const bool vec = dim % 8 == 0 && aligned16(tok) && aligned16(pos) && aligned16(out);
    const dim3 grid(grid_1d(n * (vec ? dim / 8 : dim), NT)), block(NT);
#define COMAT_EMBED_FWD(TO, VEC) \
    hipLaunchKernelGGL((embed_fwd_kernel<TO, VEC>), grid, block, 0, ST, ids, tok, pos, (TO*)out, n, L, dim, vocab)
    if (out_dtype == COMAT_BF16) {
        if (vec) COMAT_EMBED_FWD(bf16_t, 8); else COMAT_EMBED_FWD(bf16_t, 1);
    } else {
        if (vec) COMAT_EMBED_FWD(float, 8); else COMAT_EMBED_FWD(float, 1);
    }
#undef COMAT_EMBED_FWD
    return comat_check_launch("comat_embed_fwd");
}

extern "C" int comat_embed_grad(const int64_t* ids, const void* dy, float* dtable, int64_t n, int32_t dim, int64_t vocab,
                                int32_t dy_dtype, void* stream) {
    COMAT_REQUIRE(ids && dy && dtable, "comat_embed_grad: null pointer");
    COMAT_REQUIRE(n > 0 && dim > 0 && vocab > 0, "comat_embed_grad: bad shape (n %lld, dim %d, vocab %lld)", (long long)n, dim,
                  (long long)vocab);
    COMAT_REQUIRE(n <= COMAT_EMBED_GRAD_MAX_N, "comat_embed_grad: n = %lld, at most %d ids per launch", (long long)n,
                  COMAT_EMBED_GRAD_MAX_N);
    COMAT_REQUIRE(dtype_ok(dy_dtype), "comat_embed_grad: bad dtype");
    const bool vec = dim % 8 == 0 && aligned16(dy) && aligned16(dtable);
    const int64_t chunks = cdiv64(vec ? dim / 8 : dim, EG_NT);
    COMAT_REQUIRE(chunks <= 65535, "comat_embed_grad: dim %d too large", dim);
    const dim3 grid((unsigned)n, (unsigned)chunks), block(EG_NT);
#define COMAT_EMBED_GRAD(TG, VEC) \
    hipLaunchKernelGGL((embed_grad_kernel<TG, VEC>), grid, block, 0, ST, ids, (const TG*)dy, dtable, (int)n, dim, vocab)
    if (dy_dtype == COMAT_BF16) {
        if (vec) COMAT_EMBED_GRAD(bf16_t, 8); else COMAT_EMBED_GRAD(bf16_t, 1);
    } else {
        if (vec) COMAT_EMBED_GRAD(float, 8); else COMAT_EMBED_GRAD(float, 1);
    }
#undef COMAT_EMBED_GRAD
    return comat_check_launch("comat_embed_grad");
}

extern "C" int comat_image_u8(const void* x, uint8_t* out, int32_t* bad, int32_t B, int32_t H, int32_t W, int32_t C,
                              int32_t dtype, int32_t denorm, int64_t out_pitch, int32_t cols, int32_t pad, void* stream) {
    COMAT_REQUIRE(x && out, "comat_image_u8: null pointer");
    COMAT_REQUIRE(B > 0 && H > 0 && W > 0, "comat_image_u8: bad shape (B %d, H %d, W %d must be positive)", B, H, W);
    COMAT_REQUIRE(C >= 1 && C <= 4, "comat_image_u8: C = %d, 1 to 4 channels", C);
    COMAT_REQUIRE(dtype_ok(dtype), "comat_image_u8: bad dtype");
    COMAT_REQUIRE(cols >= 1, "comat_image_u8: cols = %d, at least one image a sheet row", cols);
    COMAT_REQUIRE(pad >= 0, "comat_image_u8: pad = %d must not be negative", pad);
    const int64_t n = (int64_t)W * C, cell = ((int64_t)W + pad) * C, left = (int64_t)pad * C;
    const int64_t used = B < cols ? B : cols;  // images in the fullest sheet row
    const int64_t widest = left + (used - 1) * cell + n;
    COMAT_REQUIRE(out_pitch >= widest, "comat_image_u8: out_pitch = %lld, the widest row written has %lld bytes", (long long)out_pitch,
                  (long long)widest);
    const int64_t rows = (int64_t)B * H;
    COMAT_REQUIRE(rows <= INT32_MAX && n <= INT32_MAX - 16, "comat_image_u8: bad shape (B * H or W * C beyond 2^31)");
    const int E = dtype == COMAT_BF16 ? 8 : 4;
    const int slots = (int)cdiv64(n, E) + 1;
    const dim3 grid((unsigned)cdiv64(slots, NT), (unsigned)(rows < 65535 ? rows : 65535)), block(NT);
#define COMAT_IMAGE_U8(T)                                                                                                       \
    hipLaunchKernelGGL((image_u8_kernel<T>), grid, block, 0, ST, (const T*)x, out, bad, (int)rows, H, (int)n, denorm != 0, \
                       out_pitch, cols, pad, cell, left, slots)
    if (dtype == COMAT_BF16) COMAT_IMAGE_U8(bf16_t); else COMAT_IMAGE_U8(float);
#undef COMAT_IMAGE_U8
    return comat_check_launch("comat_image_u8");
}
