// attrcon.hip — the attribute-concentration loss as device work (StepConfig.attrcon_on_device): the object-mask resize and a
// batched gather / loss / gradient family over the captured cross-attention maps, driven by ragged per-sample tables that live
// in device memory (include/comat_hip.h, "attribute concentration on the device").  The per-sample kernels of loss.hip
// (comat_attnmap_gather_*) stay as they are; these take the whole batch, read the token counts on the device and leave the
// remaining arithmetic of losses.grounding_loss_by_layer to one small launch instead of host-side torch operators.
// No floating-point atomics: every sum runs in a fixed order (partials in the caller's workspace, then a second stage).
#include "common.h"

namespace {

constexpr int NT = 256;

// ---- mask resize: out = 1 iff a source pixel inside the window of positive-weight taps is set -----------------------------
// Grid (output row, mask).  Phase 1 folds the rows [ylo, yhi) of the window into one row of column flags in LDS (integer OR:
// any order gives the same bits), 16 source bytes per load where the row starts on a 16-byte boundary; phase 2 folds each
// output pixel's columns [xlo, xhi).
__global__ __launch_bounds__(NT) void mask_resize_any_kernel(const uint8_t* __restrict__ masks, const int32_t* __restrict__ ylo,
                                                             const int32_t* __restrict__ yhi, const int32_t* __restrict__ xlo,
                                                             const int32_t* __restrict__ xhi, float* __restrict__ out, int H,
                                                             int W, int res) {
    extern __shared__ __attribute__((aligned(16))) char tile[];
    uint32_t* col = (uint32_t*)tile;  // ceil(W / 16) * 4 words: byte x is column x's flag
    const int oy = blockIdx.x;
    const int64_t obj = blockIdx.y;
    const int nchunk = (W + 15) >> 4;
    for (int i = threadIdx.x; i < nchunk * 4; i += NT) col[i] = 0u;
    __syncthreads();
    const int y0 = max(ylo[oy], 0), y1 = min(yhi[oy], H);
    const uint8_t* src = masks + obj * H * W;
    const int items = max(y1 - y0, 0) * nchunk;
    for (int it = threadIdx.x; it < items; it += NT) {
        const int y = y0 + it / nchunk, c = it % nchunk;
        const uint8_t* row = src + (int64_t)y * W;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (c * 16 + 16 <= W && ((uintptr_t)row & 15) == 0) {
            const uint4 v = *(const uint4*)(row + c * 16);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
            const int n = min(16, W - c * 16);
            for (int e = 0; e < n; ++e) w[e >> 2] |= (uint32_t)row[c * 16 + e] << ((e & 3) * 8);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (w[k]) atomicOr(&col[c * 4 + k], w[k]);  // LDS integer OR (masks are sparse: most words are skipped)
    }
    __syncthreads();
    const uint8_t* cb = (const uint8_t*)col;
    for (int ox = threadIdx.x; ox < res; ox += NT) {
        const int x0 = max(xlo[ox], 0), x1 = min(xhi[ox], W);
        uint32_t any = 0u;
        for (int x = x0; x < x1; ++x) any |= cb[x];
        out[(obj * res + oy) * res + ox] = any ? 1.0f : 0.0f;
    }
}

// ---- batched gather over one captured map [bs * heads, npix, L] -------------------------------------------------------------
// Tables (device memory): n_obj[bs], n_tok[bs]; tok_idx, tok_obj, inv_len [bs, TOK]; masks [bs, OBJ, npix] fp32 {0,1}.
// A sample with n_obj = 0 has no tokens: its blocks leave at once.
__device__ __forceinline__ int sample_tokens(const int32_t* n_obj, const int32_t* n_tok, int b, int TOK) {
    return n_obj[b] > 0 ? min(max(n_tok[b], 0), TOK) : 0;
}

// Grid (256-pixel chunk, head, sample).  ws = [bs, nblk, heads, TOK, 2] partial (masked sum, sum), then [bs, heads, TOK, npix]
// per-head values; attrcon_gather_final_kernel combines both in a fixed order.
__global__ __launch_bounds__(NT) void attrcon_gather_kernel(const void* __restrict__ amap, const float* __restrict__ masks,
                                                            const int32_t* __restrict__ n_obj, const int32_t* __restrict__ n_tok,
                                                            const int32_t* __restrict__ tok_idx,
                                                            const int32_t* __restrict__ tok_obj, float* __restrict__ ws, int bs,
                                                            int heads, int npix, int L, int OBJ, int TOK, int dt) {
    __shared__ float sbuf[4];
    const int h = blockIdx.y, b = blockIdx.z;
    const int nt = sample_tokens(n_obj, n_tok, b, TOK);
    if (nt == 0) return;
    const int px = blockIdx.x * NT + threadIdx.x;
    const int64_t nblk = gridDim.x;
    float* wsp = ws + (((int64_t)b * nblk + blockIdx.x) * heads + h) * TOK * 2;
    float* wsv = ws + (int64_t)bs * nblk * heads * TOK * 2 + ((int64_t)b * heads + h) * TOK * npix;
    const float* mk = masks + (int64_t)b * OBJ * npix;
    for (int t = 0; t < nt; ++t) {
        const int c = tok_idx[b * TOK + t], o = min(max(tok_obj[b * TOK + t], 0), OBJ - 1);
        float v = 0.f, vm = 0.f;
        if (px < npix && (unsigned)c < (unsigned)L) {
            v = ld_dt(amap, (((int64_t)b * heads + h) * npix + px) * L + c, dt);
            vm = v * mk[(int64_t)o * npix + px];
        }
        if (px < npix) wsv[(int64_t)t * npix + px] = v;
        const float sn = block_sum_256(vm, sbuf);
        const float sd = block_sum_256(v, sbuf);
        if (threadIdx.x == 0) {
            wsp[t * 2] = sn;
            wsp[t * 2 + 1] = sd;
        }
    }
}

// The same pass with the block's RPB rows of the map staged through LDS by 16-byte loads (loss.hip: attnmap_fwd_lds_kernel);
// the host launches it when every block's row chunk starts on a 16-byte boundary and is a whole number of 16-byte vectors.
template <typename T, int RPB>
__global__ __launch_bounds__(NT) void attrcon_gather_lds_kernel(const T* __restrict__ amap, const float* __restrict__ masks,
                                                                const int32_t* __restrict__ n_obj,
                                                                const int32_t* __restrict__ n_tok,
                                                                const int32_t* __restrict__ tok_idx,
                                                                const int32_t* __restrict__ tok_obj, float* __restrict__ ws,
                                                                int bs, int heads, int npix, int L, int OBJ, int TOK) {
    extern __shared__ __attribute__((aligned(16))) char tile[];
    float* sbuf = (float*)tile;  // 4 floats for the block reductions, then the rows (16-byte aligned)
    T* rows = (T*)(tile + 16);
    const int h = blockIdx.y, b = blockIdx.z;
    const int nt = sample_tokens(n_obj, n_tok, b, TOK);
    if (nt == 0) return;
    const int px0 = blockIdx.x * RPB;
    const int nrows = min(RPB, npix - px0);
    const int64_t nbytes = (int64_t)nrows * L * (int)sizeof(T);  // host: a multiple of 16
    const char* src = (const char*)(amap + (((int64_t)b * heads + h) * npix + px0) * L);
    for (int64_t o = (int64_t)threadIdx.x * 16; o < nbytes; o += (int64_t)NT * 16)
        *(uint4*)((char*)rows + o) = *(const uint4*)(src + o);
    __syncthreads();
    const int px = px0 + threadIdx.x;
    const bool act = (int)threadIdx.x < nrows;
    const int64_t nblk = gridDim.x;
    float* wsp = ws + (((int64_t)b * nblk + blockIdx.x) * heads + h) * TOK * 2;
    float* wsv = ws + (int64_t)bs * nblk * heads * TOK * 2 + ((int64_t)b * heads + h) * TOK * npix;
    const float* mk = masks + (int64_t)b * OBJ * npix;
    for (int t = 0; t < nt; ++t) {
        const int c = tok_idx[b * TOK + t], o = min(max(tok_obj[b * TOK + t], 0), OBJ - 1);
        float v = 0.f, vm = 0.f;
        if (act) {
            if ((unsigned)c < (unsigned)L) {
                v = ldf<T>(rows + (int64_t)threadIdx.x * L + c);
                vm = v * mk[(int64_t)o * npix + px];
            }
            wsv[(int64_t)t * npix + px] = v;
        }
        const float sn = block_sum_256(vm, sbuf);
        const float sd = block_sum_256(v, sbuf);
        if (threadIdx.x == 0) {
            wsp[t * 2] = sn;
            wsp[t * 2 + 1] = sd;
        }
    }
}

// num[b,h,t] = sum_blk partial, den likewise (blocks in ascending order); avg[b,t,px] += (1/heads) sum_h value (ascending h).
// Grid (chunk of max(heads * TOK, TOK * npix), sample).
__global__ __launch_bounds__(NT) void attrcon_gather_final_kernel(const float* __restrict__ ws, const int32_t* __restrict__ n_obj,
                                                                  const int32_t* __restrict__ n_tok, int nblk, int bs, int heads,
                                                                  int npix, int TOK, float* __restrict__ num,
                                                                  float* __restrict__ den, float* __restrict__ avg) {
    const int b = blockIdx.y;
    const int nt = sample_tokens(n_obj, n_tok, b, TOK);
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int ht = heads * TOK;
    if (i < ht && (int)(i % TOK) < nt) {
        const float* p = ws + (int64_t)b * nblk * ht * 2;
        float a = 0.f, d = 0.f;
        for (int k = 0; k < nblk; ++k) {
            a += p[((int64_t)k * ht + i) * 2];
            d += p[((int64_t)k * ht + i) * 2 + 1];
        }
        num[(int64_t)b * ht + i] = a;
        den[(int64_t)b * ht + i] = d;
    }
    const int64_t tp = (int64_t)TOK * npix;
    if (i < tp && (int)(i / npix) < nt) {
        const float* wsv = ws + (int64_t)bs * nblk * ht * 2 + (int64_t)b * heads * tp;
        float a = 0.f;
        for (int h = 0; h < heads; ++h) a += wsv[(int64_t)h * tp + i];
        avg[(int64_t)b * tp + i] += a / heads;
    }
}

// ---- loss of one (timestep, layer): M maps' num / den [M, bs, heads, TOK], avg [bs, TOK, npix] ------------------------------
// losses._bce on one probability: the logarithms clamped at -100 (a NaN is not below -100: it is carried), the derivative zero
// where a clamp is active, a NaN probability carried into it
__device__ __forceinline__ void bce_term(float p, float t, float* loss, float* dp) {
    const float lp = logf(p), lq = logf(1.0f - p);
    const float cp = lp < -100.0f ? -100.0f : lp, cq = lq < -100.0f ? -100.0f : lq;
    *loss = (t - 1.0f) * cq - t * cp;
    const float nanp = p != p ? p : 0.0f;
    const float dcp = lp >= -100.0f ? 1.0f / p : nanp;            // d clamp(log p) / dp
    const float dcq = lq >= -100.0f ? -1.0f / (1.0f - p) : nanp;  // d clamp(log(1 - p)) / dp
    *dp = (t - 1.0f) * dcq - t * dcp;
}

// Grid (256-pixel chunk, sample): pixel loss.  word[i, px] = sum over the tokens of object i (ascending t) of avg[t, px] / M;
// the block's sum of bce(word, mask) / (n_obj npix bs) goes to part[b, blk]; g_avg[b, t, px] = that weight * dbce / M.
__global__ __launch_bounds__(NT) void attrcon_pixel_kernel(const float* __restrict__ avg, const float* __restrict__ masks,
                                                           const int32_t* __restrict__ n_obj, const int32_t* __restrict__ n_tok,
                                                           const int32_t* __restrict__ tok_obj, float* __restrict__ g_avg,
                                                           float* __restrict__ part, int M, int bs, int npix, int OBJ, int TOK) {
    __shared__ float sbuf[4];
    const int b = blockIdx.y;
    const int nt = sample_tokens(n_obj, n_tok, b, TOK);
    const int no = nt > 0 ? min(n_obj[b], OBJ) : 0;  // (an object without tokens still counts: its word is 0)
    const int px = blockIdx.x * NT + threadIdx.x;
    float acc = 0.f;
    if (no > 0 && px < npix) {
        const float wgt = 1.0f / ((float)no * (float)npix * (float)bs), inv_m = 1.0f / (float)M;
        const float* av = avg + (int64_t)b * TOK * npix + px;
        float* ga = g_avg + (int64_t)b * TOK * npix + px;
        const int32_t* to = tok_obj + b * TOK;
        for (int i = 0; i < no; ++i) {
            float word = 0.f;
            for (int t = 0; t < nt; ++t)
                if (to[t] == i) word += av[(int64_t)t * npix];
            word *= inv_m;
            float l, d;
            bce_term(word, masks[((int64_t)b * OBJ + i) * npix + px], &l, &d);
            acc += l;
            d *= wgt * inv_m;
            for (int t = 0; t < nt; ++t)
                if (to[t] == i) ga[(int64_t)t * npix] = d;
        }
        acc *= wgt;
    }
    acc = block_sum_256(acc, sbuf);
    if (threadIdx.x == 0) part[(int64_t)b * gridDim.x + blockIdx.x] = acc;
}

// One block.  Token loss: item (m, b, t) -> act = mean_h num / den, term = inv_len (1 - act)^2 / (n_obj bs), its derivatives to
// g_num / g_den; items and the pixel partials are taken thread-strided and folded by the block sum (a fixed order).
// out[0] = token loss, out[1] = pixel loss, both summed over the samples and divided by bs.
__global__ __launch_bounds__(NT) void attrcon_token_kernel(const float* __restrict__ num, const float* __restrict__ den,
                                                           const int32_t* __restrict__ n_obj, const int32_t* __restrict__ n_tok,
                                                           const float* __restrict__ inv_len, const float* __restrict__ part,
                                                           int nparts, float* __restrict__ g_num, float* __restrict__ g_den,
                                                           float* __restrict__ out, int M, int bs, int heads, int TOK) {
    __shared__ float sbuf[4];
    float tl = 0.f, pl = 0.f;
    const int items = M * bs * TOK;
    for (int it = threadIdx.x; it < items; it += NT) {
        const int t = it % TOK, b = (it / TOK) % bs, m = it / (TOK * bs);
        if (t >= sample_tokens(n_obj, n_tok, b, TOK)) continue;
        const int64_t base = (((int64_t)m * bs + b) * heads) * TOK + t;
        float act = 0.f;
        for (int h = 0; h < heads; ++h) act += num[base + (int64_t)h * TOK] / den[base + (int64_t)h * TOK];
        act /= heads;
        const float w = inv_len[b * TOK + t] / ((float)n_obj[b] * (float)bs);
        tl += w * (1.0f - act) * (1.0f - act);
        const float ga = -2.0f * w * (1.0f - act) / heads;  // d loss / d (num / den) of every head
        for (int h = 0; h < heads; ++h) {
            const float n = num[base + (int64_t)h * TOK], d = den[base + (int64_t)h * TOK];
            g_num[base + (int64_t)h * TOK] = ga / d;
            g_den[base + (int64_t)h * TOK] = -ga * n / (d * d);
        }
    }
    for (int i = threadIdx.x; i < nparts; i += NT) pl += part[i];
    tl = block_sum_256(tl, sbuf);
    pl = block_sum_256(pl, sbuf);
    if (threadIdx.x == 0) {
        out[0] = tl;
        out[1] = pl;
    }
}

// ---- dense gradient of one map ---------------------------------------------------------------------------------------------
// value of token t at (h, px): go[0] (g_num[h, t] mask[obj_t, px] + g_den[h, t]) + go[1] g_avg[t, px] / heads
__device__ __forceinline__ float attrcon_grad(const float* g_num, const float* g_den, const float* g_avg, const float* mk,
                                              int64_t ht, int64_t t, int o, int npix, int px, float go_t, float go_p,
                                              float inv_h) {
    return go_t * (g_num[ht] * mk[(int64_t)o * npix + px] + g_den[ht]) + go_p * g_avg[t * npix + px] * inv_h;
}

// Grid (RPB-row chunk, head, sample): the block builds its dense rows in LDS (zeros + the token columns, accumulated in fp32 in
// ascending t, so a column named twice adds up) and writes them as one stream of 16-byte stores (loss.hip:
// attnmap_bwd_lds_kernel).  A sample with n_obj = 0 has no tokens: its rows are written as zeros.
template <typename T, int RPB>
__global__ __launch_bounds__(NT) void attrcon_bwd_lds_kernel(const float* __restrict__ g_num, const float* __restrict__ g_den,
                                                             const float* __restrict__ g_avg, const float* __restrict__ masks,
                                                             const int32_t* __restrict__ n_obj, const int32_t* __restrict__ n_tok,
                                                             const int32_t* __restrict__ tok_idx,
                                                             const int32_t* __restrict__ tok_obj, const float* __restrict__ go,
                                                             T* __restrict__ damap, int heads, int npix, int L, int OBJ, int TOK) {
    extern __shared__ __attribute__((aligned(16))) char tile[];
    float* acc = (float*)tile;  // [RPB][L]
    const int h = blockIdx.y, b = blockIdx.z;
    const int nt = sample_tokens(n_obj, n_tok, b, TOK);
    const int px0 = blockIdx.x * RPB;
    const int nrows = min(RPB, npix - px0);
    for (int i = threadIdx.x; i < nrows * L; i += NT) acc[i] = 0.f;
    __syncthreads();
    const int px = px0 + threadIdx.x;
    if ((int)threadIdx.x < nrows && nt > 0) {
        const float inv_h = 1.0f / heads, go_t = go[0], go_p = go[1];
        const float* mk = masks + (int64_t)b * OBJ * npix;
        const float* ga = g_avg + (int64_t)b * TOK * npix;
        for (int t = 0; t < nt; ++t) {
            const int c = tok_idx[b * TOK + t], o = min(max(tok_obj[b * TOK + t], 0), OBJ - 1);
            if ((unsigned)c < (unsigned)L)
                acc[threadIdx.x * L + c] += attrcon_grad(g_num, g_den, ga, mk, ((int64_t)b * heads + h) * TOK + t, t, o, npix, px,
                                                         go_t, go_p, inv_h);
        }
    }
    __syncthreads();
    T* dst = damap + (((int64_t)b * heads + h) * npix + px0) * L;
    if (sizeof(T) == 4) {
        const int64_t nbytes = (int64_t)nrows * L * 4;  // host: a multiple of 16
        for (int64_t o = (int64_t)threadIdx.x * 16; o < nbytes; o += (int64_t)NT * 16)
            *(uint4*)((char*)dst + o) = *(const uint4*)((const char*)acc + o);
    } else {
        const int n8 = nrows * L / 8;  // host: (nrows * L) % 8 == 0
        for (int i = threadIdx.x; i < n8; i += NT) {
            union { uint4 u; bf16_t hh[8]; } pk;
#pragma unroll
            for (int e = 0; e < 8; ++e) pk.hh[e] = f32_to_bf16(acc[i * 8 + e]);
            *(uint4*)((bf16_t*)dst + (int64_t)i * 8) = pk.u;
        }
    }
}

// The plain form (row chunks that do not vectorise): one thread per row writes its L elements, each the sum over the tokens
// that name the column in ascending t - the same order as the LDS form, so the two give the same bits.
__global__ __launch_bounds__(NT) void attrcon_bwd_kernel(const float* __restrict__ g_num, const float* __restrict__ g_den,
                                                         const float* __restrict__ g_avg, const float* __restrict__ masks,
                                                         const int32_t* __restrict__ n_obj, const int32_t* __restrict__ n_tok,
                                                         const int32_t* __restrict__ tok_idx, const int32_t* __restrict__ tok_obj,
                                                         const float* __restrict__ go, void* __restrict__ damap, int heads,
                                                         int npix, int L, int OBJ, int TOK, int dt) {
    const int h = blockIdx.y, b = blockIdx.z;
    const int px = blockIdx.x * NT + threadIdx.x;
    if (px >= npix) return;
    const int nt = sample_tokens(n_obj, n_tok, b, TOK);
    const float inv_h = 1.0f / heads, go_t = go[0], go_p = go[1];
    const float* mk = masks + (int64_t)b * OBJ * npix;
    const float* ga = g_avg + (int64_t)b * TOK * npix;
    const int64_t row = (((int64_t)b * heads + h) * npix + px) * L;
    for (int c = 0; c < L; ++c) {
        float g = 0.f;
        for (int t = 0; t < nt; ++t)
            if (tok_idx[b * TOK + t] == c) {
                const int o = min(max(tok_obj[b * TOK + t], 0), OBJ - 1);
                g += attrcon_grad(g_num, g_den, ga, mk, ((int64_t)b * heads + h) * TOK + t, t, o, npix, px, go_t, go_p, inv_h);
            }
        st_dt(damap, row + c, g, dt);
    }
}

constexpr int RPB16 = 256, RPB32 = 128;  // rows per block of the staged gather (bf16 / fp32 maps)
constexpr int RPBB = 128;                // rows per block of the staged gradient writer (fp32 accumulation tile)

// every block's row chunk of a [bs * heads, npix, L] map starts on a 16-byte boundary, is a whole number of 16-byte vectors
// and fits the LDS tile
bool chunks_vectorise(const void* p, int npix, int L, int es, int rpb, int64_t lds_bytes) {
    return ((uintptr_t)p % 16) == 0 && ((int64_t)npix * L * es) % 16 == 0 && ((int64_t)rpb * L * es) % 16 == 0 &&
           ((int64_t)(npix % rpb) * L * es) % 16 == 0 && lds_bytes <= 64 * 1024;
}

int gather_blocks(const void* amap, int npix, int L, int dtype, bool* staged) {
    const int es = dtype == COMAT_BF16 ? 2 : 4, rpb = dtype == COMAT_BF16 ? RPB16 : RPB32;
    *staged = chunks_vectorise(amap, npix, L, es, rpb, (int64_t)rpb * L * es + 16);
    return *staged ? (npix + rpb - 1) / rpb : (npix + NT - 1) / NT;
}

int attrcon_shape_check(const char* who, int32_t bs, int32_t heads, int32_t npix, int32_t L, int32_t OBJ, int32_t TOK) {
    COMAT_REQUIRE(bs > 0 && bs <= 65535 && heads > 0 && heads <= 65535 && npix > 0 && L > 0 && OBJ > 0 && TOK > 0,
                  "%s: bs, heads in [1, 65535], npix, L, OBJ, TOK positive (got %d, %d, %d, %d, %d, %d)", who, bs, heads, npix,
                  L, OBJ, TOK);
    COMAT_REQUIRE((int64_t)bs * heads * npix * L < (1ll << 40) && (int64_t)bs * heads * TOK * npix < (1ll << 40) &&
                  (int64_t)bs * TOK < (1ll << 24), "%s: the batch is too large", who);
    return COMAT_OK;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int comat_mask_resize_any(const uint8_t* masks, const int32_t* ylo, const int32_t* yhi, const int32_t* xlo,
                                     const int32_t* xhi, float* out, int32_t n, int32_t H, int32_t W, int32_t res,
                                     void* stream) {
    COMAT_REQUIRE(n >= 0 && n <= 65535 && H > 0 && W > 0 && W <= 32768 && res > 0 && res <= 65535,
                  "comat_mask_resize_any: n in [0, 65535], H, W, res positive, W <= 32768 (got %d, %d, %d, %d)", n, H, W, res);
    if (n == 0) return COMAT_OK;  // no launch
    COMAT_REQUIRE(masks && ylo && yhi && xlo && xhi && out, "comat_mask_resize_any: null pointer");
    hipLaunchKernelGGL(mask_resize_any_kernel, dim3(res, n), dim3(NT), (size_t)((W + 15) / 16) * 16, ST, masks, ylo, yhi, xlo,
                       xhi, out, H, W, res);
    return comat_check_launch("comat_mask_resize_any");
}

extern "C" int64_t comat_attrcon_workspace_floats(int32_t M, int32_t bs, int32_t heads, int32_t npix, int32_t TOK) {
    if (M <= 0 || bs <= 0 || heads <= 0 || npix <= 0 || TOK <= 0) return 0;
    const int64_t nblk = (npix + RPB32 - 1) / RPB32;  // the finest chunking any variant uses
    const int64_t gather = (int64_t)bs * heads * TOK * (nblk * 2 + npix);
    const int64_t parts = (int64_t)bs * ((npix + NT - 1) / NT);
    return gather > parts ? gather : parts;
}

extern "C" int comat_attrcon_gather_fwd(const void* amap, const float* masks, const int32_t* n_obj, const int32_t* n_tok,
                                        const int32_t* tok_idx, const int32_t* tok_obj, float* num, float* den, float* avg,
                                        float* ws, int32_t bs, int32_t heads, int32_t npix, int32_t L, int32_t OBJ, int32_t TOK,
                                        int32_t dtype, void* stream) {
    COMAT_REQUIRE(amap && masks && n_obj && n_tok && tok_idx && tok_obj && num && den && avg && ws,
                  "comat_attrcon_gather_fwd: null pointer");
    COMAT_REQUIRE(dtype_ok(dtype), "comat_attrcon_gather_fwd: bad dtype %d", dtype);
    if (int rc = attrcon_shape_check("comat_attrcon_gather_fwd", bs, heads, npix, L, OBJ, TOK)) return rc;
    bool staged;
    const int nblk = gather_blocks(amap, npix, L, dtype, &staged);
    const dim3 grid(nblk, heads, bs);
    if (staged && dtype == COMAT_BF16)
        hipLaunchKernelGGL((attrcon_gather_lds_kernel<bf16_t, RPB16>), grid, dim3(NT), 16 + RPB16 * L * 2, ST,
                           (const bf16_t*)amap, masks, n_obj, n_tok, tok_idx, tok_obj, ws, bs, heads, npix, L, OBJ, TOK);
    else if (staged)
        hipLaunchKernelGGL((attrcon_gather_lds_kernel<float, RPB32>), grid, dim3(NT), 16 + RPB32 * L * 4, ST,
                           (const float*)amap, masks, n_obj, n_tok, tok_idx, tok_obj, ws, bs, heads, npix, L, OBJ, TOK);
    else
        hipLaunchKernelGGL(attrcon_gather_kernel, grid, dim3(NT), 0, ST, amap, masks, n_obj, n_tok, tok_idx, tok_obj, ws, bs,
                           heads, npix, L, OBJ, TOK, dtype);
    const int64_t work = (int64_t)TOK * (npix > heads ? npix : heads);
    hipLaunchKernelGGL(attrcon_gather_final_kernel, dim3((unsigned)cdiv64(work, NT), bs), dim3(NT), 0, ST, (const float*)ws,
                       n_obj, n_tok, nblk, bs, heads, npix, TOK, num, den, avg);
    return comat_check_launch("comat_attrcon_gather_fwd");
}

extern "C" int comat_attrcon_loss(const float* num, const float* den, const float* avg, const float* masks,
                                  const int32_t* n_obj, const int32_t* n_tok, const int32_t* tok_obj, const float* inv_len,
                                  float* g_num, float* g_den, float* g_avg, float* out, float* ws, int32_t M, int32_t bs,
                                  int32_t heads, int32_t npix, int32_t OBJ, int32_t TOK, void* stream) {
    COMAT_REQUIRE(num && den && avg && masks && n_obj && n_tok && tok_obj && inv_len && g_num && g_den && g_avg && out && ws,
                  "comat_attrcon_loss: null pointer");
    COMAT_REQUIRE(M > 0 && M <= 1024, "comat_attrcon_loss: M in [1, 1024] (got %d)", M);
    if (int rc = attrcon_shape_check("comat_attrcon_loss", bs, heads, npix, 1, OBJ, TOK)) return rc;
    const int nblk = (npix + NT - 1) / NT;
    hipLaunchKernelGGL(attrcon_pixel_kernel, dim3(nblk, bs), dim3(NT), 0, ST, avg, masks, n_obj, n_tok, tok_obj, g_avg, ws, M,
                       bs, npix, OBJ, TOK);
    hipLaunchKernelGGL(attrcon_token_kernel, dim3(1), dim3(NT), 0, ST, num, den, n_obj, n_tok, inv_len, (const float*)ws,
                       nblk * bs, g_num, g_den, out, M, bs, heads, TOK);
    return comat_check_launch("comat_attrcon_loss");
}

extern "C" int comat_attrcon_gather_bwd(const float* g_num, const float* g_den, const float* g_avg, const float* masks,
                                        const int32_t* n_obj, const int32_t* n_tok, const int32_t* tok_idx,
                                        const int32_t* tok_obj, const float* go, void* damap, int32_t bs, int32_t heads,
                                        int32_t npix, int32_t L, int32_t OBJ, int32_t TOK, int32_t dtype, void* stream) {
    COMAT_REQUIRE(g_num && g_den && g_avg && masks && n_obj && n_tok && tok_idx && tok_obj && go && damap,
                  "comat_attrcon_gather_bwd: null pointer");
    COMAT_REQUIRE(dtype_ok(dtype), "comat_attrcon_gather_bwd: bad dtype %d", dtype);
    if (int rc = attrcon_shape_check("comat_attrcon_gather_bwd", bs, heads, npix, L, OBJ, TOK)) return rc;
    const int es = dtype == COMAT_BF16 ? 2 : 4;
    const bool staged = chunks_vectorise(damap, npix, L, es, RPBB, (int64_t)RPBB * L * 4);
    if (staged && dtype == COMAT_BF16)
        hipLaunchKernelGGL((attrcon_bwd_lds_kernel<bf16_t, RPBB>), dim3((npix + RPBB - 1) / RPBB, heads, bs), dim3(NT),
                           RPBB * L * 4, ST, g_num, g_den, g_avg, masks, n_obj, n_tok, tok_idx, tok_obj, go, (bf16_t*)damap,
                           heads, npix, L, OBJ, TOK);
    else if (staged)
        hipLaunchKernelGGL((attrcon_bwd_lds_kernel<float, RPBB>), dim3((npix + RPBB - 1) / RPBB, heads, bs), dim3(NT),
                           RPBB * L * 4, ST, g_num, g_den, g_avg, masks, n_obj, n_tok, tok_idx, tok_obj, go, (float*)damap,
                           heads, npix, L, OBJ, TOK);
    else
        hipLaunchKernelGGL(attrcon_bwd_kernel, dim3((npix + NT - 1) / NT, heads, bs), dim3(NT), 0, ST, g_num, g_den, g_avg, masks,
                           n_obj, n_tok, tok_idx, tok_obj, go, damap, heads, npix, L, OBJ, TOK, dtype);
    return comat_check_launch("comat_attrcon_gather_bwd");
}
