// refresh.hip — the compute copies of every fully trained weight of a model in ONE launch (include/comat_hip.h:
// comat_weights_refresh), the UNet under `--full_finetuning`.
//
// The optimizer updates a flat fp32 master.  The products read a compute-dtype copy of each weight in two orientations: the
// forward one (a Linear's w [N, K], a conv's w [Cout, KH, KW, Cin]) and the data-gradient one (wt [K, N]; wd [Cin, KH, KW, Cout]
// with flipped taps).  Both are pitched transposes of row-major matrices: a Linear is one matrix, a conv one matrix per tap
// (rows = Cout at pitch KH KW Cin, columns = Cin; its transpose lands at tap KH KW - 1 - t of wd at pitch KH KW Cout).  So one
// problem is (source, R, C, pitches), one workgroup moves one 64 x 64 tile of it: read once from the master, rounded ONCE to
// bf16, staged in LDS, and both copies leave in 16-byte rows - the same bits in both.  HBM-bound by construction: 4 bytes read
// and 2 x 2 written per element.  In fp32 mode the master is the forward copy and only the transpose is written.
// Tile edges and rows that are not 16-byte aligned go element by element; nothing outside [R, C] is read or written.
//
// comat_weights_refresh_q8: the same launch also serves the fp8 forward of a fully trained model.  A third table gives every
// problem the SLOT of the quantised weight it belongs to (-1: not quantised).  The tile pass folds the abs-max of the rounded
// values it holds into the slot's word (agent-scope atomic max on the uint bits of a non-negative float: exact, order-independent);
// a second pass over the same tile table reads the forward copy, derives the slot's scale from that word and writes the e4m3 bytes
// at the forward copy's element offsets in 8-byte rows: 4 + 2 x 2 + 2 + 1 = 11 bytes per element of a quantised weight in bf16 mode.
#include "gemm_shared.h"

namespace {

constexpr int WR_T = 64;          // tile edge
constexpr int WR_LDH = WR_T + 8;  // LDS row pitch in bf16: 16-byte aligned rows, no 2-way conflicts on the column gathers
constexpr int WR_LDF = WR_T + 1;  // LDS row pitch in fp32

struct WrProblem {  // mirrors the int64 [n, 8] table of comat_weights_refresh (offsets in elements)
    int64_t src, w, wt, R, C, lds, ldw, ldt;
};

// tile[r][c] = master value at (r0 + r, c0 + c), zero outside the matrix: 16 lanes x 16 bytes per row, 16 rows per pass
// -> the largest magnitude among the (rounded) values this lane stored
template <typename T, int LD>
__device__ __forceinline__ float wr_load_tile(T* tile, const float* __restrict__ src, int64_t lds, int R, int C, int r0, int c0) {
    const bool vec = ((uintptr_t)src % 16 == 0) && lds % 4 == 0;
    const int c4 = (threadIdx.x & 15) * 4;
    float m = 0.0f;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int r = pass * 16 + (threadIdx.x >> 4);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < R) {
            const float* p = src + (int64_t)(r0 + r) * lds + c0 + c4;
            if (vec && c0 + c4 + 3 < C) {
                const float4 q = *(const float4*)p;
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c0 + c4 + e < C) v[e] = p[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (sizeof(T) == 2) {
                const bf16_t h = f32_to_bf16(v[e]);
                tile[r * LD + c4 + e] = h;
                m = amax_fold(m, bf16_to_f32(h));
            } else {
                tile[r * LD + c4 + e] = v[e];
                m = amax_fold(m, v[e]);
            }
        }
    }
    return m;
}

// Q8: the tile's abs-max joins the running maximum of the problem's slot (slots[problem] >= 0)
template <bool Q8>
__device__ __forceinline__ void wr_fold_amax(float m, const int32_t* __restrict__ slots, int problem, unsigned* __restrict__ amax_bits,
                                             float* sbuf) {
    if constexpr (Q8) {
        const int s = slots[problem];  // block-uniform
        if (s < 0) return;
        m = block_amax_256(m, sbuf);
        if (threadIdx.x == 0) fp8_amax_track(amax_bits + s, m);
    }
}

template <bool Q8>
__global__ __launch_bounds__(256) void weights_refresh_bf16_kernel(const float* __restrict__ master, bf16_t* __restrict__ wbase,
                                                                   bf16_t* __restrict__ wtbase, const WrProblem* __restrict__ problems,
                                                                   const int32_t* __restrict__ tiles, const int32_t* __restrict__ slots,
                                                                   unsigned* __restrict__ amax_bits) {
    __shared__ __attribute__((aligned(16))) bf16_t tile[WR_T * WR_LDH];
    __shared__ float sbuf[4];
    const int32_t* t = tiles + (int64_t)blockIdx.x * 3;
    const WrProblem p = problems[t[0]];
    const int r0 = t[1], c0 = t[2], R = (int)p.R, C = (int)p.C;
    const float m = wr_load_tile<bf16_t, WR_LDH>(tile, master + p.src, p.lds, R, C, r0, c0);
    wr_fold_amax<Q8>(m, slots, t[0], amax_bits, sbuf);
    __syncthreads();
    const int c8 = (threadIdx.x & 7) * 8;
    {  // w rows: 8 lanes x 16 bytes per row, 32 rows per pass
        bf16_t* w = wbase + p.w;
        const bool vec = ((uintptr_t)w % 16 == 0) && p.ldw % 8 == 0;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int r = pass * 32 + (threadIdx.x >> 3);
            if (r0 + r >= R || c0 + c8 >= C) continue;
            bf16_t* d = w + (int64_t)(r0 + r) * p.ldw + c0 + c8;
            if (vec && c0 + c8 + 7 < C) {
                *(uint4*)d = *(const uint4*)(tile + r * WR_LDH + c8);
            } else {
                for (int e = 0; e < 8 && c0 + c8 + e < C; ++e) d[e] = tile[r * WR_LDH + c8 + e];
            }
        }
    }
    {  // wt rows (= columns of the tile): 8 consecutive source rows per lane, gathered down a tile column
        bf16_t* wt = wtbase + p.wt;
        const bool vec = ((uintptr_t)wt % 16 == 0) && p.ldt % 8 == 0;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int c = pass * 32 + (threadIdx.x >> 3);
            if (c0 + c >= C || r0 + c8 >= R) continue;
            Pack16 pk;
#pragma unroll
            for (int e = 0; e < 8; ++e) pk.h[e] = tile[(c8 + e) * WR_LDH + c];
            bf16_t* d = wt + (int64_t)(c0 + c) * p.ldt + r0 + c8;
            if (vec && r0 + c8 + 7 < R) {
                *(uint4*)d = pk.u;
            } else {
                for (int e = 0; e < 8 && r0 + c8 + e < R; ++e) d[e] = pk.h[e];
            }
        }
    }
}

// fp32 parity mode: the master is the forward copy; only the transpose is written
template <bool Q8>
__global__ __launch_bounds__(256) void weights_refresh_f32_kernel(const float* __restrict__ master, float* __restrict__ wtbase,
                                                                  const WrProblem* __restrict__ problems,
                                                                  const int32_t* __restrict__ tiles, const int32_t* __restrict__ slots,
                                                                  unsigned* __restrict__ amax_bits) {
    __shared__ __attribute__((aligned(16))) float tile[WR_T * WR_LDF];
    __shared__ float sbuf[4];
    const int32_t* t = tiles + (int64_t)blockIdx.x * 3;
    const WrProblem p = problems[t[0]];
    const int r0 = t[1], c0 = t[2], R = (int)p.R, C = (int)p.C;
    const float m = wr_load_tile<float, WR_LDF>(tile, master + p.src, p.lds, R, C, r0, c0);
    wr_fold_amax<Q8>(m, slots, t[0], amax_bits, sbuf);
    __syncthreads();
    float* wt = wtbase + p.wt;
    const bool vec = ((uintptr_t)wt % 16 == 0) && p.ldt % 4 == 0;
    const int r4 = (threadIdx.x & 15) * 4;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int c = pass * 16 + (threadIdx.x >> 4);
        if (c0 + c >= C || r0 + r4 >= R) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tile[(r4 + e) * WR_LDF + c];
        float* d = wt + (int64_t)(c0 + c) * p.ldt + r0 + r4;
        if (vec && r0 + r4 + 3 < R) {
            *(float4*)d = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int e = 0; e < 4 && r0 + r4 + e < R; ++e) d[e] = v[e];
        }
    }
}

// comat_weights_refresh_q8 starts every slot's running maximum from zero
__global__ __launch_bounds__(256) void weights_amax_zero_kernel(unsigned* __restrict__ amax_bits, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) __hip_atomic_store(amax_bits + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the second pass of comat_weights_refresh_q8, over the same tile table: T = bf16_t reads the forward copy the first pass wrote
// (`fwd` = w, offsets p.w, pitch p.ldw), T = float the master itself (offsets p.src, pitch p.lds).  Every slot's maximum is complete
// (the first pass has ended), so each block derives the scale on its own; the first tile of a problem also stores it.  Bytes go to
// q8 + p.w at pitch p.ldw: 8 lanes x 8 columns per row, 32 rows per pass; one 8-byte store where the row allows, else byte by byte.
template <typename T>
__global__ __launch_bounds__(256) void weights_quantize_kernel(const T* __restrict__ fwd, unsigned char* __restrict__ q8base,
                                                               float* __restrict__ scales, const unsigned* __restrict__ amax_bits,
                                                               const WrProblem* __restrict__ problems, const int32_t* __restrict__ slots,
                                                               const int32_t* __restrict__ tiles) {
    const int32_t* t = tiles + (int64_t)blockIdx.x * 3;
    const int s = slots[t[0]];
    if (s < 0) return;
    const WrProblem p = problems[t[0]];
    const int r0 = t[1], c0 = t[2], R = (int)p.R, C = (int)p.C;
    const float scale = fp8_scale_of(__uint_as_float(__hip_atomic_load(amax_bits + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
    if (threadIdx.x == 0 && r0 == 0 && c0 == 0) scales[s] = scale;  // (every problem of the slot stores the same bits)
    const float inv = 1.0f / scale;
    constexpr bool H = sizeof(T) == 2;
    const T* src = fwd + (H ? p.w : p.src);
    const int64_t ld = H ? p.ldw : p.lds;
    const bool vin = ((uintptr_t)src % 16 == 0) && ld % (H ? 8 : 4) == 0;
    unsigned char* q = q8base + p.w;
    const bool vout = ((uintptr_t)q % 8 == 0) && p.ldw % 8 == 0;
    const int c8 = (threadIdx.x & 7) * 8;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int r = pass * 32 + (threadIdx.x >> 3);
        if (r0 + r >= R || c0 + c8 >= C) continue;
        const bool full = c0 + c8 + 7 < C;
        const T* sp = src + (int64_t)(r0 + r) * ld + c0 + c8;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (vin && full) {
            if constexpr (H) {
                Pack16 pk;
                pk.u = *(const uint4*)sp;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = bf16_to_f32(pk.h[e]);
            } else {
                const float4 a = *(const float4*)sp, b = *(const float4*)(sp + 4);
                v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + c8 + e < C) v[e] = ldf<T>(sp + e);
        }
        const uint2 b8 = fp8_pack8(v, inv);  // the clamp on every element, the tail included
        unsigned char* d = q + (int64_t)(r0 + r) * p.ldw + c0 + c8;
        if (vout && full) {
            *(uint2*)d = b8;
        } else {
            for (int e = 0; e < 8 && c0 + c8 + e < C; ++e) d[e] = (unsigned char)(((e < 4 ? b8.x : b8.y) >> (8 * (e & 3))) & 0xffu);
        }
    }
}

}  // namespace

extern "C" int comat_weights_refresh(const float* master, void* w, void* wt, const int64_t* problems, const int32_t* tiles,
                                     int64_t n_tiles, int32_t dtype, void* stream) {
    COMAT_REQUIRE(master && wt && problems && tiles, "comat_weights_refresh: null operand");
    COMAT_REQUIRE(dtype_ok(dtype), "comat_weights_refresh: the compute dtype must be bf16 or fp32");
    COMAT_REQUIRE(dtype == COMAT_F32 || w, "comat_weights_refresh: bf16 mode needs the forward copy w");
    COMAT_REQUIRE(n_tiles > 0 && n_tiles < (1ll << 31), "comat_weights_refresh: n_tiles must be in [1, 2^31) (got %lld)",
                  (long long)n_tiles);
    static_assert(sizeof(WrProblem) == 8 * sizeof(int64_t), "problem table layout");
    if (dtype == COMAT_F32)
        hipLaunchKernelGGL(weights_refresh_f32_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, master,
                           (float*)wt, (const WrProblem*)problems, tiles, (const int32_t*)nullptr, (unsigned*)nullptr);
    else
        hipLaunchKernelGGL(weights_refresh_bf16_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, master,
                           (bf16_t*)w, (bf16_t*)wt, (const WrProblem*)problems, tiles, (const int32_t*)nullptr, (unsigned*)nullptr);
    return comat_check_launch("comat_weights_refresh");
}

extern "C" int comat_weights_refresh_q8(const float* master, void* w, void* wt, uint8_t* q8, float* scales, uint32_t* amax_bits,
                                        const int64_t* problems, const int32_t* slots, const int32_t* tiles, int64_t n_tiles,
                                        int32_t n_slots, int32_t dtype, void* stream) {
    COMAT_REQUIRE(master && wt && q8 && scales && amax_bits && problems && slots && tiles, "comat_weights_refresh_q8: null operand");
    COMAT_REQUIRE(dtype_ok(dtype), "comat_weights_refresh_q8: the compute dtype must be bf16 or fp32");
    COMAT_REQUIRE(dtype == COMAT_F32 || w, "comat_weights_refresh_q8: bf16 mode needs the forward copy w");
    COMAT_REQUIRE(n_tiles > 0 && n_tiles < (1ll << 31), "comat_weights_refresh_q8: n_tiles must be in [1, 2^31) (got %lld)",
                  (long long)n_tiles);
    COMAT_REQUIRE(n_slots >= 1, "comat_weights_refresh_q8: n_slots must be >= 1 (got %d)", (int)n_slots);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_tiles), block(256);
    // three launches whatever the number of weights: the maxima start from zero IN this call (nothing an earlier call or an aborted
    // one left behind can reach a scale), the tile pass, the byte pass.  The zeroing is a kernel like the other two, so that a
    // captured call consists of kernel nodes only, as every other entry point's does (no memset node in a step's graphs).
    hipLaunchKernelGGL(weights_amax_zero_kernel, dim3((unsigned)cdiv64(n_slots, 256)), dim3(256), 0, st, (unsigned*)amax_bits, (int)n_slots);
    if (dtype == COMAT_F32) {
        hipLaunchKernelGGL(weights_refresh_f32_kernel<true>, grid, block, 0, st, master, (float*)wt, (const WrProblem*)problems, tiles, slots,
                           (unsigned*)amax_bits);
        hipLaunchKernelGGL(weights_quantize_kernel<float>, grid, block, 0, st, master, q8, scales, (const unsigned*)amax_bits,
                           (const WrProblem*)problems, slots, tiles);
    } else {
        hipLaunchKernelGGL(weights_refresh_bf16_kernel<true>, grid, block, 0, st, master, (bf16_t*)w, (bf16_t*)wt,
                           (const WrProblem*)problems, tiles, slots, (unsigned*)amax_bits);
        hipLaunchKernelGGL(weights_quantize_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)w, q8, scales, (const unsigned*)amax_bits,
                           (const WrProblem*)problems, slots, tiles);
    }
    return comat_check_launch("comat_weights_refresh_q8");
}
