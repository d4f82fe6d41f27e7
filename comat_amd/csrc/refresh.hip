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
#include "gemm_shared.h"

namespace {

constexpr int WR_T = 64;          // tile edge
constexpr int WR_LDH = WR_T + 8;  // LDS row pitch in bf16: 16-byte aligned rows, no 2-way conflicts on the column gathers
constexpr int WR_LDF = WR_T + 1;  // LDS row pitch in fp32

struct WrProblem {  // mirrors the int64 [n, 8] table of comat_weights_refresh (offsets in elements)
    int64_t src, w, wt, R, C, lds, ldw, ldt;
};

// tile[r][c] = master value at (r0 + r, c0 + c), zero outside the matrix: 16 lanes x 16 bytes per row, 16 rows per pass
template <typename T, int LD>
__device__ __forceinline__ void wr_load_tile(T* tile, const float* __restrict__ src, int64_t lds, int R, int C, int r0, int c0) {
    const bool vec = ((uintptr_t)src % 16 == 0) && lds % 4 == 0;
    const int c4 = (threadIdx.x & 15) * 4;
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
            if constexpr (sizeof(T) == 2) tile[r * LD + c4 + e] = f32_to_bf16(v[e]);
            else tile[r * LD + c4 + e] = v[e];
        }
    }
}

__global__ __launch_bounds__(256) void weights_refresh_bf16_kernel(const float* __restrict__ master, bf16_t* __restrict__ wbase,
                                                                   bf16_t* __restrict__ wtbase, const WrProblem* __restrict__ problems,
                                                                   const int32_t* __restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) bf16_t tile[WR_T * WR_LDH];
    const int32_t* t = tiles + (int64_t)blockIdx.x * 3;
    const WrProblem p = problems[t[0]];
    const int r0 = t[1], c0 = t[2], R = (int)p.R, C = (int)p.C;
    wr_load_tile<bf16_t, WR_LDH>(tile, master + p.src, p.lds, R, C, r0, c0);
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
__global__ __launch_bounds__(256) void weights_refresh_f32_kernel(const float* __restrict__ master, float* __restrict__ wtbase,
                                                                  const WrProblem* __restrict__ problems,
                                                                  const int32_t* __restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) float tile[WR_T * WR_LDF];
    const int32_t* t = tiles + (int64_t)blockIdx.x * 3;
    const WrProblem p = problems[t[0]];
    const int r0 = t[1], c0 = t[2], R = (int)p.R, C = (int)p.C;
    wr_load_tile<float, WR_LDF>(tile, master + p.src, p.lds, R, C, r0, c0);
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
        hipLaunchKernelGGL(weights_refresh_f32_kernel, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, master, (float*)wt,
                           (const WrProblem*)problems, tiles);
    else
        hipLaunchKernelGGL(weights_refresh_bf16_kernel, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, master, (bf16_t*)w,
                           (bf16_t*)wt, (const WrProblem*)problems, tiles);
    return comat_check_launch("comat_weights_refresh");
}
