// The column-tile frame of the kernels that work along depth: ctsi_depth_project (depth_consistency.hip)
// and ctsi_depth_residual_adj (measure_guide.hip).  Tensors are fp32 NCDHW contiguous; a "column" is the depth vector at one
// (plane = n c, position = h w).  One block of four waves owns TILE consecutive positions of one plane and stages whole columns
// in LDS, rows of TILE floats: x is read from HBM once and written once.  A lane is a position (unit-stride LDS rows: no bank
// conflicts); the waves split the rows of a phase, so at TILE = 64 a row is wave-uniform and its W / P / band operands are
// scalar loads; TILE = 32 (deep volumes) puts two rows in a wave.  Statistics leave a block through fixed_reduce.h into one
// slot per DT_SLOT positions, so the slot layout (ctsi_depth_project_blocks) is the same whichever tile a kernel picks.
// The frame holds no arithmetic: each kernel keeps its own body between stage_rows and store_rows.
#pragma once
#include "fixed_reduce.h"

constexpr int DT_MAX_D_IN = 64;
constexpr int DT_MAX_D_OUT = 512;
constexpr int DT_THREADS = FR_THREADS;
constexpr int DT_WAVES = FR_WAVES;
constexpr int DT_SLOT = 32;                  // positions per partial slot: the narrow tile, so the layout fits both tiles
constexpr int DT_LDS_TWO_BLOCKS = 80 * 1024; // half of the CU's 160 KiB

#define DT_CHECK_DEPTHS(fn, d_in, d_out)                                                                         \
    CTSI_CHECK_ARG((d_in) <= DT_MAX_D_IN && (d_out) <= DT_MAX_D_OUT,                                            \
                   fn ": depths d_in=%d d_out=%d exceed the limits d_in <= %d, d_out <= %d", (d_in), (d_out),  \
                   DT_MAX_D_IN, DT_MAX_D_OUT)

static inline int slots_per_plane(int hw) { return (hw + DT_SLOT - 1) / DT_SLOT; }

// two blocks per CU at the 64-wide tile (256 B: the reduction scratch beside the tile), else the 32-wide one; a kernel passes
// the dynamic LDS it would take at 64 positions
static inline int tile_for(size_t lds_bytes_at_64) { return lds_bytes_at_64 + 256 <= (size_t)DT_LDS_TWO_BLOCKS ? 64 : 32; }

__device__ __forceinline__ void band_of(const int* __restrict__ band, int row, int limit, int& lo, int& hi) {
    lo = band[2 * row], hi = band[2 * row + 1];
    lo = lo < 0 ? 0 : lo;                    // a bad table must not index outside the tile
    hi = hi >= limit ? limit - 1 : hi;
}

// the block's place in the grid of planes x tiles_pp tiles, and this thread's in the tile
template <int TILE, bool VEC>
struct DepthTile {
    static constexpr int RPW = 64 / TILE;               // rows per wave
    static constexpr int STRIDE = DT_WAVES * RPW;       // a thread takes the rows row0, row0 + STRIDE, ...
    int tile, p0, valid;                                 // valid: positions before the plane's end
    long long plane;

    __device__ __forceinline__ DepthTile(int tiles_pp, int hw) {
        tile = blockIdx.x % tiles_pp;
        plane = blockIdx.x / tiles_pp;
        p0 = tile * TILE;
        valid = hw - p0 < TILE ? hw - p0 : TILE;
    }
    // this thread's position in the tile and its first row (RPW == 1: wave-uniform, so W / P / band loads are scalar)
    __device__ __forceinline__ static int pos() { return (threadIdx.x & 63) % TILE; }
    __device__ __forceinline__ static int row0() {
        return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * RPW + (threadIdx.x & 63) / TILE;
    }

    // stage the column tile: d_out rows of x, then d_in rows of y behind them (one row index); positions past the plane's end
    // read as 0.  xg, yg: position p0 of the plane's first row.  Four independent loads per thread are issued before the first
    // LDS store: a block then has its whole tile in flight at the production depth ((48 + 8) rows x 64 positions = 3.5 16-byte
    // loads per thread), not one load per thread and trip
    __device__ __forceinline__ void stage_rows(float* xs, const float* xg, const float* yg, int d_out, int d_in, int hw) const {
        if (VEC) {
            constexpr int Q = TILE / 4;
            const int total = (d_out + d_in) * Q;
            for (int base = threadIdx.x; base < total; base += 4 * DT_THREADS) {
                float4 t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = base + u * DT_THREADS;
                    const int row = i / Q, p = (i - row * Q) * 4;
                    t[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (i < total && p < valid)
                        t[u] = row < d_out ? *reinterpret_cast<const float4*>(xg + (long long)row * hw + p)
                                           : *reinterpret_cast<const float4*>(yg + (long long)(row - d_out) * hw + p);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = base + u * DT_THREADS;
                    const int row = i / Q, p = (i - row * Q) * 4;
                    if (i < total) *reinterpret_cast<float4*>(xs + row * TILE + p) = t[u];
                }
            }
        } else {
            const int total = (d_out + d_in) * TILE;
            for (int base = threadIdx.x; base < total; base += 4 * DT_THREADS) {
                float t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = base + u * DT_THREADS;
                    const int row = i / TILE, p = i - row * TILE;
                    t[u] = 0.0f;
                    if (i < total && p < valid)
                        t[u] = row < d_out ? xg[(long long)row * hw + p] : yg[(long long)(row - d_out) * hw + p];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = base + u * DT_THREADS;
                    if (i < total) xs[i] = t[u];          // row * TILE + p == i
                }
            }
        }
    }

    // the first d_out rows of the tile back to HBM; the padded positions are never stored
    __device__ __forceinline__ void store_rows(float* dst, const float* xs, int d_out, int hw) const {
        if (VEC) {
            constexpr int Q = TILE / 4;
            for (int i = threadIdx.x; i < d_out * Q; i += DT_THREADS) {
                const int row = i / Q, p = (i - row * Q) * 4;
                if (p < valid)
                    *reinterpret_cast<float4*>(dst + (long long)row * hw + p) = *reinterpret_cast<const float4*>(xs + row * TILE + p);
            }
        } else {
            for (int i = threadIdx.x; i < d_out * TILE; i += DT_THREADS) {
                const int row = i / TILE, p = i - row * TILE;
                if (p < valid) dst[(long long)row * hw + p] = xs[row * TILE + p];
            }
        }
    }

    // thread 0, after block_reduce: the block's Q values into its slot.  One slot per DT_SLOT positions: a 64-wide tile owns
    // two, the second one (when the plane has it) holds zeros
    template <int Q>
    __device__ __forceinline__ void write_slot(double* partials, int slots_pp, const double* v) const {
        const int slot = tile * (TILE / DT_SLOT);
        double* out = partials + (plane * slots_pp + slot) * Q;
        for (int q = 0; q < Q; ++q) out[q] = v[q];
        if (TILE / DT_SLOT == 2 && slot + 1 < slots_pp)
            for (int q = 0; q < Q; ++q) out[Q + q] = 0.0;
    }
};

// Kernel::get<TILE, VEC>() names the four instantiations of a kernel written against DepthTile; its more than 64 KiB of
// dynamic LDS are a function attribute, set once per device and instantiation
template <class Kernel, int TILE, bool VEC, class Args>
void launch_tile(const Args& a, long long blocks, size_t lds, void* stream) {
    auto k = Kernel::template get<TILE, VEC>();
    static CtsiPerDeviceOnce attr_once;
    if (attr_once.first()) hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, DT_LDS_TWO_BLOCKS);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(DT_THREADS), lds, (hipStream_t)stream, a);
}

template <class Kernel, class Args>
void launch_tiled(const Args& a, int tile, bool vec, long long blocks, size_t lds, void* stream) {
    if (tile == 64) {
        if (vec) launch_tile<Kernel, 64, true>(a, blocks, lds, stream);
        else launch_tile<Kernel, 64, false>(a, blocks, lds, stream);
    } else {
        if (vec) launch_tile<Kernel, 32, true>(a, blocks, lds, stream);
        else launch_tile<Kernel, 32, false>(a, blocks, lds, stream);
    }
}
