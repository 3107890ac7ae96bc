// The fixed-order reduction of the statistics kernels (depth_consistency.hip, measure_guide.hip, ensemble.hip): blocks of 256
// threads write one slot of fp64 partials each, a second launch folds the slots.  No atomics, one association order: the same
// bits on every run.  The reductions of guidance.hip, optim.hip, feat_common.h and the loss kernels add their wave sums pairwise
// or in contiguous runs -- another order, other bits -- and stay where they are.
#pragma once
#include "ctsi_internal.h"

constexpr int FR_THREADS = 256;
constexpr int FR_WAVES = FR_THREADS / 64;

// Q values per thread reduced over the block in a fixed order, bit q of MAXMASK set: a maximum, else a sum (thread 0 holds
// the result): 64 lanes by shuffles, then the four wave values in wave order
template <int Q, unsigned MAXMASK>
__device__ __forceinline__ void block_reduce(double* v, double* red /* [Q][FR_WAVES] */) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        double s = v[q];
        for (int o = 32; o > 0; o >>= 1) {
            const double t = __shfl_down(s, o, 64);
            s = ((MAXMASK >> q) & 1u) ? (t > s ? t : s) : s + t;
        }
        if ((threadIdx.x & 63) == 0) red[q * FR_WAVES + (threadIdx.x >> 6)] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            double s = red[q * FR_WAVES];
            for (int w = 1; w < FR_WAVES; ++w) {
                const double t = red[q * FR_WAVES + w];
                s = ((MAXMASK >> q) & 1u) ? (t > s ? t : s) : s + t;
            }
            v[q] = s;
        }
    }
}

// The second launch, one block per plane or sample: block b folds the `slots` slots from b * slots on, each slot_stride
// doubles apart with its Q values first, into out[b][Q].  Thread t takes slots t, t + 256, ... ascending (neighbouring lanes
// read neighbouring slots), then the 256 values go through the tree of block_reduce.  Four slots' loads are issued before the
// first use: one block walks a whole plane's slots (8192 at 512 x 512), and a trip per slot would pay the memory latency 32
// times over
template <int Q, unsigned MAXMASK>
__global__ void __launch_bounds__(FR_THREADS)
fold_slots_kernel(const double* __restrict__ partials, double* __restrict__ out, long long slots, int slot_stride) {
    __shared__ double red[Q * FR_WAVES];
    const double* p = partials + (long long)blockIdx.x * slots * slot_stride;
    double v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = 0.0;           // 0: the identity of both folds (every maximum folded here is >= 0)
    for (long long base = threadIdx.x; base < slots; base += 4 * FR_THREADS) {
        double t[4][Q];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = base + u * FR_THREADS;
#pragma unroll
            for (int q = 0; q < Q; ++q) t[u][q] = i < slots ? p[i * slot_stride + q] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < Q; ++q) v[q] = ((MAXMASK >> q) & 1u) ? (t[u][q] > v[q] ? t[u][q] : v[q]) : v[q] + t[u][q];
    }
    block_reduce<Q, MAXMASK>(v, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int q = 0; q < Q; ++q) out[(long long)blockIdx.x * Q + q] = v[q];
}
