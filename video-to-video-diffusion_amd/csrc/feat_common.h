// Helpers shared by the feature-loss passes (vgg_loss.hip, lpips.hip): bf16 pair access, the capped streaming grid and the
// fixed-order block sum of their two-stage reductions.
#pragma once
#include "ctsi_internal.h"

// the two bf16 halves of a dword as fp32
__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

static unsigned grid_for(long long items, int cap = 8192) {
    long long blocks = (items + 255) / 256;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

// fixed-order sum of one value per thread of a 256-thread block; the result is valid in thread 0
__device__ __forceinline__ double block_sum_256(double v, double* s_part) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}
