// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) and the
// dropout keep rule built on it.  ONE text for the device kernels and the host entry points (norm_act.hip, norm_bwd.hip): the training
// backward regenerates the forward's mask from (seed, layer, element) instead of storing it.
#pragma once
#include <stdint.h>

#define CTSI_PHILOX_M0 0xD2511F53u
#define CTSI_PHILOX_M1 0xCD9E8D57u
#define CTSI_PHILOX_W0 0x9E3779B9u
#define CTSI_PHILOX_W1 0xBB67AE85u

__host__ __device__ inline void ctsi_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    uint32_t k0 = key[0], k1 = key[1];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)CTSI_PHILOX_M0 * c0;
        const uint64_t p1 = (uint64_t)CTSI_PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += CTSI_PHILOX_W0;
        k1 += CTSI_PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Keep bits of one 16-byte chunk (8 consecutive channels of one voxel): bit j set <=> channel j of the chunk is kept.
// chunk = ((sample * vox + voxel) * C + ch) / 8 on the logical NDHWC tensor; counter (lo32, hi32, layer, 0), key = seed halves;
// channel j takes the 16-bit lane (out[j >> 1] >> (16 * (j & 1))) & 0xffff and is kept iff lane >= thr.
__host__ __device__ inline uint32_t ctsi_dropout_keep8(unsigned long long chunk, uint32_t layer, unsigned long long seed,
                                                       uint32_t thr) {
    const uint32_t ctr[4] = {(uint32_t)chunk, (uint32_t)(chunk >> 32), layer, 0u};
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t o[4];
    ctsi_philox4x32_10(ctr, key, o);
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t lane = (o[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        bits |= (lane >= thr ? 1u : 0u) << j;
    }
    return bits;
}
