// What the GroupNorm passes share (norm_act.hip, f32_ops.hip, norm_bwd.hip): the bf16x8 unpack / pack pair, SiLU's derivative, the
// optionally non-temporal 16-byte access, the fp64 (sum, sumsq) -> (mean, rstd) step, and on the host the grid rules of the forward
// and of the backward's third pass, the statistics-tile rule and the backward's workspace layout.  ONE text each: a retuned
// range, threshold or tile size reaches the default passes and the scale-shift / dropout forms together.
#pragma once
#include "ctsi_internal.h"
#include <math.h>
#include <stdlib.h>

__device__ __forceinline__ void gn_unpack8(const uint4 v, float* f) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 gn_pack8(const float* f) {
    uint4 v;
    v.x = pack_bf16x2(f[0], f[1]); v.y = pack_bf16x2(f[2], f[3]);
    v.z = pack_bf16x2(f[4], f[5]); v.w = pack_bf16x2(f[6], f[7]);
    return v;
}
// d/dz [z * sigmoid(z)]
__device__ __forceinline__ float silu_grad_f(float z) {
    const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * z));
    return s * (1.0f + z * (1.0f - s));
}

// 16-byte accesses, optionally non-temporal (tensors far larger than the Infinity Cache: streamed once)
typedef unsigned int gn_u4_t __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ uint4 gn_ld(const bf16_t* p) {
    if (NT) {
        const gn_u4_t v = __builtin_nontemporal_load(reinterpret_cast<const gn_u4_t*>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    return *reinterpret_cast<const uint4*>(p);
}
template <bool NT>
__device__ __forceinline__ void gn_st(bf16_t* p, const uint4 v) {
    if (NT) {
        const gn_u4_t w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, reinterpret_cast<gn_u4_t*>(p));
    } else {
        *reinterpret_cast<uint4*>(p) = v;
    }
}

// (sum, sumsq) of one (sample, group) over cnt elements -> mean and 1 / sqrt(var + eps), in fp64.  The bf16 passes cast both to
// float at their own sites; the fp32 passes go on in double.
struct GnMeanRstd { double mean, rstd; };
__device__ __forceinline__ GnMeanRstd gn_mean_rstd(const double* __restrict__ pair, double cnt, float eps) {
    const double m = pair[0] / cnt;
    double var = pair[1] / cnt - m * m;
    if (var < 0.0) var = 0.0;
    return {m, 1.0 / sqrt(var + (double)eps)};
}

// eight floats of an LDS row of per-channel coefficients, as two 16-byte reads
__device__ __forceinline__ void gn_lds8(float* dst, const float* s_row, int q) {
    *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(s_row + q * 8);
    *reinterpret_cast<float4*>(dst + 4) = *reinterpret_cast<const float4*>(s_row + q * 8 + 4);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static inline int gn_gcd256(int cpr) {
    int gq = cpr, g256 = 256;
    while (g256) { const int t = gq % g256; gq = g256; g256 = t; }
    return gq;
}

// Grid of the bf16 forward (ctsi_gn_apply, ctsi_gn_apply_mod): (blocks, n) x 256 threads over vox * c / 8 16-byte chunks.
// A grid stride that is a multiple of the chunks per voxel row (c / 8) keeps every thread on one 8-channel chunk (constq).
// Contiguous ranges: every block takes ONE batch of 4 x 256 consecutive 16-byte chunks (16 KB) and the blocks are dispatched in
// address order, so the chip's working front moves linearly through the tensor.  Against 2048 grid-striding blocks (each
// thread's loads 8 MB apart) the decoder-size tensors go from 4.7-4.8 to 6.0-6.3 TB/s (3.2 GB at 128 channels x 48 x 512^2: 1345 ->
// 1069 us; with a residual 2044 -> 1554 us), the U-Net's 201 MB tensors from 6.5 to 6.7 TB/s.  Needs 256 % (c / 8) == 0 (a
// thread then stays on one 8-channel chunk); other channel counts keep the grid-stride form.  CTSI_GN_CONTIG=0 forces it.
// Tensors well beyond the 256 MB Infinity Cache (> 512 MB: measured threshold) are streamed with non-temporal accesses
// (CTSI_GN_NT=0 / 1 overrides).  Both switches are read once per process.
struct GnFwdGrid {
    long long blocks, per_block;   // per_block > 0: chunks of a block's contiguous range; 0: grid-stride
    bool constq, nt;
};
static inline GnFwdGrid gn_fwd_grid(int n, int c, long long vox) {
    GnFwdGrid g;
    const long long total = vox * (c / 8);
    g.blocks = (total + 256 * 8 - 1) / (256 * 8);
    if (g.blocks > 2048) g.blocks = 2048;
    if (g.blocks < 1) g.blocks = 1;
    const int cpr = c / 8;
    const int need = cpr / gn_gcd256(cpr);                             // blocks must be a multiple of this
    if (g.blocks >= need) g.blocks -= g.blocks % need;
    g.constq = (g.blocks * 256) % cpr == 0;
    g.per_block = 0;
    static const char* cg = getenv("CTSI_GN_CONTIG");
    if (!(cg && atoi(cg) == 0) && 256 % cpr == 0) {
        g.per_block = 1024;
        g.blocks = (total + g.per_block - 1) / g.per_block;
        g.constq = true;
    }
    static const char* nt_env = getenv("CTSI_GN_NT");
    g.nt = nt_env ? atoi(nt_env) != 0 : (long long)n * vox * c * 2 > (512ll << 20);
    return g;
}

// The options of the ResBlock's middle pass, as the forward and the backward launchers take them; the default
// entry points pass GnOptions{}.
struct GnOptions {
    bool mod = false;                         // the middle pass's own entry point (ctsi_gn_*_mod)
    int film = 0;                             // 1: scale-shift, the time row holds (s | b)
    uint32_t thr = 0;                         // dropout threshold in 1 / 65536 units, 0 = none
    float inv_keep = 0.0f;
    const unsigned long long* seed = nullptr;
    uint32_t layer_id = 0;
    int form() const { return film | (thr > 0 ? 2 : 0); }     // bit 0 FILM, bit 1 DROP
};

// Grid of the backward's third pass: contiguous batches of 512 chunks per block when 256 % (c / 8) == 0, else a grid stride
// that is a multiple of the chunks per voxel row (cpr <= 256: one block's 256 threads times need).
struct GnBwdGrid { long long blocks; int contig; };
static inline GnBwdGrid gn_bwd_apply_grid(int c, long long vox) {
    const int cpr = c >> 3;
    const long long total = vox * cpr;
    GnBwdGrid g;
    g.blocks = (total + 255) / 256;
    if (g.blocks > 2048) g.blocks = 2048;
    g.contig = 0;
    if (256 % cpr == 0) {
        g.contig = 1;
        g.blocks = (total + 511) / 512;
    } else {
        const int need = cpr / gn_gcd256(cpr);
        g.blocks = (g.blocks + need - 1) / need * need;
    }
    return g;
}

// Rows per statistics tile of the backward's first pass: 512 for large tensors; halved until the launch has ~2048 blocks, down to
// one batch of four rows per thread lane.  With fixed 512-row tiles the coarse levels of a 192^2 patch were 16-216 blocks whose
// threads walked 32-128 voxels one load batch after the other: 38-47 us per launch whatever the tensor size
// (profiles/r03_train_kernel_stats.csv).
#define GN_BWD_TILE_ROWS 512
static inline int gn_bwd_tile_rows(int n, int c, long long vox) {
    const int rows_par = 256 / (c >> 3);
    const int min_rows = rows_par * 4 > 16 ? rows_par * 4 : 16;
    int rows = GN_BWD_TILE_ROWS;
    while (rows > min_rows && (long long)n * ((vox + rows - 1) / rows) < 2048) rows >>= 1;
    return rows;
}

// The backward's workspace: colsum [n][tiles][4][c] | s12 [n][groups][2] | pgrad [n][4][c], in floats
struct GnBwdWorkspace {
    int tile_rows, tiles;
    long long s12_off, pgrad_off, floats;
    GnBwdWorkspace(int n, int c, long long vox, int groups) {
        tile_rows = gn_bwd_tile_rows(n, c, vox);
        const long long t = (vox + tile_rows - 1) / tile_rows;
        tiles = (int)t;
        s12_off = (long long)n * t * 4 * c;
        pgrad_off = s12_off + (long long)n * groups * 2;
        floats = pgrad_off + (long long)n * 4 * c;
    }
};
