// GroupNorm statistics + fused normalise / SiLU / time-bias / residual kernels (HBM-bound).
// Replaces nn.GroupNorm + nn.SiLU + the ResBlock tails of the reference:
//   models/unet3d.py:59-60,70-74,95-98,116-133,151,167,328-330 and models/vae.py:28-35,44-56,69-76,90-97.
// All tensors are bf16 NDHWC; every global access is a 16-byte (8-channel) vector per lane.
// Statistics path: per-tile column sums (conv epilogue or gn_colsum_kernel) -> gn_finalize_kernel
// (fp64 (sum, sumsq) per (sample, group)) -> gn_apply_kernel.
// gn_apply_kernel also serves the ResBlock's middle pass with the ADM-style options (ctsi_gn_apply_mod); the
// dropout-mask and Philox windows the tests read are at the end.  What the passes share with the fp32 forward (f32_ops.hip) and
// the backward (norm_bwd.hip) is gn_frame.h.
#include "ctsi_internal.h"
#include "ctsi_philox.h"
#include "gn_frame.h"

#define GN_TILE_ROWS 512

// ---- column sums of a tensor no conv produced ------------------------------------------------
// grid: (tiles_per_sample, n); block 256.  cpr = c/8 16-byte chunks per voxel.
__global__ void __launch_bounds__(256)
gn_colsum_kernel(const bf16_t* __restrict__ x, float* __restrict__ colsum, int n_total, int c,
                 long long vox_per_sample, int tps) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_red = reinterpret_cast<float*>(smem_raw);  // [rows_par][c][2]
    const int cpr = c >> 3;
    const int rows_par = 256 / cpr;
    const int tid = threadIdx.x;
    const int q = tid % cpr, rl = tid / cpr;
    const int tile = blockIdx.x, nb = blockIdx.y;
    const long long v0 = (long long)tile * GN_TILE_ROWS;
    long long v1 = v0 + GN_TILE_ROWS;
    if (v1 > vox_per_sample) v1 = vox_per_sample;
    float s1[8], s2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s1[k] = s2[k] = 0.0f;
    if (rl < rows_par) {
        const bf16_t* base = x + ((long long)nb * vox_per_sample) * c + q * 8;
        for (long long v = v0 + rl; v < v1; v += rows_par) {
            const uint4 raw = *reinterpret_cast<const uint4*>(base + v * c);
            float f[8];
            gn_unpack8(raw, f);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                s1[k] += f[k];
                s2[k] += f[k] * f[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            s_red[((rl * c) + q * 8 + k) * 2 + 0] = s1[k];
            s_red[((rl * c) + q * 8 + k) * 2 + 1] = s2[k];
        }
    }
    __syncthreads();
    for (int col = tid; col < c; col += 256) {
        float t1 = 0.0f, t2 = 0.0f;
        for (int r = 0; r < rows_par; ++r) {
            t1 += s_red[(r * c + col) * 2 + 0];
            t2 += s_red[(r * c + col) * 2 + 1];
        }
        const long long tg = (long long)nb * tps + tile;
        const long long slab = (long long)n_total * tps * c;
        colsum[tg * c + col] = t1;
        colsum[slab + tg * c + col] = t2;
    }
}

extern "C" int ctsi_gn_colsum_tiles(int d, int h, int w) {
    const long long vox = (long long)d * h * w;
    return (int)((vox + GN_TILE_ROWS - 1) / GN_TILE_ROWS);
}

extern "C" int ctsi_gn_colsum(const void* x, float* colsum, int n, int c, int d, int h, int w,
                              int* tiles_per_sample, void* stream) {
    CTSI_CHECK_ARG(x && colsum, "ctsi_gn_colsum: null argument");
    CTSI_CHECK_ARG(c % 8 == 0 && c >= 8 && c <= 2048, "ctsi_gn_colsum: c=%d must be a multiple of 8 in [8,2048]", c);
    const int tps = ctsi_gn_colsum_tiles(d, h, w);
    if (tiles_per_sample) *tiles_per_sample = tps;
    const int cpr = c / 8, rows_par = 256 / cpr;
    const size_t lds = (size_t)rows_par * c * 2 * sizeof(float);
    hipLaunchKernelGGL(gn_colsum_kernel, dim3(tps, n), dim3(256), lds, (hipStream_t)stream,
                       (const bf16_t*)x, colsum, n, c, (long long)d * h * w, tps);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- finalize: column-sum slab -> (sum, sumsq) per (sample, group), fp64 -----------------------
// grid: (groups, n); block 1024.  ONE block owns one (sample, group): every thread sums a fixed, strided subset of the
// tile partials in a fixed order, the block combines them with a fixed-shape tree, and the result is WRITTEN (not
// accumulated) -- the statistics are bit-identical from run to run by construction (no atomics, no dependence on block
// scheduling), and the sums buffer needs no zeroing.
// Split form (gridDim.z = S > 1: tensors with tens of thousands of tiles -- the VAE at full resolution: 24576 tiles, 3 MB of
// partials per group, 71 us per launch when ONE block read them): slice s of a (sample, group) sums items
// [s * per, (s + 1) * per) the same way, parks its pair in a scratch row (agent-scope stores) and takes a ticket; the block that
// draws the last ticket adds the S pairs IN SLICE ORDER and writes the result: still no dependence on block scheduling.
// The scratch rows and tickets are process-global and the slot rotates per call: launches that could run CONCURRENTLY on one
// device (two streams, two host threads, two graphs replayed side by side) must not both take the split form -- the engine
// issues everything of a device on ONE stream (Ctx), which is what makes this safe; a caller that cannot promise that sets
// CTSI_GN_FIN_SPLIT=0.
#define GN_FIN_ROWS 2048
#define GN_FIN_SMAX 64
#define GN_FIN_SLOTS 4
__device__ double g_fin_part[GN_FIN_SLOTS][GN_FIN_ROWS][GN_FIN_SMAX][2];
__device__ unsigned int g_fin_ticket[GN_FIN_SLOTS][GN_FIN_ROWS];

__global__ void __launch_bounds__(1024)
gn_finalize_kernel(const float* __restrict__ colsum, double* __restrict__ sums, int n_total, int c_pad,
                   int groups, int cpg, int tps, int nclass, int accumulate, int slot) {
    const int g = blockIdx.x, nb = blockIdx.y;
    const int tid = threadIdx.x;
    const int S = gridDim.z, sl = blockIdx.z;
    const long long slab = (long long)nclass * n_total * tps * c_pad;
    const int items = tps * cpg;
    double a1[4] = {0.0, 0.0, 0.0, 0.0}, a2[4] = {0.0, 0.0, 0.0, 0.0};
    if ((cpg & 3) == 0 && (c_pad & 3) == 0) {
        // 16-byte loads, 8 of them in flight per thread and statistic: a group's cpg channels of one tile row are contiguous.
        // Large tensors (the VAE decoder at full resolution: 24576 tiles per sample) are latency-, not bandwidth-bound here:
        // the scalar form below took 30-140 us per launch on them (15 launches per decode), this one a few us.
        const int q4 = cpg >> 2, items4_all = tps * q4;
        const int per = S > 1 ? ((items4_all + S - 1) / S + 1023) / 1024 * 1024 : items4_all;   // (whole thread rounds per slice)
        const int it0 = sl * per;
        const int items4 = it0 + per < items4_all ? it0 + per : items4_all;
        const float4* cs1 = reinterpret_cast<const float4*>(colsum);
        const float4* cs2 = reinterpret_cast<const float4*>(colsum + slab);
        for (int cls = 0; cls < nclass; ++cls) {
            const long long tbase = ((long long)cls * n_total + nb) * tps;
            int it = it0 + tid;
            for (; it + 7 * 1024 < items4; it += 8 * 1024) {
                float4 v1[8], v2[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i2 = it + u * 1024;
                    const long long idx = (((tbase + i2 / q4) * c_pad + g * cpg) >> 2) + i2 % q4;
                    v1[u] = cs1[idx];
                    v2[u] = cs2[idx];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    a1[u & 3] += ((double)v1[u].x + (double)v1[u].y) + ((double)v1[u].z + (double)v1[u].w);
                    a2[u & 3] += ((double)v2[u].x + (double)v2[u].y) + ((double)v2[u].z + (double)v2[u].w);
                }
            }
            for (int u = 0; it < items4; it += 1024, ++u) {
                const long long idx = (((tbase + it / q4) * c_pad + g * cpg) >> 2) + it % q4;
                const float4 w1 = cs1[idx], w2 = cs2[idx];
                a1[u & 3] += ((double)w1.x + (double)w1.y) + ((double)w1.z + (double)w1.w);
                a2[u & 3] += ((double)w2.x + (double)w2.y) + ((double)w2.z + (double)w2.w);
            }
        }
    } else
    for (int cls = 0; cls < nclass; ++cls) {
        const long long tbase = ((long long)cls * n_total + nb) * tps;
        int it = tid;
        for (; it + 3 * 1024 < items; it += 4 * 1024) {   // four independent loads in flight per statistic
            float v1[4], v2[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i2 = it + u * 1024;
                const long long idx = (tbase + i2 / cpg) * c_pad + g * cpg + i2 % cpg;
                v1[u] = colsum[idx];
                v2[u] = colsum[slab + idx];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a1[u] += (double)v1[u];
                a2[u] += (double)v2[u];
            }
        }
        for (int u = 0; it < items; it += 1024, ++u) {
            const long long idx = (tbase + it / cpg) * c_pad + g * cpg + it % cpg;
            a1[u] += (double)colsum[idx];
            a2[u] += (double)colsum[slab + idx];
        }
    }
    // fixed-shape reduction: butterfly inside each wave (6 steps, no barrier), then the 16 wave partials in wave order
    double r1 = (a1[0] + a1[1]) + (a1[2] + a1[3]), r2 = (a2[0] + a2[1]) + (a2[2] + a2[3]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        r1 += __shfl_xor(r1, off);
        r2 += __shfl_xor(r2, off);
    }
    __shared__ double s1[16], s2[16];
    if ((tid & 63) == 0) {
        s1[tid >> 6] = r1;
        s2[tid >> 6] = r2;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 16; ++w) {
            s1[0] += s1[w];
            s2[0] += s2[w];
        }
    }
    if (tid == 0) {
        double t1 = s1[0], t2 = s2[0];
        bool last = true;
        if (S > 1) {
            const int row = nb * groups + g;
            double* part = &g_fin_part[slot][row][0][0];
            __hip_atomic_store(part + 2 * sl + 0, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(part + 2 * sl + 1, t2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned tk = __hip_atomic_fetch_add(&g_fin_ticket[slot][row], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = tk == (unsigned)(S - 1);
            if (last) {
                __hip_atomic_store(&g_fin_ticket[slot][row], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
                t1 = 0.0;
                t2 = 0.0;
                for (int k = 0; k < S; ++k) {
                    t1 += __hip_atomic_load(part + 2 * k + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    t2 += __hip_atomic_load(part + 2 * k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (last) {
            double* o = sums + ((long long)nb * groups + g) * 2;
            o[0] = (accumulate ? o[0] : 0.0) + t1;
            o[1] = (accumulate ? o[1] : 0.0) + t2;
        }
    }
}

extern "C" int ctsi_gn_finalize(const float* colsum, double* sums, int n, int c, int c_pad, int groups,
                                int tiles_per_sample, int nclass, int accumulate, void* stream) {
    CTSI_CHECK_ARG(colsum && sums, "ctsi_gn_finalize: null argument");
    CTSI_CHECK_ARG(groups > 0 && c % groups == 0, "ctsi_gn_finalize: c=%d not divisible by groups=%d", c, groups);
    const int cpg = c / groups;
    // slices: one per 2048 16-byte items of a (sample, group) (the vector path only), at most 64; scratch rows rotate over 4
    // slots per call so that consecutive launches never share one
    int S = 1;
    static int call_no = 0;
    if ((cpg & 3) == 0 && (c_pad & 3) == 0 && nclass == 1 && (long long)n * groups <= GN_FIN_ROWS) {
        const long long items4 = (long long)tiles_per_sample * (cpg >> 2);
        S = (int)(items4 / 2048);       // (round 4: 2048 instead of 8192 items per slice, up to 64 slices: the VAE's 8-group norms gave
                                        //  96 blocks of 256 KB each at full resolution -- 27 us per launch, latency-bound)
        if (S > GN_FIN_SMAX) S = GN_FIN_SMAX;
        if (S < 1) S = 1;
        static const char* fs = getenv("CTSI_GN_FIN_SPLIT");
        if (fs && atoi(fs) == 0) S = 1;
    }
    const int slot = S > 1 ? (call_no++ & (GN_FIN_SLOTS - 1)) : 0;
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(groups, n, S), dim3(1024), 0, (hipStream_t)stream, colsum, sums, n, c_pad,
                       groups, cpg, tiles_per_sample, nclass, accumulate, slot);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- apply --------------------------------------------------------------------------------------
// grid: (blocks_per_sample, n); block 256 (gn_fwd_grid of gn_frame.h).  The options are template parameters: with run-time flags
// the compiler if-converted both SiLU sites into unconditional code (2 exp + 2 rcp per element and a select chain: ~25 VALU
// instructions per element, 2.3 TB/s each way -- VALU-bound, not HBM-bound).  CONSTQ: the grid stride is a multiple of the row's
// chunk count, so a thread meets the same 8 channels every iteration and keeps their scale / shift / time bias in registers.
// The ResBlock's middle pass with the ADM-style options is the form <SILU_PRE, TB, no RES, no SILU_POST> plus
//   FILM  y = silu(gn(x) * (1 + s) + b) with a time row (s | b) of 2c values: the prologue only -- the per-(sample, channel)
//         coefficients become sc * (1 + s) and sh * (1 + s) + b, and no time bias is added afterwards;
//   DROP  y * keep * inv with the keep bits of ctsi_philox.h: one Philox call per 16-byte chunk, applied last, still in fp32.
template <bool SILU_PRE, bool TB, bool RES, bool SILU_POST, bool FILM, bool DROP, bool CONSTQ, bool NT>
__global__ void __launch_bounds__(256)
gn_apply_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, const double* __restrict__ sums,
                const float* __restrict__ gamma, const float* __restrict__ beta, int c, long long vox,
                long long vox_stat, int groups, float eps, const float* __restrict__ tbias, int tbias_stride,
                const int* __restrict__ step_ptr, int n_total, const bf16_t* __restrict__ residual, long long per_block,
                uint32_t thr, float inv_keep, const unsigned long long* __restrict__ seed_ptr, uint32_t layer_id) {
    constexpr bool ADD_TB = TB && !FILM;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_scale = reinterpret_cast<float*>(smem_raw);
    float* s_shift = s_scale + c;
    float* s_tb = s_shift + c;
    const int nb = blockIdx.y, tid = threadIdx.x;
    const int cpg = c / groups;
    const double cnt = (double)cpg * (double)vox_stat;
    long long trow = nb;
    if (TB && step_ptr) trow += (long long)(*step_ptr) * n_total;
    for (int ch = tid; ch < c; ch += 256) {
        const GnMeanRstd st = gn_mean_rstd(sums + ((long long)nb * groups + ch / cpg) * 2, cnt, eps);
        const float rstd = (float)st.rstd;
        const float sc = gamma[ch] * rstd;
        const float sh = beta[ch] - (float)st.mean * sc;
        if (FILM) {
            const float s1 = 1.0f + tbias[trow * tbias_stride + ch];
            s_scale[ch] = sc * s1;
            s_shift[ch] = sh * s1 + tbias[trow * tbias_stride + c + ch];
        } else {
            s_scale[ch] = sc;
            s_shift[ch] = sh;
            if (TB) s_tb[ch] = tbias[trow * tbias_stride + ch];
        }
    }
    __syncthreads();
    const unsigned long long seed = DROP ? *seed_ptr : 0ull;
    const int cpr = c >> 3;
    // per_block > 0: every block walks its own contiguous range of per_block chunks (stride 256); 0: grid-stride
    long long total = vox * cpr;
    const unsigned long long chunk0 = (unsigned long long)nb * (unsigned long long)total;   // first chunk of this sample
    const bf16_t* xb = x + (long long)nb * vox * c;
    bf16_t* yb = y + (long long)nb * vox * c;
    const bf16_t* rb = RES ? residual + (long long)nb * vox * c : nullptr;
    const long long stride = per_block > 0 ? 256 : (long long)gridDim.x * 256;
    const int dq = CONSTQ ? 0 : (int)(stride % cpr);
    constexpr int U = 4;   // independent 16-byte loads in flight per thread
    long long e = (per_block > 0 ? (long long)blockIdx.x * per_block : (long long)blockIdx.x * 256) + tid;
    if (per_block > 0 && (long long)(blockIdx.x + 1) * per_block < total) total = (long long)(blockIdx.x + 1) * per_block;
    int q = (int)(e % cpr);   // 8-channel chunk index inside the voxel row
    float csc[8], csh[8], ctb[8];
    auto coef = [&](int qq, float* sc, float* sh, float* tb) {   // 16-byte LDS reads
        gn_lds8(sc, s_scale, qq);
        gn_lds8(sh, s_shift, qq);
        if (ADD_TB) gn_lds8(tb, s_tb, qq);
    };
    if (CONSTQ) coef(q, csc, csh, ctb);
    // one dword = channels (2 j, 2 j + 1): the pair stays a 2-vector from the unpack to the single v_cvt_pk_bf16_f32
    auto one = [&](const uint4 raw, const uint4 rraw, long long ee, int qq) {
        float lsc[8], lsh[8], ltb[8];
        if (!CONSTQ) coef(qq, lsc, lsh, ltb);
        const float* sc = CONSTQ ? csc : lsc;
        const float* sh = CONSTQ ? csh : lsh;
        const float* tb = CONSTQ ? ctb : ltb;
        const uint32_t xin[4] = {raw.x, raw.y, raw.z, raw.w}, rin[4] = {rraw.x, rraw.y, rraw.z, rraw.w};
        uint32_t keep = 0xffu;
        if (DROP) keep = ctsi_dropout_keep8(chunk0 + (unsigned long long)ee, layer_id, seed, thr);
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x2_t v = {__uint_as_float(xin[j] << 16), __uint_as_float(xin[j] & 0xffff0000u)};
            const f32x2_t s2 = {sc[2 * j], sc[2 * j + 1]}, h2 = {sh[2 * j], sh[2 * j + 1]};
            v = v * s2 + h2;
            if (SILU_PRE) v = silu2_f(v);
            if (ADD_TB) v += f32x2_t{tb[2 * j], tb[2 * j + 1]};
            if (RES) v += f32x2_t{__uint_as_float(rin[j] << 16), __uint_as_float(rin[j] & 0xffff0000u)};
            if (SILU_POST) v = silu2_f(v);
            if (DROP) {
                v.x = (keep >> (2 * j)) & 1u ? v.x * inv_keep : 0.0f;
                v.y = (keep >> (2 * j + 1)) & 1u ? v.y * inv_keep : 0.0f;
            }
            o[j] = pack_bf16x2_v(v);
        }
        gn_st<NT>(yb + ee * 8, make_uint4(o[0], o[1], o[2], o[3]));
    };
    for (; e + (U - 1) * stride < total; e += U * stride) {
        uint4 raw[U], rraw[U];
        int qs[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            raw[u] = gn_ld<NT>(xb + (e + u * stride) * 8);
            rraw[u] = RES ? gn_ld<NT>(rb + (e + u * stride) * 8) : make_uint4(0, 0, 0, 0);
            qs[u] = q;
            if (!CONSTQ) q = (q + dq >= cpr) ? q + dq - cpr : q + dq;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) one(raw[u], rraw[u], e + u * stride, qs[u]);
    }
    for (; e < total; e += stride) {
        const uint4 raw = gn_ld<NT>(xb + e * 8);
        const uint4 rraw = RES ? gn_ld<NT>(rb + e * 8) : make_uint4(0, 0, 0, 0);
        one(raw, rraw, e, q);
        if (!CONSTQ) q = (q + dq >= cpr) ? q + dq - cpr : q + dq;
    }
}

typedef void (*gn_apply_fn)(const bf16_t*, bf16_t*, const double*, const float*, const float*, int, long long, long long, int,
                            float, const float*, int, const int*, int, const bf16_t*, long long, uint32_t, float,
                            const unsigned long long*, uint32_t);
// idx: bit 0 SILU_PRE, 1 TB, 2 RES, 3 SILU_POST, 4 CONSTQ, 5 NT -- the 64 forms of ctsi_gn_apply
template <int I>
static gn_apply_fn gn_apply_pick(int idx) {
    if constexpr (I >= 64) {
        return nullptr;
    } else {
        if (idx == I)
            return gn_apply_kernel<(I & 1) != 0, (I & 2) != 0, (I & 4) != 0, (I & 8) != 0, false, false, (I & 16) != 0, (I & 32) != 0>;
        return gn_apply_pick<I + 1>(idx);
    }
}
// idx: bit 0 FILM, 1 DROP, 2 CONSTQ, 3 NT -- the middle pass; neither option: the instantiation ctsi_gn_apply(silu_pre, tbias) runs
template <int I>
static gn_apply_fn gn_apply_mod_pick(int idx) {
    if constexpr (I >= 16) {
        return nullptr;
    } else {
        if (idx == I) return gn_apply_kernel<true, true, false, false, (I & 1) != 0, (I & 2) != 0, (I & 4) != 0, (I & 8) != 0>;
        return gn_apply_mod_pick<I + 1>(idx);
    }
}

static int gn_apply_launch(const void* x, void* y, const double* sums, const float* gamma, const float* beta, int n, int c, int d,
                           int h, int w, int d_stat, int groups, float eps, int silu_pre, const float* tbias, int tbias_stride,
                           const int* step_ptr, const void* residual, int silu_post, const GnOptions& mod, void* stream) {
    const long long vox = (long long)d * h * w;
    const GnFwdGrid g = gn_fwd_grid(n, c, vox);
    const size_t lds = (size_t)c * 3 * sizeof(float);
    const gn_apply_fn fn =
        mod.form()
            ? gn_apply_mod_pick<0>(mod.form() | (g.constq ? 4 : 0) | (g.nt ? 8 : 0))
            : gn_apply_pick<0>((silu_pre ? 1 : 0) | (tbias ? 2 : 0) | (residual ? 4 : 0) | (silu_post ? 8 : 0) |
                               (g.constq ? 16 : 0) | (g.nt ? 32 : 0));
    hipLaunchKernelGGL(fn, dim3((unsigned)g.blocks, n), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y, sums,
                       gamma, beta, c, vox, (long long)d_stat * h * w, groups, eps, tbias, tbias_stride, step_ptr, n,
                       (const bf16_t*)residual, g.per_block, mod.thr, mod.inv_keep, mod.seed,
                       mod.layer_id);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_gn_apply(const void* x, void* y, const double* sums, const float* gamma, const float* beta,
                             int n, int c, int d, int h, int w, int d_stat, int groups, float eps, int silu_pre,
                             const float* tbias, int tbias_stride, const int* step_ptr,
                             const void* residual, int silu_post, void* stream) {
    CTSI_CHECK_ARG(x && y && sums && gamma && beta, "ctsi_gn_apply: null argument");
    CTSI_CHECK_ARG(c % 8 == 0 && groups > 0 && c % groups == 0, "ctsi_gn_apply: bad c=%d groups=%d", c, groups);
    CTSI_CHECK_ARG(d_stat >= d, "ctsi_gn_apply: d_stat=%d < d=%d", d_stat, d);
    return gn_apply_launch(x, y, sums, gamma, beta, n, c, d, h, w, d_stat, groups, eps, silu_pre, tbias, tbias_stride, step_ptr,
                           residual, silu_post, GnOptions{}, stream);
}

extern "C" int ctsi_gn_apply_mod(const void* x, void* y, const double* sums, const float* gamma, const float* beta,
                                 int n, int c, int d, int h, int w, int d_stat, int groups, float eps, int silu_pre,
                                 const float* tbias, int tbias_stride, const int* step_ptr, const void* residual,
                                 int silu_post, int film, int p_thr16, float inv_keep, const void* seed, int layer_id,
                                 void* stream) {
    CTSI_CHECK_ARG(x && y && sums && gamma && beta, "ctsi_gn_apply_mod: null argument");
    CTSI_CHECK_ARG(c % 8 == 0 && c >= 8 && c <= 2048 && groups > 0 && c % groups == 0, "ctsi_gn_apply_mod: bad c=%d groups=%d", c, groups);
    CTSI_CHECK_ARG(n > 0 && d > 0 && h > 0 && w > 0 && d_stat >= d, "ctsi_gn_apply_mod: bad sizes (d_stat=%d, d=%d)", d_stat, d);
    CTSI_CHECK_ARG(silu_pre && tbias && !residual && !silu_post,
                   "ctsi_gn_apply_mod: the ResBlock's middle pass only (silu_pre, a time row, no residual, no outer SiLU)");
    CTSI_CHECK_ARG(tbias_stride >= (film ? 2 * c : c), "ctsi_gn_apply_mod: tbias_stride=%d shorter than the time row", tbias_stride);
    CTSI_CHECK_ARG(p_thr16 >= 0 && p_thr16 < 65536, "ctsi_gn_apply_mod: p_thr16=%d outside [0, 65536)", p_thr16);
    CTSI_CHECK_ARG(p_thr16 == 0 || seed, "ctsi_gn_apply_mod: dropout needs the seed buffer");
    CTSI_CHECK_ARG(layer_id >= 0, "ctsi_gn_apply_mod: layer_id=%d", layer_id);
    const GnOptions mod = {true, film ? 1 : 0, (uint32_t)p_thr16, inv_keep, (const unsigned long long*)seed, (uint32_t)layer_id};
    return gn_apply_launch(x, y, sums, gamma, beta, n, c, d, h, w, d_stat, groups, eps, 1, tbias, tbias_stride, step_ptr, nullptr,
                           0, mod, stream);
}

// ---- the dropout mask and the Philox function, for tests ------------------------------------------------------------------------
// keep bytes (1 = kept) of the first `count` elements of a layer's logical NDHWC tensor
__global__ void __launch_bounds__(256)
dropout_mask_kernel(const unsigned long long* __restrict__ seed_ptr, uint32_t layer_id, uint32_t thr, long long count,
                    unsigned char* __restrict__ out) {
    const long long chunk = (long long)blockIdx.x * 256 + threadIdx.x;
    if (chunk * 8 >= count) return;
    const uint32_t keep = ctsi_dropout_keep8((unsigned long long)chunk, layer_id, *seed_ptr, thr);
    for (int j = 0; j < 8; ++j)
        if (chunk * 8 + j < count) out[chunk * 8 + j] = (unsigned char)((keep >> j) & 1u);
}

extern "C" int ctsi_dropout_mask(const void* seed, int layer_id, int p_thr16, long long count, void* out_u8, void* stream) {
    CTSI_CHECK_ARG(seed && out_u8, "ctsi_dropout_mask: null argument");
    CTSI_CHECK_ARG(count > 0 && count <= (1ll << 40), "ctsi_dropout_mask: count=%lld", count);
    CTSI_CHECK_ARG(p_thr16 >= 0 && p_thr16 < 65536 && layer_id >= 0, "ctsi_dropout_mask: p_thr16=%d layer_id=%d", p_thr16,
                   layer_id);
    const long long chunks = (count + 7) / 8;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long*)seed, (uint32_t)layer_id, (uint32_t)p_thr16, count, (unsigned char*)out_u8);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_philox4x32_10_host(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
    CTSI_CHECK_ARG(ctr && key && out, "ctsi_philox4x32_10_host: null argument");
    ctsi_philox4x32_10(ctr, key, out);
    return CTSI_OK;
}

// host twin of ctsi_dropout_mask (the same inline function), for machines without a GPU
extern "C" int ctsi_dropout_mask_host(unsigned long long seed, int layer_id, int p_thr16, long long count, void* out_u8) {
    CTSI_CHECK_ARG(out_u8 && count > 0, "ctsi_dropout_mask_host: bad argument");
    CTSI_CHECK_ARG(p_thr16 >= 0 && p_thr16 < 65536 && layer_id >= 0, "ctsi_dropout_mask_host: p_thr16=%d layer_id=%d", p_thr16,
                   layer_id);
    unsigned char* out = (unsigned char*)out_u8;
    for (long long chunk = 0; chunk * 8 < count; ++chunk) {
        const uint32_t keep = ctsi_dropout_keep8((unsigned long long)chunk, (uint32_t)layer_id, seed, (uint32_t)p_thr16);
        for (int j = 0; j < 8 && chunk * 8 + j < count; ++j) out[chunk * 8 + j] = (unsigned char)((keep >> j) & 1u);
    }
    return CTSI_OK;
}
