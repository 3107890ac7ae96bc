// GroupNorm backward: the default pass (ctsi_gn_bwd: what autograd derives for models/unet3d.py:51-133) and the ResBlock's middle
// pass with the ADM-style options (ctsi_gn_bwd_mod), as ONE set of passes.
// forward (ctsi_gn_apply):  h = gn(x);  a = silu_pre ? silu(h) : h;  b = a + tbias;  c = b + residual;
//                           y = silu_post ? silu(c) : c
// backward: gc = dy * (silu_post ? silu'(c) : 1)   (= grad of residual; its per-sample channel sum = grad of tbias)
//           g  = gc * (silu_pre ? silu'(h) : 1)    (= grad of h)
//           dx = rstd * (gamma*g - mean_grp(gamma*g) - xhat * mean_grp(gamma*g*xhat))
//           dgamma = sum g*xhat, dbeta = sum g.
// middle pass with options:  h = xhat * G + B with the per-sample effective weight / bias
//             scale-shift: G = gamma * (1 + s), B = beta * (1 + s) + b;   additive: G = gamma, B = beta
//           y = drop( silu(h) [+ e] ),  drop(v) = v * keep * inv: the keep bits of ctsi_philox.h, a pure function of (seed, layer,
//           element), regenerated here
// backward: gc = dy * keep * inv;  g = gc * silu'(h)
//           d_b = sum_vox g;  d_s = gamma * sum g*xhat + beta * sum g;  d_e (additive) = sum_vox gc
//           dgamma = sum_n (1 + s) sum g*xhat;  dbeta = sum_n (1 + s) sum g
//           dx = rstd * (G*g - mean_grp(G*g) - xhat * mean_grp(G*g*xhat))
// Three passes: per-tile column sums (sum g, sum g*xhat, sum gc, sum xhat) -> per-(sample, group) terms and per-sample parameter
// partials -> dx.  Activations and their gradients are bf16 NDHWC with 16-byte (8-channel) accesses; statistics and parameter
// gradients are fp32 / fp64.  Reductions have a fixed order (deterministic, no float atomics).
#include "ctsi_internal.h"
#include "ctsi_philox.h"
#include "gn_frame.h"

// rstd, -mean * rstd and the effective weight / bias of every channel of sample nb, into LDS.  trow: the sample's time row (FILM)
template <bool FILM>
__device__ __forceinline__ void gn_bwd_coeffs(float* s_rs, float* s_mr, float* s_G, float* s_B, const double* sums,
                                              const float* gamma, const float* beta, const float* trow, int c, int groups,
                                              long long vox, float eps, int nb) {
    const int cpg = c / groups;
    const double cnt = (double)cpg * (double)vox;
    for (int ch = threadIdx.x; ch < c; ch += 256) {
        const GnMeanRstd st = gn_mean_rstd(sums + ((long long)nb * groups + ch / cpg) * 2, cnt, eps);
        const float rstd = (float)st.rstd;
        s_rs[ch] = rstd;
        s_mr[ch] = -(float)st.mean * rstd;
        if (FILM) {
            const float s1 = 1.0f + trow[ch];
            s_G[ch] = gamma[ch] * s1;
            s_B[ch] = beta[ch] * s1 + trow[c + ch];
        } else {
            s_G[ch] = gamma[ch];
            s_B[ch] = beta[ch];
        }
    }
}

// Pass 1: writes g (bf16, optional) and per-tile column sums [n][tiles][4][c] = (sum g, sum g*xhat, sum gc, sum xhat).
// grid (tiles, n), block 256.  dy may be a depth-broadcast tensor (n, 1, h, w, c): dy_mod = h*w, else 0.
// SILU_PRE / RES / SILU_POST are template parameters: as run-time flags the compiler evaluated both SiLU sites for every
// element and selected afterwards (the kernel was VALU-bound, like gn_apply before its options became template parameters).
// MOD (the middle pass with options: SILU_PRE alone, FILM / DROP): the residual stream, the depth-broadcast dy and the g buffer are
// absent at compile time.
template <bool SILU_PRE, bool RES, bool SILU_POST, bool MOD, bool FILM, bool DROP>
__global__ void __launch_bounds__(256)
gn_bwd_reduce_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, long long dy_mod_arg,
                     const double* __restrict__ sums, const float* __restrict__ gamma,
                     const float* __restrict__ beta, int c, long long vox, int groups, float eps,
                     const bf16_t* __restrict__ residual, bf16_t* __restrict__ g_out,
                     float* __restrict__ colsum, int tiles, int tile_rows, const float* __restrict__ tbias, int tbias_stride,
                     uint32_t thr, float inv_keep, const unsigned long long* __restrict__ seed_ptr, uint32_t layer_id) {
    static_assert(MOD || !(FILM || DROP), "FILM / DROP belong to the middle pass");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_rs = reinterpret_cast<float*>(smem_raw);   // rstd
    float* s_mr = s_rs + c;                              // -mean*rstd
    float* s_ga = s_mr + c;
    float* s_be = s_ga + c;
    float* s_red = s_be + c;                             // [rows_par][4][c]
    const int nb = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    gn_bwd_coeffs<FILM>(s_rs, s_mr, s_ga, s_be, sums, gamma, beta, FILM ? tbias + (long long)nb * tbias_stride : nullptr, c, groups,
                        vox, eps, nb);
    __syncthreads();
    const unsigned long long seed = DROP ? *seed_ptr : 0ull;
    const long long dy_mod = MOD ? 0 : dy_mod_arg;
    const int cpr = c >> 3;
    const int rows_par = 256 / cpr;
    const int q = tid % cpr, rl = tid / cpr;
    const long long v0 = (long long)tile * tile_rows;
    long long v1 = v0 + tile_rows;
    if (v1 > vox) v1 = vox;
    float a0[8], a1[8], a2[8], a3[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a0[k] = a1[k] = a2[k] = a3[k] = 0.0f;
    if (rl < rows_par) {
        const bf16_t* xb = x + (long long)nb * vox * c + q * 8;
        const bf16_t* rb = (RES && SILU_POST) ? residual + (long long)nb * vox * c + q * 8 : nullptr;
        bf16_t* gb = (!MOD && g_out != nullptr) ? g_out + (long long)nb * vox * c + q * 8 : nullptr;   // (NULL: pass 3 re-derives g)
        const bf16_t* db = dy + (long long)nb * (dy_mod ? dy_mod : vox) * c + q * 8;
        float rs[8], mr[8], ga[8], be[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            rs[k] = s_rs[q * 8 + k]; mr[k] = s_mr[q * 8 + k]; ga[k] = s_ga[q * 8 + k]; be[k] = s_be[q * 8 + k];
        }
        // 4 voxels per iteration: all 8-12 loads are issued before the first use (memory-level parallelism)
        constexpr int U = 4;
        for (long long vb = v0 + rl; vb < v1; vb += (long long)rows_par * U) {
            uint4 xr[U], dr[U], rr[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long v = vb + (long long)u * rows_par;
                if (v < v1) {
                    xr[u] = *reinterpret_cast<const uint4*>(xb + v * c);
                    const long long dv = dy_mod ? (v % dy_mod) : v;
                    dr[u] = *reinterpret_cast<const uint4*>(db + dv * c);
                    if (RES && SILU_POST) rr[u] = *reinterpret_cast<const uint4*>(rb + v * c);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long v = vb + (long long)u * rows_par;
                if (v >= v1) break;
                float xf[8], df[8], rf[8], gf[8];
                gn_unpack8(xr[u], xf);
                gn_unpack8(dr[u], df);
                if (RES && SILU_POST) gn_unpack8(rr[u], rf);
                uint32_t keep = 0xffu;
                if (DROP)
                    keep = ctsi_dropout_keep8(((unsigned long long)nb * (unsigned long long)vox + (unsigned long long)v) * cpr + q,
                                              layer_id, seed, thr);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float xh = xf[k] * rs[k] + mr[k];
                    const float h = xh * ga[k] + be[k];
                    float gc = df[k];
                    if (SILU_POST) {
                        float cc = SILU_PRE ? silu_f(h) : h;
                        if (RES) cc += rf[k];
                        gc *= silu_grad_f(cc);
                    }
                    if (DROP) gc = (keep >> k) & 1u ? gc * inv_keep : 0.0f;
                    float g = gc;
                    if (SILU_PRE) g *= silu_grad_f(h);
                    gf[k] = g;
                    a0[k] += g;
                    a1[k] += g * xh;
                    a2[k] += gc;
                    a3[k] += xh;
                }
                if (gb != nullptr) *reinterpret_cast<uint4*>(gb + v * c) = gn_pack8(gf);
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            s_red[(rl * 4 + 0) * c + q * 8 + k] = a0[k];
            s_red[(rl * 4 + 1) * c + q * 8 + k] = a1[k];
            s_red[(rl * 4 + 2) * c + q * 8 + k] = a2[k];
            s_red[(rl * 4 + 3) * c + q * 8 + k] = a3[k];
        }
    }
    __syncthreads();
    float* out = colsum + ((long long)nb * tiles + tile) * 4 * c;
    for (int e = tid; e < 4 * c; e += 256) {
        float t = 0.0f;
        for (int r = 0; r < rows_par; ++r) t += s_red[r * 4 * c + e];
        out[e] = t;
    }
}

// Pass 2a, default form: grid (group chunks, n), block 256.  A block owns `gpb` whole groups (CB = gpb*cpg <= max(64, cpg)
// channels) and 256/CB tile lanes; it sums the tiles, forms the group terms and writes per-sample partial grads:
//   s12[n][groups][2] = (sum_grp gamma*g, sum_grp gamma*g*xhat) / m
//   pgrad[n][4][c] = (sum g*xhat, sum g, sum gc, sum_v dx)   with  sum_v dx = rstd*(gamma*sum g - V*S1/m - S2/m*sum xhat)
//   (the last one is the bias gradient of the convolution that produced x)
__global__ void __launch_bounds__(256)
gn_bwd_finalize_kernel(const float* __restrict__ colsum, const float* __restrict__ gamma,
                       const double* __restrict__ sums, float eps, int c, long long vox, int groups, int tiles,
                       int gpb, float* __restrict__ s12, float* __restrict__ pgrad) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int cpg = c / groups;
    const int CB = gpb * cpg;
    const int TL = CB >= 256 ? 1 : 256 / CB;
    float* s_part = reinterpret_cast<float*>(smem_raw);   // [TL][4][CB]
    float* s_tot = s_part + TL * 4 * CB;                   // [4][CB]: sum g, sum g*xhat, sum gc, sum xhat
    float* s_g1 = s_tot + 4 * CB;                          // [gpb] S1/m
    float* s_g2 = s_g1 + gpb;
    const int nb = blockIdx.y, tid = threadIdx.x;
    const int g0 = blockIdx.x * gpb;
    const int ngr = min(gpb, groups - g0);
    const int c0 = g0 * cpg, cn = ngr * cpg;
    const float* base = colsum + (long long)nb * tiles * 4 * c + c0;
    for (int chl = tid % CB, tl = tid / CB; chl < cn && tl < TL; chl += 256 * ((CB + 255) / 256)) {
        float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
        int t = tl;
        for (; t + 3 * TL < tiles; t += 4 * TL) {       // 16 independent loads in flight (fixed order: deterministic)
            float r[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float* row = base + (long long)(t + u * TL) * 4 * c + chl;
                r[u][0] = row[0]; r[u][1] = row[c]; r[u][2] = row[2 * c]; r[u][3] = row[3 * c];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                t0 += r[u][0]; t1 += r[u][1]; t2 += r[u][2]; t3 += r[u][3];
            }
        }
        for (; t < tiles; t += TL) {
            const float* row = base + (long long)t * 4 * c + chl;
            t0 += row[0];
            t1 += row[c];
            t2 += row[2 * c];
            t3 += row[3 * c];
        }
        s_part[(tl * 4 + 0) * CB + chl] = t0;
        s_part[(tl * 4 + 1) * CB + chl] = t1;
        s_part[(tl * 4 + 2) * CB + chl] = t2;
        s_part[(tl * 4 + 3) * CB + chl] = t3;
        if (CB <= 256) break;
    }
    __syncthreads();
    for (int e = tid; e < 4 * CB; e += 256) {
        const int k = e / CB, chl = e - k * CB;
        float t = 0.0f;
        if (chl < cn)
            for (int tl = 0; tl < TL; ++tl) t += s_part[(tl * 4 + k) * CB + chl];
        s_tot[e] = t;
    }
    __syncthreads();
    const double cnt = (double)cpg * (double)vox;
    const float inv_m = (float)(1.0 / cnt);
    for (int g = tid; g < ngr; g += 256) {
        float sa = 0.0f, sb = 0.0f;
        for (int k = 0; k < cpg; ++k) {
            const float ga = gamma[c0 + g * cpg + k];
            sa += ga * s_tot[0 * CB + g * cpg + k];
            sb += ga * s_tot[1 * CB + g * cpg + k];
        }
        s_g1[g] = sa * inv_m;
        s_g2[g] = sb * inv_m;
        s12[((long long)nb * groups + g0 + g) * 2 + 0] = sa * inv_m;
        s12[((long long)nb * groups + g0 + g) * 2 + 1] = sb * inv_m;
    }
    __syncthreads();
    for (int chl = tid; chl < cn; chl += 256) {
        const int g = chl / cpg, ch = c0 + chl;
        const float rstd = (float)gn_mean_rstd(sums + ((long long)nb * groups + g0 + g) * 2, cnt, eps).rstd;
        pgrad[((long long)nb * 4 + 0) * c + ch] = s_tot[1 * CB + chl];
        pgrad[((long long)nb * 4 + 1) * c + ch] = s_tot[0 * CB + chl];
        pgrad[((long long)nb * 4 + 2) * c + ch] = s_tot[2 * CB + chl];
        pgrad[((long long)nb * 4 + 3) * c + ch] =
            rstd * (gamma[ch] * s_tot[0 * CB + chl] - (float)vox * s_g1[g] - s_g2[g] * s_tot[3 * CB + chl]);
    }
}

// Pass 2a, scale-shift / dropout form (a different design with its own summation order; the two stay side by side): grid
// (groups, n), block 1024: one block owns one (sample, group).  Every (statistic, channel) item of the group is
// summed over the tiles by TL = 1024 / items lanes, each in a fixed strided order with eight loads in flight, and the lanes are
// combined in lane order (deterministic: no atomics, no dependence on block scheduling).  A large tensor has thousands of tiles
// and only groups x n blocks here, so the pass is latency-bound: with 256 threads and four loads in flight the backward took
// 65 us (201 MB tensor) and 98 us (101 MB tensor) longer (profiles/resblock_options_bench.log, last block).  Writes
//   s12[n][groups][2] = (sum_grp G*gu, sum_grp G*gu*xhat) / m
//   pgrad[n][4][c]    = (sum gu*xhat, sum gu, sum ga, sum_vox dx)      sum_vox dx = rstd * (G * sum gu - V*S1/m - S2/m * sum xhat)
#define GNM_FIN_THREADS 1024
template <bool FILM>
__global__ void __launch_bounds__(GNM_FIN_THREADS)
gn_bwd_mod_finalize_kernel(const float* __restrict__ colsum, const float* __restrict__ gamma, const double* __restrict__ sums,
                           float eps, int c, long long vox, int groups, int tiles, const float* __restrict__ tbias,
                           int tbias_stride, float* __restrict__ s12, float* __restrict__ pgrad) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int cpg = c / groups;
    const int items = 4 * cpg;
    const int TL = items >= GNM_FIN_THREADS ? 1 : GNM_FIN_THREADS / items;
    float* s_part = reinterpret_cast<float*>(smem_raw);   // [TL][items]
    float* s_tot = s_part + TL * items;                    // [4][cpg]
    float* s_g = s_tot + items;                            // S1/m, S2/m
    const int g = blockIdx.x, nb = blockIdx.y, tid = threadIdx.x;
    const int c0 = g * cpg;
    const float* base = colsum + (long long)nb * tiles * 4 * c + c0;
    auto col = [&](int off, int t0, int step) {     // tiles t0, t0 + step, ...: eight loads in flight, fixed order
        float a[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        int tl = t0;
        for (; tl + 7 * step < tiles; tl += 8 * step) {
            float r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) r[u] = base[(long long)(tl + u * step) * 4 * c + off];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += r[u];
        }
#pragma unroll
        for (int u = 0; u < 7; ++u)       // at most seven tiles are left: a predicated, unrolled tail keeps a[] in registers
            if (tl + u * step < tiles) a[u] += base[(long long)(tl + u * step) * 4 * c + off];
        return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    };
    if (TL == 1) {
        for (int it = tid; it < items; it += GNM_FIN_THREADS) {
            const int k = it / cpg, chl = it - k * cpg;
            s_part[it] = col(k * c + chl, 0, 1);
        }
    } else if (tid < TL * items) {
        const int it = tid % items, lane = tid / items;
        const int k = it / cpg, chl = it - k * cpg;
        s_part[lane * items + it] = col(k * c + chl, lane, TL);
    }
    __syncthreads();
    for (int it = tid; it < items; it += GNM_FIN_THREADS) {
        float t = 0.0f;
        for (int lane = 0; lane < TL; ++lane) t += s_part[lane * items + it];
        s_tot[it] = t;
    }
    __syncthreads();
    const double cnt = (double)cpg * (double)vox;
    const float inv_m = (float)(1.0 / cnt);
    const float* trow = tbias + (long long)nb * tbias_stride;
    if (tid == 0) {
        float sa = 0.0f, sb = 0.0f;
        for (int k = 0; k < cpg; ++k) {
            const float G = FILM ? gamma[c0 + k] * (1.0f + trow[c0 + k]) : gamma[c0 + k];
            sa += G * s_tot[0 * cpg + k];
            sb += G * s_tot[1 * cpg + k];
        }
        s_g[0] = sa * inv_m;
        s_g[1] = sb * inv_m;
        s12[((long long)nb * groups + g) * 2 + 0] = sa * inv_m;
        s12[((long long)nb * groups + g) * 2 + 1] = sb * inv_m;
    }
    __syncthreads();
    const float rstd = (float)gn_mean_rstd(sums + ((long long)nb * groups + g) * 2, cnt, eps).rstd;
    for (int chl = tid; chl < cpg; chl += GNM_FIN_THREADS) {
        const int ch = c0 + chl;
        const float G = FILM ? gamma[ch] * (1.0f + trow[ch]) : gamma[ch];
        pgrad[((long long)nb * 4 + 0) * c + ch] = s_tot[1 * cpg + chl];
        pgrad[((long long)nb * 4 + 1) * c + ch] = s_tot[0 * cpg + chl];
        pgrad[((long long)nb * 4 + 2) * c + ch] = s_tot[2 * cpg + chl];
        pgrad[((long long)nb * 4 + 3) * c + ch] = rstd * (G * s_tot[0 * cpg + chl] - (float)vox * s_g[0] - s_g[1] * s_tot[3 * cpg + chl]);
    }
}

// Pass 2b: one thread per channel, samples in order.  dgamma[c] = sum_n pgrad[n][0][c], dbeta[c] = sum_n pgrad[n][1][c] (FILM: each
// sample's term times 1 + s); dtb (optional, row stride dtb_stride): dtb[n][ch] = pgrad[n][2][ch], FILM: dtb[n][ch] = d_s,
// dtb[n][c + ch] = d_b; dxsum[c] = sum_n pgrad[n][3][c] (optional).  gamma / beta / tbias are read by FILM only.
template <bool FILM>
__global__ void __launch_bounds__(256)
gn_bwd_param_kernel(const float* __restrict__ pgrad, int n, int c, const float* __restrict__ gamma,
                    const float* __restrict__ beta, const float* __restrict__ tbias, int tbias_stride,
                    float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dtb, long long dtb_stride,
                    float* __restrict__ dxsum) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= c) return;
    float a = 0.0f, b = 0.0f, d = 0.0f;
    const float ga = FILM ? gamma[ch] : 0.0f, be = FILM ? beta[ch] : 0.0f;
    for (int i = 0; i < n; ++i) {
        const float gx = pgrad[((long long)i * 4 + 0) * c + ch];     // sum g * xhat
        const float g1 = pgrad[((long long)i * 4 + 1) * c + ch];     // sum g
        d += pgrad[((long long)i * 4 + 3) * c + ch];
        if (FILM) {
            const float s1 = 1.0f + tbias[(long long)i * tbias_stride + ch];
            a += s1 * gx;
            b += s1 * g1;
            if (dtb) {
                dtb[(long long)i * dtb_stride + ch] = ga * gx + be * g1;
                dtb[(long long)i * dtb_stride + c + ch] = g1;
            }
        } else {
            a += gx;
            b += g1;
            if (dtb) dtb[(long long)i * dtb_stride + ch] = pgrad[((long long)i * 4 + 2) * c + ch];
        }
    }
    dgamma[ch] = a;
    dbeta[ch] = b;
    if (dxsum) dxsum[ch] = d;
}

// Pass 3: dx = rstd*(G*g - S1/m - xhat*S2/m) (+ add).  grid (blocks, n), block 256 (gn_bwd_apply_grid of gn_frame.h).  The stride
// is a multiple of the row's chunk count, so a thread keeps its 8 channels' coefficients in registers.  The two kernels below
// share the walk -- contig: one contiguous batch of 2 x 256 chunks per block, blocks in address order (see gn_fwd_grid); else
// grid-stride; two iterations (4-6 16-byte loads) in flight -- and differ in the element body, which body(gf, xf, e, of) holds.
struct GnBwdRange {
    long long e0, end, stride;
    int q;     // stride % cpr == 0: the same chunk every iteration
};
__device__ __forceinline__ GnBwdRange gn_bwd_range(long long total, int cpr, int contig) {
    GnBwdRange r;
    r.stride = contig ? 256 : (long long)gridDim.x * 256;
    r.e0 = (contig ? (long long)blockIdx.x * 512 : (long long)blockIdx.x * 256) + threadIdx.x;
    r.end = contig && (long long)(blockIdx.x + 1) * 512 < total ? (long long)(blockIdx.x + 1) * 512 : total;
    r.q = (int)(r.e0 % cpr);
    return r;
}
// BCAST: gb may be a depth-broadcast dy of dy_mod voxels per sample
template <bool ADD, bool BCAST, class Body>
__device__ __forceinline__ void gn_bwd_walk(const GnBwdRange r, const bf16_t* gb, const bf16_t* xb, const bf16_t* ab, bf16_t* ob,
                                            int cpr, long long dy_mod, Body body) {
    auto one = [&](const uint4 graw, const uint4 xraw, const uint4 araw, long long e) {
        float gf[8], xf[8], af[8], of[8];
        gn_unpack8(graw, gf);
        gn_unpack8(xraw, xf);
        if (ADD) gn_unpack8(araw, af);
        body(gf, xf, e, of);
        if (ADD) {
#pragma unroll
            for (int k = 0; k < 8; ++k) of[k] += af[k];
        }
        *reinterpret_cast<uint4*>(ob + e * 8) = gn_pack8(of);
    };
    const long long stride = r.stride;
    constexpr int U = 2;
    long long e = r.e0;
    for (; e + (U - 1) * stride < r.end; e += U * stride) {
        uint4 gr[U], xr[U], ar[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long eg = (BCAST && dy_mod) ? ((e + u * stride) / cpr % dy_mod) * cpr + r.q : e + u * stride;
            gr[u] = *reinterpret_cast<const uint4*>(gb + eg * 8);
            xr[u] = *reinterpret_cast<const uint4*>(xb + (e + u * stride) * 8);
            ar[u] = ADD ? *reinterpret_cast<const uint4*>(ab + (e + u * stride) * 8) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) one(gr[u], xr[u], ar[u], e + u * stride);
    }
    for (; e < r.end; e += stride) {
        const long long eg = (BCAST && dy_mod) ? (e / cpr % dy_mod) * cpr + r.q : e;
        one(*reinterpret_cast<const uint4*>(gb + eg * 8), *reinterpret_cast<const uint4*>(xb + e * 8),
            ADD ? *reinterpret_cast<const uint4*>(ab + e * 8) : make_uint4(0, 0, 0, 0), e);
    }
}

// Default form.  GMODE 0: g is read from pass 1's buffer; 1: g = dy * silu'(gn(x)) re-derived from dy (pass 1 wrote no g: nothing
// else needs it -- one tensor write less, and pass 3 re-reads what pass 1 just read through the Infinity Cache), rounded to bf16 as
// pass 1's buffer was; 2: g = dy (dy_mod > 0: a depth-broadcast dy).  In modes 1 / 2 `g` is dy.
template <bool ADD, int GMODE>
__global__ void __launch_bounds__(256)
gn_bwd_apply_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ x, const double* __restrict__ sums,
                    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ s12,
                    const bf16_t* __restrict__ add, bf16_t* __restrict__ dx, int c, long long vox, int groups,
                    float eps, int contig, long long dy_mod) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_rs = reinterpret_cast<float*>(smem_raw);
    float* s_mr = s_rs + c;
    float* s_ag = s_mr + c;   // rstd*gamma
    float* s_b1 = s_ag + c;   // rstd*S1/m
    float* s_b2 = s_b1 + c;   // rstd*S2/m
    const int nb = blockIdx.y, tid = threadIdx.x;
    const int cpg = c / groups;
    const double cnt = (double)cpg * (double)vox;
    for (int ch = tid; ch < c; ch += 256) {
        const int gi = ch / cpg;
        const GnMeanRstd st = gn_mean_rstd(sums + ((long long)nb * groups + gi) * 2, cnt, eps);
        const float rstd = (float)st.rstd;
        s_rs[ch] = rstd;
        s_mr[ch] = -(float)st.mean * rstd;
        s_ag[ch] = rstd * gamma[ch];
        s_b1[ch] = rstd * s12[((long long)nb * groups + gi) * 2 + 0];
        s_b2[ch] = rstd * s12[((long long)nb * groups + gi) * 2 + 1];
    }
    __syncthreads();
    const int cpr = c >> 3;
    const GnBwdRange r = gn_bwd_range(vox * cpr, cpr, contig);
    const int q = r.q;
    float rs[8], mr[8], ag[8], b1[8], b2[8], ga[8], be[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        ga[k] = GMODE == 1 ? gamma[q * 8 + k] : 0.0f;
        be[k] = GMODE == 1 ? beta[q * 8 + k] : 0.0f;
    }
    gn_lds8(rs, s_rs, q);
    gn_lds8(mr, s_mr, q);
    gn_lds8(ag, s_ag, q);
    gn_lds8(b1, s_b1, q);
    gn_lds8(b2, s_b2, q);
    gn_bwd_walk<ADD, GMODE != 0>(
        r, g + (long long)nb * ((GMODE != 0 && dy_mod) ? dy_mod : vox) * c, x + (long long)nb * vox * c,
        ADD ? add + (long long)nb * vox * c : nullptr, dx + (long long)nb * vox * c, cpr, dy_mod,
        [&](const float* gf, const float* xf, long long, float* of) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float xh = xf[k] * rs[k] + mr[k];
                float gg = gf[k];
                if (GMODE == 1) gg = bf16_to_f32(f32_to_bf16(gg * silu_grad_f(xh * ga[k] + be[k])));   // (rounded as pass 1's buffer was)
                of[k] = ag[k] * gg - b1[k] - xh * b2[k];
            }
        });
}

// Scale-shift / dropout form: g is re-derived from dy (no buffer for it exists) and stays in fp32: dx is rounded once, at the store.
template <bool FILM, bool DROP>
__global__ void __launch_bounds__(256)
gn_bwd_mod_apply_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const double* __restrict__ sums,
                        const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ s12,
                        bf16_t* __restrict__ dx, int c, long long vox, int groups, float eps, int contig,
                        const float* __restrict__ tbias, int tbias_stride, uint32_t thr, float inv_keep,
                        const unsigned long long* __restrict__ seed_ptr, uint32_t layer_id) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_rs = reinterpret_cast<float*>(smem_raw);
    float* s_mr = s_rs + c;
    float* s_G = s_mr + c;
    float* s_B = s_G + c;
    float* s_b1 = s_B + c;    // rstd*S1/m
    float* s_b2 = s_b1 + c;   // rstd*S2/m
    const int nb = blockIdx.y, tid = threadIdx.x;
    gn_bwd_coeffs<FILM>(s_rs, s_mr, s_G, s_B, sums, gamma, beta, tbias + (long long)nb * tbias_stride, c, groups, vox, eps, nb);
    __syncthreads();
    const int cpg = c / groups;
    for (int ch = tid; ch < c; ch += 256) {
        const int gi = ch / cpg;
        s_b1[ch] = s_rs[ch] * s12[((long long)nb * groups + gi) * 2 + 0];
        s_b2[ch] = s_rs[ch] * s12[((long long)nb * groups + gi) * 2 + 1];
    }
    __syncthreads();
    const unsigned long long seed = DROP ? *seed_ptr : 0ull;
    const int cpr = c >> 3;
    const long long total = vox * cpr;
    const unsigned long long chunk0 = (unsigned long long)nb * (unsigned long long)total;
    const GnBwdRange r = gn_bwd_range(total, cpr, contig);
    float rs[8], mr[8], G[8], B[8], b1[8], b2[8];
    gn_lds8(rs, s_rs, r.q);
    gn_lds8(mr, s_mr, r.q);
    gn_lds8(G, s_G, r.q);
    gn_lds8(B, s_B, r.q);
    gn_lds8(b1, s_b1, r.q);
    gn_lds8(b2, s_b2, r.q);
    gn_bwd_walk<false, false>(
        r, dy + (long long)nb * vox * c, x + (long long)nb * vox * c, nullptr, dx + (long long)nb * vox * c, cpr, 0,
        [&](const float* gf, const float* xf, long long e, float* of) {
            uint32_t keep = 0xffu;
            if (DROP) keep = ctsi_dropout_keep8(chunk0 + (unsigned long long)e, layer_id, seed, thr);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float xh = xf[k] * rs[k] + mr[k];
                float ga = gf[k];
                if (DROP) ga = (keep >> k) & 1u ? ga * inv_keep : 0.0f;
                const float gu = ga * silu_grad_f(xh * G[k] + B[k]);
                of[k] = rs[k] * (G[k] * gu) - b1[k] - xh * b2[k];
            }
        });
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
extern "C" int ctsi_gn_bwd_tiles(int d, int h, int w) {      // (tiles at the full 512-row tile; see gn_bwd_tile_rows)
    const long long vox = (long long)d * h * w;
    return (int)((vox + GN_BWD_TILE_ROWS - 1) / GN_BWD_TILE_ROWS);
}

typedef void (*gn_bwd_reduce_fn)(const bf16_t*, const bf16_t*, long long, const double*, const float*, const float*, int, long long,
                                 int, float, const bf16_t*, bf16_t*, float*, int, int, const float*, int, uint32_t, float,
                                 const unsigned long long*, uint32_t);

// pass 1 of both entry points
static int gn_bwd_reduce_launch(const char* api, const void* x, const void* dy, long long dy_mod, const double* sums,
                                const float* gamma, const float* beta, int n, int c, long long vox, int groups, float eps,
                                int silu_pre, const void* residual, int silu_post, void* g_buf, float* colsum,
                                const GnBwdWorkspace& ws, const float* tbias, int tbias_stride, const GnOptions& mod,
                                hipStream_t st) {
    const int rows_par = 256 / (c >> 3);
    const size_t lds1 = (size_t)(4 * c + rows_par * 4 * c) * sizeof(float);
    CTSI_CHECK_ARG(lds1 <= 160 * 1024, "%s: LDS budget exceeded for c=%d", api, c);
    static const gn_bwd_reduce_fn tab[8] = {
        gn_bwd_reduce_kernel<false, false, false, false, false, false>, gn_bwd_reduce_kernel<true, false, false, false, false, false>,
        gn_bwd_reduce_kernel<false, true, false, false, false, false>,  gn_bwd_reduce_kernel<true, true, false, false, false, false>,
        gn_bwd_reduce_kernel<false, false, true, false, false, false>,  gn_bwd_reduce_kernel<true, false, true, false, false, false>,
        gn_bwd_reduce_kernel<false, true, true, false, false, false>,   gn_bwd_reduce_kernel<true, true, true, false, false, false>};
    static const gn_bwd_reduce_fn mod_tab[4] = {
        gn_bwd_reduce_kernel<true, false, false, true, false, false>, gn_bwd_reduce_kernel<true, false, false, true, true, false>,
        gn_bwd_reduce_kernel<true, false, false, true, false, true>,  gn_bwd_reduce_kernel<true, false, false, true, true, true>};
    const gn_bwd_reduce_fn reduce = mod.mod ? mod_tab[mod.form()]
                                              : tab[(silu_pre ? 1 : 0) | (residual ? 2 : 0) | (silu_post ? 4 : 0)];
    if (lds1 > 64 * 1024)
        CTSI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(reduce),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
    hipLaunchKernelGGL(reduce, dim3(ws.tiles, n), dim3(256), lds1, st, (const bf16_t*)x, (const bf16_t*)dy, dy_mod, sums, gamma,
                       beta, c, vox, groups, eps, (const bf16_t*)residual, (bf16_t*)g_buf, colsum, ws.tiles, ws.tile_rows,
                       tbias, tbias_stride, mod.thr, mod.inv_keep, mod.seed, mod.layer_id);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

static int gn_bwd_param_launch(const float* pgrad, int n, int c, const float* gamma, const float* beta, const float* tbias,
                               int tbias_stride, int film,                               float* dgamma, float* dbeta, float* dtbias, long long dtbias_stride, float* dxsum, hipStream_t st) {
    hipLaunchKernelGGL(film ? gn_bwd_param_kernel<true> : gn_bwd_param_kernel<false>, dim3((c + 255) / 256), dim3(256), 0, st,
                       pgrad, n, c, gamma, beta, tbias, tbias_stride, dgamma, dbeta, dtbias, dtbias_stride, dxsum);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_gn_bwd(const void* x, const void* dy, int dy_bcast_d, const double* sums, const float* gamma,
                           const float* beta, int n, int c, int d, int h, int w, int groups, float eps, int silu_pre,
                           const void* residual, int silu_post, const void* add, void* g_buf, void* dx,
                           float* workspace, float* dgamma, float* dbeta, float* dtbias, long long dtbias_stride,
                           float* dxsum, void* stream) {
    CTSI_CHECK_ARG(x && dy && sums && gamma && beta && dx && workspace && dgamma && dbeta,
                   "ctsi_gn_bwd: null argument");
    // g_buf may be NULL when nothing but pass 3 needs the GroupNorm output's gradient: pass 3 re-derives it from dy
    CTSI_CHECK_ARG(g_buf || (!residual && !silu_post), "ctsi_gn_bwd: g_buf may only be omitted without residual / post-SiLU");
    CTSI_CHECK_ARG(c % 8 == 0 && c <= 2048 && groups > 0 && c % groups == 0, "ctsi_gn_bwd: bad c=%d groups=%d", c,
                   groups);
    const long long vox = (long long)d * h * w;
    const GnBwdWorkspace ws(n, c, vox, groups);
    const int tiles = ws.tiles;
    hipStream_t st = (hipStream_t)stream;
    float* colsum = workspace;
    float* s12 = workspace + ws.s12_off;
    float* pgrad = workspace + ws.pgrad_off;
    CTSI_CHECK_ARG(256 / (c >> 3) >= 1, "ctsi_gn_bwd: c=%d too wide", c);
    int rc = gn_bwd_reduce_launch("ctsi_gn_bwd", x, dy, dy_bcast_d ? (long long)h * w : 0ll, sums, gamma, beta, n, c, vox, groups,
                                  eps, silu_pre, residual, silu_post, g_buf, colsum, ws, nullptr, 0, GnOptions{}, st);
    if (rc != CTSI_OK) return rc;
    {
        const int cpg = c / groups;
        // channels per block: 64 (4 tile lanes) when there are few tiles; 16 (16 lanes, 4 x the blocks) when a (sample, group)
        // has many -- with the smaller statistics tiles of pass 1 a 4-lane block walked up to 216 tile rows one batch after
        // the other (21 us per launch on average against 9 before the tile change)
        int gpb = (tiles > 32 ? 16 : 64) / cpg;
        if (gpb < 1) gpb = 1;
        if (gpb > groups) gpb = groups;
        const int CB = gpb * cpg;
        const int TL = CB >= 256 ? 1 : 256 / CB;
        const size_t lds2 = (size_t)(TL * 4 * CB + 4 * CB + 2 * gpb) * sizeof(float);
        hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3((groups + gpb - 1) / gpb, n), dim3(256), lds2, st, colsum, gamma,
                           sums, eps, c, vox, groups, tiles, gpb, s12, pgrad);
    }
    CTSI_LAUNCH_CHECK();
    rc = gn_bwd_param_launch(pgrad, n, c, gamma, beta, nullptr, 0, 0, dgamma, dbeta, dtbias, dtbias_stride, dxsum, st);
    if (rc != CTSI_OK) return rc;
    const GnBwdGrid grid = gn_bwd_apply_grid(c, vox);
    {
        typedef void (*apply_fn)(const bf16_t*, const bf16_t*, const double*, const float*, const float*, const float*,
                                 const bf16_t*, bf16_t*, int, long long, int, float, int, long long);
        static const apply_fn apply_tab[6] = {gn_bwd_apply_kernel<false, 0>, gn_bwd_apply_kernel<true, 0>,
                                              gn_bwd_apply_kernel<false, 1>, gn_bwd_apply_kernel<true, 1>,
                                              gn_bwd_apply_kernel<false, 2>, gn_bwd_apply_kernel<true, 2>};
        const int gmode = g_buf ? 0 : (silu_pre ? 1 : 2);
        const long long dy_mod = (gmode != 0 && dy_bcast_d) ? (long long)h * w : 0ll;
        hipLaunchKernelGGL(apply_tab[gmode * 2 + (add ? 1 : 0)], dim3((unsigned)grid.blocks, n), dim3(256), 5 * c * sizeof(float),
                           st, (const bf16_t*)(g_buf ? g_buf : dy), (const bf16_t*)x, sums, gamma, beta, s12, (const bf16_t*)add,
                           (bf16_t*)dx, c, vox, groups, eps, grid.contig, dy_mod);
    }
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" size_t ctsi_gn_bwd_workspace_floats(int n, int c, int d, int h, int w, int groups) {
    return (size_t)GnBwdWorkspace(n, c, (long long)d * h * w, groups).floats;
}

extern "C" size_t ctsi_gn_bwd_mod_workspace_floats(int n, int c, int d, int h, int w, int groups) {
    if (n <= 0 || c < 8 || c % 8 != 0 || c > 2048 || groups <= 0) return 0;
    return (size_t)GnBwdWorkspace(n, c, (long long)d * h * w, groups).floats;
}

extern "C" int ctsi_gn_bwd_mod(const void* x, const void* dy, const double* sums, const float* gamma, const float* beta,
                               int n, int c, int d, int h, int w, int groups, float eps, const float* tbias, int tbias_stride,
                               int film, int p_thr16, float inv_keep, const void* seed, int layer_id, void* dx,
                               float* workspace, float* dgamma, float* dbeta, float* dtbias, long long dtbias_stride,
                               float* dxsum, void* stream) {
    CTSI_CHECK_ARG(x && dy && sums && gamma && beta && dx && workspace && dgamma && dbeta && tbias,
                   "ctsi_gn_bwd_mod: null argument");
    CTSI_CHECK_ARG(c % 8 == 0 && c >= 8 && c <= 2048 && groups > 0 && c % groups == 0, "ctsi_gn_bwd_mod: bad c=%d groups=%d", c,
                   groups);
    CTSI_CHECK_ARG(n > 0 && d > 0 && h > 0 && w > 0, "ctsi_gn_bwd_mod: sizes must be positive");
    CTSI_CHECK_ARG(tbias_stride >= (film ? 2 * c : c), "ctsi_gn_bwd_mod: tbias_stride=%d shorter than the time row", tbias_stride);
    CTSI_CHECK_ARG(!dtbias || dtbias_stride >= (film ? 2 * c : c), "ctsi_gn_bwd_mod: dtbias_stride shorter than the time row");
    CTSI_CHECK_ARG(p_thr16 >= 0 && p_thr16 < 65536, "ctsi_gn_bwd_mod: p_thr16=%d outside [0, 65536)", p_thr16);
    CTSI_CHECK_ARG(p_thr16 == 0 || seed, "ctsi_gn_bwd_mod: dropout needs the seed buffer");
    CTSI_CHECK_ARG(layer_id >= 0, "ctsi_gn_bwd_mod: layer_id=%d", layer_id);
    const long long vox = (long long)d * h * w;
    const GnBwdWorkspace ws(n, c, vox, groups);
    const int tiles = ws.tiles;
    hipStream_t st = (hipStream_t)stream;
    float* colsum = workspace;
    float* s12 = workspace + ws.s12_off;
    float* pgrad = workspace + ws.pgrad_off;
    const GnOptions mod = {true, film ? 1 : 0, (uint32_t)p_thr16, inv_keep, (const unsigned long long*)seed, (uint32_t)layer_id};
    int rc = gn_bwd_reduce_launch("ctsi_gn_bwd_mod", x, dy, 0ll, sums, gamma, beta, n, c, vox, groups, eps, 1, nullptr, 0, nullptr,
                                  colsum, ws, tbias, tbias_stride, mod, st);
    if (rc != CTSI_OK) return rc;
    {
        const int cpg = c / groups;
        const int items = 4 * cpg;
        const int TL = items >= GNM_FIN_THREADS ? 1 : GNM_FIN_THREADS / items;
        const size_t lds2 = (size_t)(TL * items + items + 2) * sizeof(float);
        CTSI_CHECK_ARG(lds2 <= 64 * 1024, "ctsi_gn_bwd_mod: c / groups = %d channels per group exceed the finalize pass's LDS", cpg);
        hipLaunchKernelGGL(film ? gn_bwd_mod_finalize_kernel<true> : gn_bwd_mod_finalize_kernel<false>, dim3(groups, n),
                           dim3(GNM_FIN_THREADS), lds2, st, colsum, gamma, sums, eps, c, vox, groups, tiles, tbias, tbias_stride, s12,
                           pgrad);
        CTSI_LAUNCH_CHECK();
    }
    rc = gn_bwd_param_launch(pgrad, n, c, gamma, beta, tbias, tbias_stride, mod.film, dgamma, dbeta, dtbias, dtbias_stride, dxsum, st);
    if (rc != CTSI_OK) return rc;
    const GnBwdGrid grid = gn_bwd_apply_grid(c, vox);
    {
        typedef void (*fn_t)(const bf16_t*, const bf16_t*, const double*, const float*, const float*, const float*, bf16_t*, int,
                             long long, int, float, int, const float*, int, uint32_t, float, const unsigned long long*, uint32_t);
        static const fn_t tab[4] = {gn_bwd_mod_apply_kernel<false, false>, gn_bwd_mod_apply_kernel<true, false>,
                                    gn_bwd_mod_apply_kernel<false, true>, gn_bwd_mod_apply_kernel<true, true>};
        hipLaunchKernelGGL(tab[mod.form()], dim3((unsigned)grid.blocks, n), dim3(256), 6 * c * sizeof(float), st,
                           (const bf16_t*)dy, (const bf16_t*)x, sums, gamma, beta, s12, (bf16_t*)dx, c, vox, groups, eps,
                           grid.contig, tbias, tbias_stride, mod.thr, inv_keep, mod.seed, mod.layer_id);
        CTSI_LAUNCH_CHECK();
    }
    return CTSI_OK;
}
