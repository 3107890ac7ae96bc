// The ResBlock's middle pass with the ADM-style options: the GroupNorm pass that produces conv2's input,
//   additive      y = drop( silu(gn(x)) + e )                       e: one time row of c values
//   scale-shift   y = drop( silu(gn(x) * (1 + s) + b) )             (s | b): one time row of 2c values, scale first
// and its backward.  drop(v) = v * keep * inv with the keep bits of ctsi_philox.h: a pure function of (seed, layer, element),
// regenerated in the backward.  Same layout rules as norm_act.hip / train_ops.hip: bf16 NDHWC, 16-byte (8-channel) accesses,
// fp32 arithmetic with one rounding at the store, fixed-order reductions without float atomics.
// The default passes (ctsi_gn_apply, ctsi_gn_apply_f32, ctsi_gn_bwd) are untouched: these entry points serve the option modes only.
#include "ctsi_internal.h"
#include "ctsi_philox.h"
#include <math.h>
#include <stdlib.h>

#define GNM_TILE_ROWS 512

typedef unsigned int gnm_u4_t __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ uint4 gnm_ld(const bf16_t* p) {
    if (NT) {
        const gnm_u4_t v = __builtin_nontemporal_load(reinterpret_cast<const gnm_u4_t*>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    return *reinterpret_cast<const uint4*>(p);
}
template <bool NT>
__device__ __forceinline__ void gnm_st(bf16_t* p, const uint4 v) {
    if (NT) {
        const gnm_u4_t w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, reinterpret_cast<gnm_u4_t*>(p));
    } else {
        *reinterpret_cast<uint4*>(p) = v;
    }
}
__device__ __forceinline__ void m_unpack8(const uint4 v, float* f) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
__device__ __forceinline__ uint4 m_pack8(const float* f) {
    uint4 v;
    v.x = pack_bf16x2(f[0], f[1]); v.y = pack_bf16x2(f[2], f[3]);
    v.z = pack_bf16x2(f[4], f[5]); v.w = pack_bf16x2(f[6], f[7]);
    return v;
}
__device__ __forceinline__ float m_silu_grad_f(float z) {     // d/dz [z * sigmoid(z)], as train_ops.hip
    const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * z));
    return s * (1.0f + z * (1.0f - s));
}

// ---- forward, bf16 ----------------------------------------------------------------------------------------------------
// gn_apply_kernel of norm_act.hip (which documents the launch forms) with SILU_PRE and the time row always on, no residual, no
// outer SiLU.  FILM changes the prologue only: the per-(sample, channel) coefficients become sc * (1 + s) and sh * (1 + s) + b.
// DROP: one Philox call per 16-byte chunk, applied last, still in fp32.
template <bool FILM, bool DROP, bool CONSTQ, bool NT>
__global__ void __launch_bounds__(256)
gn_apply_mod_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, const double* __restrict__ sums,
                    const float* __restrict__ gamma, const float* __restrict__ beta, int c, long long vox,
                    long long vox_stat, int groups, float eps, const float* __restrict__ tbias, int tbias_stride,
                    const int* __restrict__ step_ptr, int n_total, long long per_block, uint32_t thr, float inv_keep,
                    const unsigned long long* __restrict__ seed_ptr, uint32_t layer_id) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_scale = reinterpret_cast<float*>(smem_raw);
    float* s_shift = s_scale + c;
    float* s_tb = s_shift + c;
    const int nb = blockIdx.y, tid = threadIdx.x;
    const int cpg = c / groups;
    const double cnt = (double)cpg * (double)vox_stat;
    long long trow = nb;
    if (step_ptr) trow += (long long)(*step_ptr) * n_total;
    for (int ch = tid; ch < c; ch += 256) {
        const int g = ch / cpg;
        const double m = sums[((long long)nb * groups + g) * 2 + 0] / cnt;
        double var = sums[((long long)nb * groups + g) * 2 + 1] / cnt - m * m;
        if (var < 0.0) var = 0.0;
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        const float sc = gamma[ch] * rstd;
        const float sh = beta[ch] - (float)m * sc;
        if (FILM) {
            const float s1 = 1.0f + tbias[trow * tbias_stride + ch];
            s_scale[ch] = sc * s1;
            s_shift[ch] = sh * s1 + tbias[trow * tbias_stride + c + ch];
        } else {
            s_scale[ch] = sc;
            s_shift[ch] = sh;
            s_tb[ch] = tbias[trow * tbias_stride + ch];
        }
    }
    __syncthreads();
    const unsigned long long seed = DROP ? *seed_ptr : 0ull;
    const int cpr = c >> 3;
    long long total = vox * cpr;
    const unsigned long long chunk0 = (unsigned long long)nb * (unsigned long long)total;   // first chunk of this sample
    const bf16_t* xb = x + (long long)nb * vox * c;
    bf16_t* yb = y + (long long)nb * vox * c;
    const long long stride = per_block > 0 ? 256 : (long long)gridDim.x * 256;
    const int dq = CONSTQ ? 0 : (int)(stride % cpr);
    constexpr int U = 4;
    long long e = (per_block > 0 ? (long long)blockIdx.x * per_block : (long long)blockIdx.x * 256) + tid;
    if (per_block > 0 && (long long)(blockIdx.x + 1) * per_block < total) total = (long long)(blockIdx.x + 1) * per_block;
    int q = (int)(e % cpr);
    float csc[8], csh[8], ctb[8];
    auto coef = [&](int qq, float* sc, float* sh, float* tb) {
        *reinterpret_cast<float4*>(sc) = *reinterpret_cast<const float4*>(s_scale + qq * 8);
        *reinterpret_cast<float4*>(sc + 4) = *reinterpret_cast<const float4*>(s_scale + qq * 8 + 4);
        *reinterpret_cast<float4*>(sh) = *reinterpret_cast<const float4*>(s_shift + qq * 8);
        *reinterpret_cast<float4*>(sh + 4) = *reinterpret_cast<const float4*>(s_shift + qq * 8 + 4);
        if (!FILM) {
            *reinterpret_cast<float4*>(tb) = *reinterpret_cast<const float4*>(s_tb + qq * 8);
            *reinterpret_cast<float4*>(tb + 4) = *reinterpret_cast<const float4*>(s_tb + qq * 8 + 4);
        }
    };
    if (CONSTQ) coef(q, csc, csh, ctb);
    auto one = [&](const uint4 raw, long long ee, int qq) {
        float lsc[8], lsh[8], ltb[8];
        if (!CONSTQ) coef(qq, lsc, lsh, ltb);
        const float* sc = CONSTQ ? csc : lsc;
        const float* sh = CONSTQ ? csh : lsh;
        const float* tb = CONSTQ ? ctb : ltb;
        const uint32_t xin[4] = {raw.x, raw.y, raw.z, raw.w};
        uint32_t keep = 0xffu;
        if (DROP) keep = ctsi_dropout_keep8(chunk0 + (unsigned long long)ee, layer_id, seed, thr);
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x2_t v = {__uint_as_float(xin[j] << 16), __uint_as_float(xin[j] & 0xffff0000u)};
            const f32x2_t s2 = {sc[2 * j], sc[2 * j + 1]}, h2 = {sh[2 * j], sh[2 * j + 1]};
            v = v * s2 + h2;
            v = silu2_f(v);
            if (!FILM) v += f32x2_t{tb[2 * j], tb[2 * j + 1]};
            if (DROP) {
                v.x = (keep >> (2 * j)) & 1u ? v.x * inv_keep : 0.0f;
                v.y = (keep >> (2 * j + 1)) & 1u ? v.y * inv_keep : 0.0f;
            }
            o[j] = pack_bf16x2_v(v);
        }
        gnm_st<NT>(yb + ee * 8, make_uint4(o[0], o[1], o[2], o[3]));
    };
    for (; e + (U - 1) * stride < total; e += U * stride) {
        uint4 raw[U];
        int qs[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            raw[u] = gnm_ld<NT>(xb + (e + u * stride) * 8);
            qs[u] = q;
            if (!CONSTQ) q = (q + dq >= cpr) ? q + dq - cpr : q + dq;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) one(raw[u], e + u * stride, qs[u]);
    }
    for (; e < total; e += stride) {
        one(gnm_ld<NT>(xb + e * 8), e, q);
        if (!CONSTQ) q = (q + dq >= cpr) ? q + dq - cpr : q + dq;
    }
}

typedef void (*gn_apply_mod_fn)(const bf16_t*, bf16_t*, const double*, const float*, const float*, int, long long, long long, int,
                                float, const float*, int, const int*, int, long long, uint32_t, float,
                                const unsigned long long*, uint32_t);
template <int I>
static gn_apply_mod_fn gn_apply_mod_pick(int idx) {
    if constexpr (I >= 16) {
        return nullptr;
    } else {
        if (idx == I) return gn_apply_mod_kernel<(I & 1) != 0, (I & 2) != 0, (I & 4) != 0, (I & 8) != 0>;
        return gn_apply_mod_pick<I + 1>(idx);
    }
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
    const long long vox = (long long)d * h * w;
    const long long total = vox * (c / 8);
    long long blocks = (total + 256 * 8 - 1) / (256 * 8);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    const int cpr = c / 8;
    int gq = cpr, g256 = 256;
    while (g256) { const int t = gq % g256; gq = g256; g256 = t; }
    const int need = cpr / gq;
    if (blocks >= need) blocks -= blocks % need;
    bool constq = (blocks * 256) % cpr == 0;
    long long per_block = 0;
    {
        static const char* cg = getenv("CTSI_GN_CONTIG");
        if (!(cg && atoi(cg) == 0) && 256 % cpr == 0) {
            per_block = 1024;
            blocks = (total + per_block - 1) / per_block;
            constq = true;
        }
    }
    const size_t lds = (size_t)c * 3 * sizeof(float);
    static const char* nt_env = getenv("CTSI_GN_NT");
    const bool nt = nt_env ? atoi(nt_env) != 0 : (long long)n * vox * c * 2 > (512ll << 20);
    const int idx = (film ? 1 : 0) | (p_thr16 > 0 ? 2 : 0) | (constq ? 4 : 0) | (nt ? 8 : 0);
    hipLaunchKernelGGL(gn_apply_mod_pick<0>(idx), dim3((unsigned)blocks, n), dim3(256), lds, (hipStream_t)stream,
                       (const bf16_t*)x, (bf16_t*)y, sums, gamma, beta, c, vox, (long long)d_stat * h * w, groups, eps,
                       tbias, tbias_stride, step_ptr, n, per_block, (uint32_t)p_thr16, inv_keep,
                       (const unsigned long long*)seed, (uint32_t)layer_id);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- forward, fp32 activations (engine_f32.py: inference, so no dropout) -------------------------------------------------
// gn_apply_f32_kernel of f32_ops.hip with SILU_PRE and the time row on; accurate expf.
template <bool FILM, bool V4>
__global__ void __launch_bounds__(256)
gn_apply_mod_f32_kernel(const float* __restrict__ x, float* __restrict__ y, const double* __restrict__ sums,
                        const float* __restrict__ gamma, const float* __restrict__ beta, int c, long long vox, long long vox_stat,
                        int groups, float eps, const float* __restrict__ tbias, int tbias_stride,
                        const int* __restrict__ step_ptr, int n_total) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_scale = reinterpret_cast<float*>(smem_raw);
    float* s_shift = s_scale + c;
    float* s_tb = s_shift + c;
    const int nb = blockIdx.y, tid = threadIdx.x;
    const int cpg = c / groups;
    const double cnt = (double)cpg * (double)vox_stat;
    long long trow = nb;
    if (step_ptr) trow += (long long)(*step_ptr) * n_total;
    for (int ch = tid; ch < c; ch += 256) {
        const int g = ch / cpg;
        const double m = sums[((long long)nb * groups + g) * 2 + 0] / cnt;
        double var = sums[((long long)nb * groups + g) * 2 + 1] / cnt - m * m;
        if (var < 0.0) var = 0.0;
        const double rstd = 1.0 / sqrt(var + (double)eps);
        const double sc = (double)gamma[ch] * rstd, sh = (double)beta[ch] - m * sc;
        if (FILM) {
            const double s1 = 1.0 + (double)tbias[trow * tbias_stride + ch];
            s_scale[ch] = (float)(sc * s1);
            s_shift[ch] = (float)(sh * s1 + (double)tbias[trow * tbias_stride + c + ch]);
            s_tb[ch] = 0.0f;
        } else {
            s_scale[ch] = (float)sc;
            s_shift[ch] = (float)sh;
            s_tb[ch] = tbias[trow * tbias_stride + ch];
        }
    }
    __syncthreads();
    const float* xb = x + (long long)nb * vox * c;
    float* yb = y + (long long)nb * vox * c;
    auto one = [&](float v, int ch) {
        v = v * s_scale[ch] + s_shift[ch];
        v = v / (1.0f + expf(-v));
        if (!FILM) v += s_tb[ch];
        return v;
    };
    const long long stride = (long long)gridDim.x * 256;
    if (V4) {
        const int c4 = c >> 2;
        const long long total = vox * c4;
        for (long long e = (long long)blockIdx.x * 256 + tid; e < total; e += stride) {
            const int ch = (int)(e % c4) * 4;
            const float4 xv = reinterpret_cast<const float4*>(xb)[e];
            float4 o;
            o.x = one(xv.x, ch);
            o.y = one(xv.y, ch + 1);
            o.z = one(xv.z, ch + 2);
            o.w = one(xv.w, ch + 3);
            reinterpret_cast<float4*>(yb)[e] = o;
        }
    } else {
        const long long total = vox * c;
        for (long long e = (long long)blockIdx.x * 256 + tid; e < total; e += stride) yb[e] = one(xb[e], (int)(e % c));
    }
}

extern "C" int ctsi_gn_apply_mod_f32(const float* x, float* y, const double* sums, const float* gamma, const float* beta, int n,
                                     int c, int d, int h, int w, int d_stat, int groups, float eps, int silu_pre,
                                     const float* tbias, int tbias_stride, const int* step_ptr, const float* residual,
                                     int silu_post, int film, void* stream) {
    CTSI_CHECK_ARG(x && y && sums && gamma && beta, "ctsi_gn_apply_mod_f32: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && c <= 4096 && d > 0 && h > 0 && w > 0, "ctsi_gn_apply_mod_f32: bad sizes (c=%d)", c);
    CTSI_CHECK_ARG(groups > 0 && c % groups == 0, "ctsi_gn_apply_mod_f32: c=%d not divisible by groups=%d", c, groups);
    CTSI_CHECK_ARG(d_stat >= d, "ctsi_gn_apply_mod_f32: d_stat=%d < d=%d", d_stat, d);
    CTSI_CHECK_ARG(silu_pre && tbias && !residual && !silu_post,
                   "ctsi_gn_apply_mod_f32: the ResBlock's middle pass only (silu_pre, a time row, no residual, no outer SiLU)");
    CTSI_CHECK_ARG(tbias_stride >= (film ? 2 * c : c), "ctsi_gn_apply_mod_f32: tbias_stride=%d shorter than the time row", tbias_stride);
    const long long vox = (long long)d * h * w;
    const bool v4 = (c % 4 == 0) && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const long long items = v4 ? vox * (c / 4) : vox * c;
    long long blocks = (items + 256 * 4 - 1) / (256 * 4);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    typedef void (*fn_t)(const float*, float*, const double*, const float*, const float*, int, long long, long long, int, float,
                         const float*, int, const int*, int);
    static const fn_t tab[4] = {gn_apply_mod_f32_kernel<false, false>, gn_apply_mod_f32_kernel<true, false>,
                                gn_apply_mod_f32_kernel<false, true>, gn_apply_mod_f32_kernel<true, true>};
    hipLaunchKernelGGL(tab[(film ? 1 : 0) | (v4 ? 2 : 0)], dim3((unsigned)blocks, n), dim3(256), (size_t)c * 3 * sizeof(float),
                       (hipStream_t)stream, x, y, sums, gamma, beta, c, vox, (long long)d_stat * h * w, groups, eps, tbias,
                       tbias_stride, step_ptr, n);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ==== backward ==========================================================================================================
// forward:  xhat = (x - mean) * rstd;  u = xhat * G + B  with the per-sample effective weight / bias
//             scale-shift: G = gamma * (1 + s), B = beta * (1 + s) + b;   additive: G = gamma, B = beta
//           y = drop( silu(u) [+ e] )
// backward: ga = dy * keep * inv;  gu = ga * silu'(u)
//           d_b = sum_vox gu;  d_s = gamma * sum gu*xhat + beta * sum gu;  d_e (additive) = sum_vox ga
//           dgamma = sum_n (1 + s) sum gu*xhat;  dbeta = sum_n (1 + s) sum gu
//           dx = rstd * (G*gu - mean_grp(G*gu) - xhat * mean_grp(G*gu*xhat))
// The three-pass shape of ctsi_gn_bwd: per-tile column sums (sum gu, sum gu*xhat, sum ga, sum xhat) -> per-(sample, group)
// terms and per-sample parameter partials -> dx.  Pass 3 re-derives gu from dy (no buffer for it exists), in fp32.
template <bool FILM>
__device__ __forceinline__ void gnm_bwd_coeffs(float* s_rs, float* s_mr, float* s_G, float* s_B, const double* sums,
                                               const float* gamma, const float* beta, const float* trow, int c, int groups,
                                               long long vox, float eps, int nb) {
    const int cpg = c / groups;
    const double cnt = (double)cpg * (double)vox;
    for (int ch = threadIdx.x; ch < c; ch += 256) {
        const int g = ch / cpg;
        const double m = sums[((long long)nb * groups + g) * 2 + 0] / cnt;
        double var = sums[((long long)nb * groups + g) * 2 + 1] / cnt - m * m;
        if (var < 0.0) var = 0.0;
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        s_rs[ch] = rstd;
        s_mr[ch] = -(float)m * rstd;
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

// Pass 1: grid (tiles, n), block 256.  colsum4 [n][tiles][4][c] = (sum gu, sum gu*xhat, sum ga, sum xhat).
template <bool FILM, bool DROP>
__global__ void __launch_bounds__(256)
gn_bwd_mod_reduce_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, const double* __restrict__ sums,
                         const float* __restrict__ gamma, const float* __restrict__ beta, int c, long long vox, int groups,
                         float eps, const float* __restrict__ tbias, int tbias_stride, float* __restrict__ colsum4, int tiles,
                         int tile_rows, uint32_t thr, float inv_keep, const unsigned long long* __restrict__ seed_ptr,
                         uint32_t layer_id) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_rs = reinterpret_cast<float*>(smem_raw);
    float* s_mr = s_rs + c;
    float* s_G = s_mr + c;
    float* s_B = s_G + c;
    float* s_red = s_B + c;                              // [rows_par][4][c]
    const int nb = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    gnm_bwd_coeffs<FILM>(s_rs, s_mr, s_G, s_B, sums, gamma, beta, tbias + (long long)nb * tbias_stride, c, groups, vox, eps, nb);
    __syncthreads();
    const unsigned long long seed = DROP ? *seed_ptr : 0ull;
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
        const bf16_t* db = dy + (long long)nb * vox * c + q * 8;
        float rs[8], mr[8], G[8], B[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            rs[k] = s_rs[q * 8 + k]; mr[k] = s_mr[q * 8 + k]; G[k] = s_G[q * 8 + k]; B[k] = s_B[q * 8 + k];
        }
        constexpr int U = 4;
        for (long long vb = v0 + rl; vb < v1; vb += (long long)rows_par * U) {
            uint4 xr[U], dr[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long v = vb + (long long)u * rows_par;
                if (v < v1) {
                    xr[u] = *reinterpret_cast<const uint4*>(xb + v * c);
                    dr[u] = *reinterpret_cast<const uint4*>(db + v * c);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long v = vb + (long long)u * rows_par;
                if (v >= v1) break;
                float xf[8], df[8];
                m_unpack8(xr[u], xf);
                m_unpack8(dr[u], df);
                uint32_t keep = 0xffu;
                if (DROP)
                    keep = ctsi_dropout_keep8(((unsigned long long)nb * (unsigned long long)vox + (unsigned long long)v) * cpr + q,
                                              layer_id, seed, thr);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float xh = xf[k] * rs[k] + mr[k];
                    const float uu = xh * G[k] + B[k];
                    float ga = df[k];
                    if (DROP) ga = (keep >> k) & 1u ? ga * inv_keep : 0.0f;
                    const float gu = ga * m_silu_grad_f(uu);
                    a0[k] += gu;
                    a1[k] += gu * xh;
                    a2[k] += ga;
                    a3[k] += xh;
                }
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
    float* out = colsum4 + ((long long)nb * tiles + tile) * 4 * c;
    for (int e = tid; e < 4 * c; e += 256) {
        float t = 0.0f;
        for (int r = 0; r < rows_par; ++r) t += s_red[r * 4 * c + e];
        out[e] = t;
    }
}

// Pass 2a: grid (groups, n), block 1024: one block owns one (sample, group).  Every (statistic, channel) item of the group is
// summed over the tiles by TL = 1024 / items lanes, each in a fixed strided order with eight loads in flight, and the lanes are
// combined in lane order (deterministic: no atomics, no dependence on block scheduling).  A large tensor has thousands of tiles
// and only groups x n blocks here, so the pass is latency-bound: with 256 threads and four loads in flight the backward took
// 65 us (201 MB tensor) and 98 us (101 MB tensor) longer (profiles/resblock_options_bench.log, last block).  Writes
//   s12[n][groups][2] = (sum_grp G*gu, sum_grp G*gu*xhat) / m
//   pgrad[n][4][c]    = (sum gu*xhat, sum gu, sum ga, sum_vox dx)      sum_vox dx = rstd * (G * sum gu - V*S1/m - S2/m * sum xhat)
#define GNM_FIN_THREADS 1024
template <bool FILM>
__global__ void __launch_bounds__(GNM_FIN_THREADS)
gn_bwd_mod_finalize_kernel(const float* __restrict__ colsum4, const float* __restrict__ gamma, const double* __restrict__ sums,
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
    const float* base = colsum4 + (long long)nb * tiles * 4 * c + c0;
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
    const double m = sums[((long long)nb * groups + g) * 2 + 0] / cnt;
    double var = sums[((long long)nb * groups + g) * 2 + 1] / cnt - m * m;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    for (int chl = tid; chl < cpg; chl += GNM_FIN_THREADS) {
        const int ch = c0 + chl;
        const float G = FILM ? gamma[ch] * (1.0f + trow[ch]) : gamma[ch];
        pgrad[((long long)nb * 4 + 0) * c + ch] = s_tot[1 * cpg + chl];
        pgrad[((long long)nb * 4 + 1) * c + ch] = s_tot[0 * cpg + chl];
        pgrad[((long long)nb * 4 + 2) * c + ch] = s_tot[2 * cpg + chl];
        pgrad[((long long)nb * 4 + 3) * c + ch] = rstd * (G * s_tot[0 * cpg + chl] - (float)vox * s_g[0] - s_g[1] * s_tot[3 * cpg + chl]);
    }
}

// Pass 2b: one thread per channel, samples in order.  scale-shift: dtb[n][ch] = d_s, dtb[n][c + ch] = d_b; additive: dtb[n][ch] = d_e.
template <bool FILM>
__global__ void __launch_bounds__(256)
gn_bwd_mod_param_kernel(const float* __restrict__ pgrad, int n, int c, const float* __restrict__ gamma,
                        const float* __restrict__ beta, const float* __restrict__ tbias, int tbias_stride,
                        float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dtb, long long dtb_stride,
                        float* __restrict__ dxsum) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= c) return;
    float a = 0.0f, b = 0.0f, d = 0.0f;
    const float ga = gamma[ch], be = beta[ch];
    for (int i = 0; i < n; ++i) {
        const float gx = pgrad[((long long)i * 4 + 0) * c + ch];     // sum gu * xhat
        const float g1 = pgrad[((long long)i * 4 + 1) * c + ch];     // sum gu
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

// Pass 3: dx = rstd * (G*gu - S1/m - xhat * S2/m), gu re-derived from dy.  grid (blocks, n), block 256; launch forms of
// gn_bwd_apply_kernel (train_ops.hip): the stride is a multiple of the row's chunk count, so a thread keeps its coefficients.
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
    gnm_bwd_coeffs<FILM>(s_rs, s_mr, s_G, s_B, sums, gamma, beta, tbias + (long long)nb * tbias_stride, c, groups, vox, eps, nb);
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
    const bf16_t* gb = dy + (long long)nb * vox * c;
    const bf16_t* xb = x + (long long)nb * vox * c;
    bf16_t* ob = dx + (long long)nb * vox * c;
    const long long stride = contig ? 256 : (long long)gridDim.x * 256;
    const long long e0 = (contig ? (long long)blockIdx.x * 512 : (long long)blockIdx.x * 256) + tid;
    const long long total_end = contig && (long long)(blockIdx.x + 1) * 512 < total ? (long long)(blockIdx.x + 1) * 512 : total;
    const int q = (int)(e0 % cpr);
    float rs[8], mr[8], G[8], B[8], b1[8], b2[8];
#pragma unroll
    for (int k = 0; k < 8; k += 4) {
        *reinterpret_cast<float4*>(rs + k) = *reinterpret_cast<const float4*>(s_rs + q * 8 + k);
        *reinterpret_cast<float4*>(mr + k) = *reinterpret_cast<const float4*>(s_mr + q * 8 + k);
        *reinterpret_cast<float4*>(G + k) = *reinterpret_cast<const float4*>(s_G + q * 8 + k);
        *reinterpret_cast<float4*>(B + k) = *reinterpret_cast<const float4*>(s_B + q * 8 + k);
        *reinterpret_cast<float4*>(b1 + k) = *reinterpret_cast<const float4*>(s_b1 + q * 8 + k);
        *reinterpret_cast<float4*>(b2 + k) = *reinterpret_cast<const float4*>(s_b2 + q * 8 + k);
    }
    auto one = [&](const uint4 graw, const uint4 xraw, long long e) {
        float gf[8], xf[8], of[8];
        m_unpack8(graw, gf);
        m_unpack8(xraw, xf);
        uint32_t keep = 0xffu;
        if (DROP) keep = ctsi_dropout_keep8(chunk0 + (unsigned long long)e, layer_id, seed, thr);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float xh = xf[k] * rs[k] + mr[k];
            float ga = gf[k];
            if (DROP) ga = (keep >> k) & 1u ? ga * inv_keep : 0.0f;
            const float gu = ga * m_silu_grad_f(xh * G[k] + B[k]);
            of[k] = rs[k] * (G[k] * gu) - b1[k] - xh * b2[k];
        }
        *reinterpret_cast<uint4*>(ob + e * 8) = m_pack8(of);
    };
    constexpr int U = 2;
    long long e = e0;
    for (; e + (U - 1) * stride < total_end; e += U * stride) {
        uint4 gr[U], xr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            gr[u] = *reinterpret_cast<const uint4*>(gb + (e + u * stride) * 8);
            xr[u] = *reinterpret_cast<const uint4*>(xb + (e + u * stride) * 8);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) one(gr[u], xr[u], e + u * stride);
    }
    for (; e < total_end; e += stride)
        one(*reinterpret_cast<const uint4*>(gb + e * 8), *reinterpret_cast<const uint4*>(xb + e * 8), e);
}

// rows per statistics tile: the rule of ctsi_gn_bwd (train_ops.hip gnb_tile_rows)
static int gnm_tile_rows(int n, int c, long long vox) {
    const int rows_par = 256 / (c >> 3);
    const int min_rows = rows_par * 4 > 16 ? rows_par * 4 : 16;
    int rows = GNM_TILE_ROWS;
    while (rows > min_rows && (long long)n * ((vox + rows - 1) / rows) < 2048) rows >>= 1;
    return rows;
}

extern "C" size_t ctsi_gn_bwd_mod_workspace_floats(int n, int c, int d, int h, int w, int groups) {
    if (n <= 0 || c < 8 || c % 8 != 0 || c > 2048 || groups <= 0) return 0;
    const long long vox = (long long)d * h * w;
    const int tile_rows = gnm_tile_rows(n, c, vox);
    const long long tiles = (vox + tile_rows - 1) / tile_rows;
    return (size_t)((long long)n * tiles * 4 * c + (long long)n * groups * 2 + (long long)n * 4 * c);
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
    const int tile_rows = gnm_tile_rows(n, c, vox);
    const int tiles = (int)((vox + tile_rows - 1) / tile_rows);
    hipStream_t st = (hipStream_t)stream;
    float* colsum4 = workspace;
    float* s12 = colsum4 + (long long)n * tiles * 4 * c;
    float* pgrad = s12 + (long long)n * groups * 2;
    const int cpr = c >> 3;
    const int rows_par = 256 / cpr;
    const size_t lds1 = (size_t)(4 * c + rows_par * 4 * c) * sizeof(float);
    CTSI_CHECK_ARG(lds1 <= 160 * 1024, "ctsi_gn_bwd_mod: LDS budget exceeded for c=%d", c);
    const bool drop = p_thr16 > 0;
    const uint32_t thr = (uint32_t)p_thr16, lid = (uint32_t)layer_id;
    const unsigned long long* sp = (const unsigned long long*)seed;
    const int vi = (film ? 1 : 0) | (drop ? 2 : 0);
    {
        typedef void (*fn_t)(const bf16_t*, const bf16_t*, const double*, const float*, const float*, int, long long, int, float,
                             const float*, int, float*, int, int, uint32_t, float, const unsigned long long*, uint32_t);
        static const fn_t tab[4] = {gn_bwd_mod_reduce_kernel<false, false>, gn_bwd_mod_reduce_kernel<true, false>,
                                    gn_bwd_mod_reduce_kernel<false, true>, gn_bwd_mod_reduce_kernel<true, true>};
        if (lds1 > 64 * 1024)
            CTSI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(tab[vi]), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds1));
        hipLaunchKernelGGL(tab[vi], dim3(tiles, n), dim3(256), lds1, st, (const bf16_t*)x, (const bf16_t*)dy, sums, gamma, beta,
                           c, vox, groups, eps, tbias, tbias_stride, colsum4, tiles, tile_rows, thr, inv_keep, sp, lid);
        CTSI_LAUNCH_CHECK();
    }
    {
        const int cpg = c / groups;
        const int items = 4 * cpg;
        const int TL = items >= GNM_FIN_THREADS ? 1 : GNM_FIN_THREADS / items;
        const size_t lds2 = (size_t)(TL * items + items + 2) * sizeof(float);
        CTSI_CHECK_ARG(lds2 <= 64 * 1024, "ctsi_gn_bwd_mod: c / groups = %d channels per group exceed the finalize pass's LDS", cpg);
        if (film)
            hipLaunchKernelGGL(gn_bwd_mod_finalize_kernel<true>, dim3(groups, n), dim3(GNM_FIN_THREADS), lds2, st, colsum4, gamma, sums, eps,
                               c, vox, groups, tiles, tbias, tbias_stride, s12, pgrad);
        else
            hipLaunchKernelGGL(gn_bwd_mod_finalize_kernel<false>, dim3(groups, n), dim3(GNM_FIN_THREADS), lds2, st, colsum4, gamma, sums, eps,
                               c, vox, groups, tiles, tbias, tbias_stride, s12, pgrad);
        CTSI_LAUNCH_CHECK();
    }
    if (film)
        hipLaunchKernelGGL(gn_bwd_mod_param_kernel<true>, dim3((c + 255) / 256), dim3(256), 0, st, pgrad, n, c, gamma, beta, tbias,
                           tbias_stride, dgamma, dbeta, dtbias, dtbias_stride, dxsum);
    else
        hipLaunchKernelGGL(gn_bwd_mod_param_kernel<false>, dim3((c + 255) / 256), dim3(256), 0, st, pgrad, n, c, gamma, beta, tbias,
                           tbias_stride, dgamma, dbeta, dtbias, dtbias_stride, dxsum);
    CTSI_LAUNCH_CHECK();
    const long long total = vox * cpr;
    long long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    int contig = 0;
    if (256 % cpr == 0) {
        contig = 1;
        blocks = (total + 511) / 512;
    } else {
        int gq = cpr, g256 = 256;
        while (g256) { const int t = gq % g256; gq = g256; g256 = t; }
        const int need = cpr / gq;
        blocks = (blocks + need - 1) / need * need;
    }
    {
        typedef void (*fn_t)(const bf16_t*, const bf16_t*, const double*, const float*, const float*, const float*, bf16_t*, int,
                             long long, int, float, int, const float*, int, uint32_t, float, const unsigned long long*, uint32_t);
        static const fn_t tab[4] = {gn_bwd_mod_apply_kernel<false, false>, gn_bwd_mod_apply_kernel<true, false>,
                                    gn_bwd_mod_apply_kernel<false, true>, gn_bwd_mod_apply_kernel<true, true>};
        hipLaunchKernelGGL(tab[vi], dim3((unsigned)blocks, n), dim3(256), 6 * c * sizeof(float), st, (const bf16_t*)dy,
                           (const bf16_t*)x, sums, gamma, beta, s12, (bf16_t*)dx, c, vox, groups, eps, contig, tbias,
                           tbias_stride, thr, inv_keep, sp, lid);
        CTSI_LAUNCH_CHECK();
    }
    return CTSI_OK;
}

// ---- windows for tests ---------------------------------------------------------------------------------------------------
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
