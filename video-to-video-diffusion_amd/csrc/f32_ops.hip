// fp32 inference mode: the element-wise passes between the convolutions (conv_f32.hip), on fp32 NDHWC activations.
//   GroupNorm column sums and apply (+SiLU, +time bias, +residual, +SiLU)   models/unet3d.py:59-74,116-133; models/vae.py:28-56
//   TemporalAttention fast mode: depth sums, normalised depth sum, broadcast add (attention.hip has the derivation)
// Statistics keep the engine's two-stage form: per-tile fp32 column sums -> ctsi_gn_finalize (fp64, fixed order) -> apply.
// Every reduction has a fixed order and no atomics: a relaunch is bit-identical.  Transcendentals are the accurate libm
// forms (expf, tanhf), not the 1-ulp hardware approximations the bf16 path rounds away.
#include "ctsi_internal.h"
#include "gn_frame.h"

#define F32_GN_TILE_ROWS 512
#define F32_ATTN_TILE_POS 64

__device__ __forceinline__ float silu_acc(float x) { return x / (1.0f + expf(-x)); }

// ---- GroupNorm column sums: grid (tiles, n, ceil(c / 64)); block = 64 columns x 4 row groups -----------------------------
__global__ void __launch_bounds__(256)
gn_colsum_f32_kernel(const float* __restrict__ x, float* __restrict__ colsum, int n_total, int c, long long vox, int tps) {
    __shared__ float red[4][64][2];
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int col = blockIdx.z * 64 + cl;
    const int tile = blockIdx.x, nb = blockIdx.y;
    const long long v0 = (long long)tile * F32_GN_TILE_ROWS;
    const long long v1 = v0 + F32_GN_TILE_ROWS < vox ? v0 + F32_GN_TILE_ROWS : vox;
    float s1 = 0.0f, s2 = 0.0f;
    if (col < c) {
        const float* base = x + (long long)nb * vox * c + col;
        for (long long v = v0 + rg; v < v1; v += 4) {
            const float f = base[v * c];
            s1 += f;
            s2 += f * f;
        }
    }
    red[rg][cl][0] = s1;
    red[rg][cl][1] = s2;
    __syncthreads();
    if (rg == 0 && col < c) {
        const float t1 = ((red[0][cl][0] + red[1][cl][0]) + red[2][cl][0]) + red[3][cl][0];
        const float t2 = ((red[0][cl][1] + red[1][cl][1]) + red[2][cl][1]) + red[3][cl][1];
        const long long tg = (long long)nb * tps + tile;
        const long long slab = (long long)n_total * tps * c;
        colsum[tg * c + col] = t1;
        colsum[slab + tg * c + col] = t2;
    }
}

extern "C" int ctsi_gn_colsum_f32_tiles(int d, int h, int w) {
    const long long vox = (long long)d * h * w;
    return (int)((vox + F32_GN_TILE_ROWS - 1) / F32_GN_TILE_ROWS);
}

extern "C" int ctsi_gn_colsum_f32(const float* x, float* colsum, int n, int c, int d, int h, int w, int* tiles_per_sample,
                                  void* stream) {
    CTSI_CHECK_ARG(x && colsum, "ctsi_gn_colsum_f32: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_gn_colsum_f32: sizes must be positive");
    const int tps = ctsi_gn_colsum_f32_tiles(d, h, w);
    if (tiles_per_sample) *tiles_per_sample = tps;
    hipLaunchKernelGGL(gn_colsum_f32_kernel, dim3(tps, n, (c + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, colsum, n, c,
                       (long long)d * h * w, tps);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- GroupNorm apply: y = [silu](gn(x)) [+ tbias] [+ residual] [silu] ------------------------------------------------------
// grid (blocks, n); block 256.  Scale / shift / time bias of every channel in LDS; 4 channels per thread when c % 4 == 0.
// FILM (the ResBlock's scale-shift option; inference, so no dropout): with SILU_PRE and a time row (s | b) of
// 2c values, y = silu(gn(x) * (1 + s) + b) -- the prologue's coefficients change, nothing is added afterwards.
template <bool SILU_PRE, bool TB, bool RES, bool SILU_POST, bool FILM, bool V4>
__global__ void __launch_bounds__(256)
gn_apply_f32_kernel(const float* __restrict__ x, float* __restrict__ y, const double* __restrict__ sums,
                    const float* __restrict__ gamma, const float* __restrict__ beta, int c, long long vox, long long vox_stat,
                    int groups, float eps, const float* __restrict__ tbias, int tbias_stride, const int* __restrict__ step_ptr,
                    int n_total, const float* __restrict__ residual) {
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
        const double m = st.mean, rstd = st.rstd;
        if (FILM) {      // the shift as mean * (gamma * rstd): the one form the engine emits, kept to the bit
            const double sc = (double)gamma[ch] * rstd, sh = (double)beta[ch] - m * sc;
            const double s1 = 1.0 + (double)tbias[trow * tbias_stride + ch];
            s_scale[ch] = (float)(sc * s1);
            s_shift[ch] = (float)(sh * s1 + (double)tbias[trow * tbias_stride + c + ch]);
        } else {
            s_scale[ch] = (float)((double)gamma[ch] * rstd);
            s_shift[ch] = (float)((double)beta[ch] - m * (double)gamma[ch] * rstd);
            if (TB) s_tb[ch] = tbias[trow * tbias_stride + ch];
        }
    }
    __syncthreads();
    const float* xb = x + (long long)nb * vox * c;
    float* yb = y + (long long)nb * vox * c;
    const float* rb = RES ? residual + (long long)nb * vox * c : nullptr;
    auto one = [&](float v, int ch, float r) {
        v = v * s_scale[ch] + s_shift[ch];
        if (SILU_PRE) v = silu_acc(v);
        if (ADD_TB) v += s_tb[ch];
        if (RES) v += r;
        if (SILU_POST) v = silu_acc(v);
        return v;
    };
    const long long stride = (long long)gridDim.x * 256;
    if (V4) {
        const int c4 = c >> 2;
        const long long total = vox * c4;
        for (long long e = (long long)blockIdx.x * 256 + tid; e < total; e += stride) {
            const int ch = (int)(e % c4) * 4;
            const float4 xv = reinterpret_cast<const float4*>(xb)[e];
            const float4 rv = RES ? reinterpret_cast<const float4*>(rb)[e] : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 o;
            o.x = one(xv.x, ch, rv.x);
            o.y = one(xv.y, ch + 1, rv.y);
            o.z = one(xv.z, ch + 2, rv.z);
            o.w = one(xv.w, ch + 3, rv.w);
            reinterpret_cast<float4*>(yb)[e] = o;
        }
    } else {
        const long long total = vox * c;
        for (long long e = (long long)blockIdx.x * 256 + tid; e < total; e += stride)
            yb[e] = one(xb[e], (int)(e % c), RES ? rb[e] : 0.0f);
    }
}

typedef void (*gn_apply_f32_fn)(const float*, float*, const double*, const float*, const float*, int, long long, long long,
                                int, float, const float*, int, const int*, int, const float*);
template <int I>
static gn_apply_f32_fn gn_apply_f32_pick(int idx) {
    if constexpr (I >= 32) {
        return nullptr;
    } else {
        if (idx == I)
            return gn_apply_f32_kernel<(I & 1) != 0, (I & 2) != 0, (I & 4) != 0, (I & 8) != 0, false, (I & 16) != 0>;
        return gn_apply_f32_pick<I + 1>(idx);
    }
}

static int gn_apply_f32_launch(const float* x, float* y, const double* sums, const float* gamma, const float* beta, int n, int c,
                               int d, int h, int w, int d_stat, int groups, float eps, int silu_pre, const float* tbias,
                               int tbias_stride, const int* step_ptr, const float* residual, int silu_post, int film,
                               void* stream) {
    const long long vox = (long long)d * h * w;
    const bool v4 = (c % 4 == 0) && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)residual) & 15) == 0;
    const long long items = v4 ? vox * (c / 4) : vox * c;
    long long blocks = (items + 256 * 4 - 1) / (256 * 4);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    const int idx = (silu_pre ? 1 : 0) | (tbias ? 2 : 0) | (residual ? 4 : 0) | (silu_post ? 8 : 0) | (v4 ? 16 : 0);
    gn_apply_f32_fn fn = gn_apply_f32_pick<0>(idx);
    if (film) fn = v4 ? gn_apply_f32_kernel<true, true, false, false, true, true> : gn_apply_f32_kernel<true, true, false, false, true, false>;
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks, n), dim3(256), (size_t)c * 3 * sizeof(float), (hipStream_t)stream, x, y, sums,
                       gamma, beta, c, vox, (long long)d_stat * h * w, groups, eps, tbias, tbias_stride, step_ptr, n, residual);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_gn_apply_f32(const float* x, float* y, const double* sums, const float* gamma, const float* beta, int n,
                                 int c, int d, int h, int w, int d_stat, int groups, float eps, int silu_pre, const float* tbias,
                                 int tbias_stride, const int* step_ptr, const float* residual, int silu_post, void* stream) {
    CTSI_CHECK_ARG(x && y && sums && gamma && beta, "ctsi_gn_apply_f32: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && c <= 4096 && d > 0 && h > 0 && w > 0, "ctsi_gn_apply_f32: bad sizes (c=%d)", c);
    CTSI_CHECK_ARG(groups > 0 && c % groups == 0, "ctsi_gn_apply_f32: c=%d not divisible by groups=%d", c, groups);
    CTSI_CHECK_ARG(d_stat >= d, "ctsi_gn_apply_f32: d_stat=%d < d=%d", d_stat, d);
    return gn_apply_f32_launch(x, y, sums, gamma, beta, n, c, d, h, w, d_stat, groups, eps, silu_pre, tbias, tbias_stride, step_ptr,
                               residual, silu_post, 0, stream);
}

// The ResBlock's middle pass (silu_pre, a time row, no residual, no outer SiLU); film = 0 is ctsi_gn_apply_f32's own form.
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
    return gn_apply_f32_launch(x, y, sums, gamma, beta, n, c, d, h, w, d_stat, groups, eps, 1, tbias, tbias_stride, step_ptr,
                               nullptr, 0, film, stream);
}

// ---- TemporalAttention, fast mode --------------------------------------------------------------------------------------
// pass 1: S[n][pos][c] = sum_d x, and GroupNorm column sums of x per tile of 64 positions.
// grid (tiles, n, ceil(c / 64)); block = 64 channels x 4 position groups.
__global__ void __launch_bounds__(256)
attn_depthsum_f32_kernel(const float* __restrict__ x, float* __restrict__ depthsum, float* __restrict__ colsum, int n_total,
                         int c, int d, int hw, int tps) {
    __shared__ float red[4][64][2];
    const int cl = threadIdx.x & 63, pg = threadIdx.x >> 6;
    const int col = blockIdx.z * 64 + cl;
    const int tile = blockIdx.x, nb = blockIdx.y;
    float c1 = 0.0f, c2 = 0.0f;
    if (col < c) {
        for (int pos = tile * F32_ATTN_TILE_POS + pg; pos < hw && pos < (tile + 1) * F32_ATTN_TILE_POS; pos += 4) {
            const float* base = x + ((long long)nb * d * hw + pos) * c + col;
            float s = 0.0f;
            for (int dd = 0; dd < d; ++dd) {
                const float f = base[(long long)dd * hw * c];
                s += f;
                c2 += f * f;
            }
            depthsum[((long long)nb * hw + pos) * c + col] = s;
            c1 += s;
        }
    }
    red[pg][cl][0] = c1;
    red[pg][cl][1] = c2;
    __syncthreads();
    if (pg == 0 && col < c) {
        const float t1 = ((red[0][cl][0] + red[1][cl][0]) + red[2][cl][0]) + red[3][cl][0];
        const float t2 = ((red[0][cl][1] + red[1][cl][1]) + red[2][cl][1]) + red[3][cl][1];
        const long long tg = (long long)nb * tps + tile;
        const long long slab = (long long)n_total * tps * c;
        colsum[tg * c + col] = t1;
        colsum[slab + tg * c + col] = t2;
    }
}

extern "C" int ctsi_attn_depthsum_f32_tiles(int h, int w) {
    return (h * w + F32_ATTN_TILE_POS - 1) / F32_ATTN_TILE_POS;
}

extern "C" int ctsi_attn_depthsum_f32(const float* x, float* depthsum, float* colsum, int n, int c, int d, int h, int w,
                                      void* stream) {
    CTSI_CHECK_ARG(x && depthsum && colsum, "ctsi_attn_depthsum_f32: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_attn_depthsum_f32: sizes must be positive");
    const int tps = ctsi_attn_depthsum_f32_tiles(h, w);
    hipLaunchKernelGGL(attn_depthsum_f32_kernel, dim3(tps, n, (c + 63) / 64), dim3(256), 0, (hipStream_t)stream, x, depthsum,
                       colsum, n, c, d, h * w, tps);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// pass 2: xs[n][pos][ch] = gamma rstd (S - D mean) + D beta   (fp32 out)
__global__ void __launch_bounds__(256)
attn_normsum_f32_kernel(const float* __restrict__ depthsum, const double* __restrict__ sums, const float* __restrict__ gamma,
                        const float* __restrict__ beta, float* __restrict__ out, int c, int d, long long hw, int groups,
                        float eps, long long total) {
    const int cpg = c / groups;
    const double cnt = (double)cpg * (double)d * (double)hw;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int ch = (int)(e % c);
        const long long nb = e / (hw * c);
        const int g = ch / cpg;
        const double m = sums[(nb * groups + g) * 2 + 0] / cnt;
        double var = sums[(nb * groups + g) * 2 + 1] / cnt - m * m;
        if (var < 0.0) var = 0.0;
        const double rstd = 1.0 / sqrt(var + (double)eps);
        out[e] = (float)((double)gamma[ch] * rstd * ((double)depthsum[e] - (double)d * m) + (double)d * (double)beta[ch]);
    }
}

extern "C" int ctsi_attn_normsum_f32(const float* depthsum, const double* sums, const float* gamma, const float* beta,
                                     float* out, int n, int c, int d, int h, int w, int groups, float eps, void* stream) {
    CTSI_CHECK_ARG(depthsum && sums && gamma && beta && out, "ctsi_attn_normsum_f32: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && groups > 0 && c % groups == 0, "ctsi_attn_normsum_f32: bad c=%d groups=%d", c, groups);
    const long long total = (long long)n * h * w * c;
    long long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(attn_normsum_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, depthsum, sums,
                       gamma, beta, out, c, d, (long long)h * w, groups, eps, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// pass 3: y[n][d][pos][ch] = x + p[n][pos][ch]; grid (blocks, n * d)
__global__ void __launch_bounds__(256)
attn_broadcast_add_f32_kernel(const float* __restrict__ x, const float* __restrict__ pterm, float* __restrict__ y, int d,
                              long long slice) {
    const int sl = blockIdx.y, nb = sl / d;
    const float* xs = x + (long long)sl * slice;
    float* ys = y + (long long)sl * slice;
    const float* ps = pterm + (long long)nb * slice;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < slice; e += (long long)gridDim.x * 256)
        ys[e] = xs[e] + ps[e];
}

extern "C" int ctsi_attn_broadcast_add_f32(const float* x, const float* p, float* y, int n, int c, int d, int h, int w,
                                           void* stream) {
    CTSI_CHECK_ARG(x && p && y, "ctsi_attn_broadcast_add_f32: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0 && (long long)n * d < 65536,
                   "ctsi_attn_broadcast_add_f32: bad sizes");
    const long long slice = (long long)h * w * c;
    long long blocks = (slice + 1023) / 1024;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(attn_broadcast_add_f32_kernel, dim3((unsigned)blocks, n * d), dim3(256), 0, (hipStream_t)stream, x, p,
                       y, d, slice);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
