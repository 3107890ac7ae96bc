// DPM-Solver++(2M) update (Lu et al. 2022, multistep, data prediction) for the captured sampler step, and the EDM
// Heun / Euler update (ctsi_heun_step, below).
// One pass over the latent per step: it reads z_i, eps_i, the previous data prediction x0_{i-1} and the coefficient row
// at *step_ptr, and writes z_{i+1}, x0_i (over x0_{i-1}) and the z slice of the U-Net input.  HBM-bound: 16-byte fp32
// accesses when the channel count allows.
#include "ctsi_internal.h"

// coef row layout (8 floats, float64 on the host, rounded once to fp32; sampler.dpm_coef_rows):
//   [0] = 1/alpha_i   [1] = sigma_i/alpha_i   [2] = a_i   [3] = b_i   [4] = c_i   [5..7] unused
//   x0_i    = clamp(nan_to_num(z_i/alpha_i - (sigma_i/alpha_i) eps_i), -10, 10)
//   z_{i+1} = a_i z_i + b_i x0_i + c_i x0_{i-1}
// c_i = 0 on the first step of a volume and at first order, but x0_prev is only ever read as a finite value: the
// buffer is allocated zeroed and only the sanitised, clamped x0 is stored, so 0 * x0_prev is exactly 0.
// nonfinite: as ctsi_ddim_step -- row *step_ptr counts {eps NaN, Inf, x0 NaN, Inf, z after update NaN, Inf}.
namespace {

__device__ __forceinline__ void count_nf(float v, int& n_nan, int& n_inf) {
    n_nan += (v != v) ? 1 : 0;
    n_inf += (v == __builtin_inff() || v == -__builtin_inff()) ? 1 : 0;
}

__device__ __forceinline__ float dpm_elem(float zt, float ep, float xp, float c0, float c1, float ca, float cb, float cc,
                                          float& x0_out, int* cnt) {
    count_nf(ep, cnt[0], cnt[1]);
    ep = nan_to_num_f(ep);
    float x0 = fmaf(-c1, ep, c0 * zt);
    count_nf(x0, cnt[2], cnt[3]);
    x0 = fminf(fmaxf(nan_to_num_f(x0), -10.0f), 10.0f);
    float zn = fmaf(cc, xp, fmaf(cb, x0, ca * zt));
    count_nf(zn, cnt[4], cnt[5]);
    x0_out = x0;
    return nan_to_num_f(zn);
}

__device__ __forceinline__ void store4(bf16_t* p, const float* v) {
    uint2 pk;
    pk.x = pack_bf16x2(v[0], v[1]);
    pk.y = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<uint2*>(p) = pk;
}
__device__ __forceinline__ void store4(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store1(bf16_t* p, float v) { *p = f32_to_bf16(v); }
__device__ __forceinline__ void store1(float* p, float v) { *p = v; }

__device__ __forceinline__ void flush_counts(const int* cnt, int* nonfinite, int step) {
    if (nonfinite == nullptr) return;
    const int any = cnt[0] | cnt[1] | cnt[2] | cnt[3] | cnt[4] | cnt[5];
    if (__any(any != 0)) {   // never taken on healthy runs
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (cnt[k]) atomicAdd(&nonfinite[step * 6 + k], cnt[k]);
    }
}

// 4 consecutive channels of one voxel per thread and iteration (c % 4 == 0, 16-byte aligned fp32 tensors)
template <typename ZT>
__global__ void __launch_bounds__(256)
dpm_step_vec4_kernel(float* __restrict__ z, const float* __restrict__ eps, float* __restrict__ x0_prev,
                     ZT* __restrict__ zin, int c_total, int c_off, const float* __restrict__ coef,
                     const int* __restrict__ step_ptr, int c, long long total4, int* __restrict__ nonfinite) {
    const int step = step_ptr ? *step_ptr : 0;
    const float* cf = coef + (long long)step * 8;
    const float c0 = cf[0], c1 = cf[1], ca = cf[2], cb = cf[3], cc = cf[4];
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total4; q += (long long)gridDim.x * 256) {
        const long long e = q * 4;
        const float4 zt = reinterpret_cast<const float4*>(z)[q];
        const float4 ep = reinterpret_cast<const float4*>(eps)[q];
        const float4 xp = reinterpret_cast<const float4*>(x0_prev)[q];
        float zn[4], x0[4];
        zn[0] = dpm_elem(zt.x, ep.x, xp.x, c0, c1, ca, cb, cc, x0[0], cnt);
        zn[1] = dpm_elem(zt.y, ep.y, xp.y, c0, c1, ca, cb, cc, x0[1], cnt);
        zn[2] = dpm_elem(zt.z, ep.z, xp.z, c0, c1, ca, cb, cc, x0[2], cnt);
        zn[3] = dpm_elem(zt.w, ep.w, xp.w, c0, c1, ca, cb, cc, x0[3], cnt);
        reinterpret_cast<float4*>(z)[q] = make_float4(zn[0], zn[1], zn[2], zn[3]);
        reinterpret_cast<float4*>(x0_prev)[q] = make_float4(x0[0], x0[1], x0[2], x0[3]);
        if (zin) {
            const long long nv = e / c;
            const int ch = (int)(e - nv * c);
            store4(zin + nv * c_total + c_off + ch, zn);
        }
    }
    flush_counts(cnt, nonfinite, step);
}

// any channel count / alignment: one element per thread and iteration
template <typename ZT>
__global__ void __launch_bounds__(256)
dpm_step_scalar_kernel(float* __restrict__ z, const float* __restrict__ eps, float* __restrict__ x0_prev,
                       ZT* __restrict__ zin, int c_total, int c_off, const float* __restrict__ coef,
                       const int* __restrict__ step_ptr, int c, long long total, int* __restrict__ nonfinite) {
    const int step = step_ptr ? *step_ptr : 0;
    const float* cf = coef + (long long)step * 8;
    const float c0 = cf[0], c1 = cf[1], ca = cf[2], cb = cf[3], cc = cf[4];
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        float x0;
        const float zn = dpm_elem(z[e], eps[e], x0_prev[e], c0, c1, ca, cb, cc, x0, cnt);
        z[e] = zn;
        x0_prev[e] = x0;
        if (zin) {
            const long long nv = e / c;
            const int ch = (int)(e - nv * c);
            store1(zin + nv * c_total + c_off + ch, zn);
        }
    }
    flush_counts(cnt, nonfinite, step);
}

inline bool aligned(const void* p, unsigned bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

template <typename ZT>
int dpm_step(float* z, const float* eps, float* x0_prev, ZT* zin, int c_total, int c_off, const float* coef,
             const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite, void* stream) {
    CTSI_CHECK_ARG(z && eps && x0_prev && coef, "ctsi_dpm_step: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_dpm_step: bad shape n=%d c=%d d=%d h=%d w=%d", n, c,
                   d, h, w);
    CTSI_CHECK_ARG(!zin || (c_off >= 0 && c_off + c <= c_total), "ctsi_dpm_step: bad channel slice");
    const long long total = (long long)n * c * d * h * w;
    const bool vec = (c % 4) == 0 && aligned(z, 16) && aligned(eps, 16) && aligned(x0_prev, 16) &&
                     (!zin || ((c_total | c_off) % 4 == 0 && aligned(zin, 4 * sizeof(ZT))));
    const long long work = vec ? total / 4 : total;
    // one item per thread (the grid-stride loop only serves huge latents); at the config-2 latent this measured the same
    // 33 us as the DDIM kernel's 4096-block cap
    long long blocks = (work + 255) / 256;
    if (blocks > (1ll << 20)) blocks = 1ll << 20;
    if (vec)
        hipLaunchKernelGGL((dpm_step_vec4_kernel<ZT>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z,
                           eps, x0_prev, zin, c_total, c_off, coef, step_ptr, c, work, nonfinite);
    else
        hipLaunchKernelGGL((dpm_step_scalar_kernel<ZT>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z,
                           eps, x0_prev, zin, c_total, c_off, coef, step_ptr, c, work, nonfinite);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- EDM Heun / Euler update (Karras et al. 2022, Algorithm 2) ------------------------------------------------------
// One pass per U-Net evaluation.  The state is the VP latent zhat = xhat / a(sigma_hat) (a(s) = sqrt(1 + s^2)), so every
// buffer stays O(1); the a(sigma) factors live in the coefficients (sampler.heun_coef_rows, float64 rounded once).
// coef row layout (8 floats):
//   [0] c0  [1] c1  [2] c2  [3] kind (0 = predictor, 1 = closing)  [4] c4  [5] c5  [6] c6  [7] c7
//   D = clamp(nan_to_num(c0 zhat + c1 D1 - c2 eps), -10, 10)              (the denoiser's data prediction)
//   predictor:  D1 <- D,  zin <- c4 zhat + c5 D                           (z keeps zhat; zin = the corrector's input)
//   closing:    z  <- c4 zhat + c5 D + c6 D1 + c7 noise,  zin <- z       (corrector, Euler step or final row; c7 folds
//                                                                          the NEXT step's churn in, noise fp32 NCDHW)
// D1 is read only when c1 or c6 is non-zero (a corrector row right after its predictor), noise only when c7 is.  D1 is
// allocated zeroed and only ever receives the clamped, finite D.
// nonfinite: row *step_ptr counts {eps NaN, Inf, D NaN, Inf, value written (zin / z) NaN, Inf}, as ctsi_dpm_step.
struct HeunCoef {
    float c0, c1, c2, c4, c5, c6, c7;
    bool closing, use_d1, use_noise;
};

__device__ __forceinline__ HeunCoef heun_coef(const float* cf, const float* noise) {
    HeunCoef k;
    k.c0 = cf[0], k.c1 = cf[1], k.c2 = cf[2], k.c4 = cf[4], k.c5 = cf[5], k.c6 = cf[6], k.c7 = cf[7];
    k.closing = cf[3] != 0.0f;
    k.use_d1 = k.c1 != 0.0f || k.c6 != 0.0f;
    k.use_noise = k.closing && noise != nullptr && k.c7 != 0.0f;
    return k;
}

// returns the value to store (zin for a predictor row, z for a closing row); D in d_out
__device__ __forceinline__ float heun_elem(float zt, float ep, float h, float nz, const HeunCoef& k, float& d_out,
                                           int* cnt) {
    count_nf(ep, cnt[0], cnt[1]);
    ep = nan_to_num_f(ep);
    float dd = fmaf(-k.c2, ep, fmaf(k.c1, h, k.c0 * zt));
    count_nf(dd, cnt[2], cnt[3]);
    dd = fminf(fmaxf(nan_to_num_f(dd), -10.0f), 10.0f);
    float v = fmaf(k.c5, dd, k.c4 * zt);
    if (k.closing) v = fmaf(k.c7, nz, fmaf(k.c6, h, v));
    count_nf(v, cnt[4], cnt[5]);
    d_out = dd;
    return nan_to_num_f(v);
}

// 4 consecutive channels of one voxel per thread and iteration (c % 4 == 0, 16-byte aligned fp32 tensors)
template <typename ZT>
__global__ void __launch_bounds__(256)
heun_step_vec4_kernel(float* __restrict__ z, const float* __restrict__ eps, float* __restrict__ d1,
                      const float* __restrict__ noise, ZT* __restrict__ zin, int c_total, int c_off,
                      const float* __restrict__ coef, const int* __restrict__ step_ptr, int c, long long vox,
                      long long total4, int* __restrict__ nonfinite) {
    const int step = step_ptr ? *step_ptr : 0;
    const HeunCoef k = heun_coef(coef + (long long)step * 8, noise);
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total4; q += (long long)gridDim.x * 256) {
        const long long e = q * 4;
        const long long nv = e / c;
        const int ch = (int)(e - nv * c);
        const float4 zt = reinterpret_cast<const float4*>(z)[q];
        const float4 ep = reinterpret_cast<const float4*>(eps)[q];
        const float4 h = k.use_d1 ? reinterpret_cast<const float4*>(d1)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (k.use_noise) {     // NCDHW: the 4 channels are vox apart (coalesced across the wave's voxels)
            const long long nb = nv / vox, v = nv - nb * vox;
            const float* np = noise + (nb * c + ch) * vox + v;
#pragma unroll
            for (int j = 0; j < 4; ++j) nz[j] = np[j * vox];
        }
        float out[4], dd[4];
        out[0] = heun_elem(zt.x, ep.x, h.x, nz[0], k, dd[0], cnt);
        out[1] = heun_elem(zt.y, ep.y, h.y, nz[1], k, dd[1], cnt);
        out[2] = heun_elem(zt.z, ep.z, h.z, nz[2], k, dd[2], cnt);
        out[3] = heun_elem(zt.w, ep.w, h.w, nz[3], k, dd[3], cnt);
        if (k.closing)
            reinterpret_cast<float4*>(z)[q] = make_float4(out[0], out[1], out[2], out[3]);
        else
            reinterpret_cast<float4*>(d1)[q] = make_float4(dd[0], dd[1], dd[2], dd[3]);
        store4(zin + nv * c_total + c_off + ch, out);
    }
    flush_counts(cnt, nonfinite, step);
}

// any channel count / alignment: one element per thread and iteration
template <typename ZT>
__global__ void __launch_bounds__(256)
heun_step_scalar_kernel(float* __restrict__ z, const float* __restrict__ eps, float* __restrict__ d1,
                        const float* __restrict__ noise, ZT* __restrict__ zin, int c_total, int c_off,
                        const float* __restrict__ coef, const int* __restrict__ step_ptr, int c, long long vox,
                        long long total, int* __restrict__ nonfinite) {
    const int step = step_ptr ? *step_ptr : 0;
    const HeunCoef k = heun_coef(coef + (long long)step * 8, noise);
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long nv = e / c;
        const int ch = (int)(e - nv * c);
        const float h = k.use_d1 ? d1[e] : 0.0f;
        float nz = 0.0f;
        if (k.use_noise) {
            const long long nb = nv / vox, v = nv - nb * vox;
            nz = noise[(nb * c + ch) * vox + v];
        }
        float dd;
        const float out = heun_elem(z[e], eps[e], h, nz, k, dd, cnt);
        if (k.closing)
            z[e] = out;
        else
            d1[e] = dd;
        store1(zin + nv * c_total + c_off + ch, out);
    }
    flush_counts(cnt, nonfinite, step);
}

template <typename ZT>
int heun_step(float* z, const float* eps, float* d1, const float* noise, ZT* zin, int c_total, int c_off,
              const float* coef, const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite, void* stream) {
    CTSI_CHECK_ARG(z && eps && d1 && zin && coef, "ctsi_heun_step: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_heun_step: bad shape n=%d c=%d d=%d h=%d w=%d", n,
                   c, d, h, w);
    CTSI_CHECK_ARG(c_off >= 0 && c_off + c <= c_total, "ctsi_heun_step: bad channel slice");
    const long long vox = (long long)d * h * w, total = (long long)n * c * vox;
    const bool vec = (c % 4) == 0 && aligned(z, 16) && aligned(eps, 16) && aligned(d1, 16) &&
                     (c_total | c_off) % 4 == 0 && aligned(zin, 4 * sizeof(ZT));
    const long long work = vec ? total / 4 : total;
    long long blocks = (work + 255) / 256;
    if (blocks > (1ll << 20)) blocks = 1ll << 20;
    if (vec)
        hipLaunchKernelGGL((heun_step_vec4_kernel<ZT>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z,
                           eps, d1, noise, zin, c_total, c_off, coef, step_ptr, c, vox, work, nonfinite);
    else
        hipLaunchKernelGGL((heun_step_scalar_kernel<ZT>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z,
                           eps, d1, noise, zin, c_total, c_off, coef, step_ptr, c, vox, work, nonfinite);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

}  // namespace

extern "C" int ctsi_dpm_step(float* z, const float* eps, float* x0_prev, void* zin, int c_total, int c_off,
                             const float* coef, const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite,
                             void* stream) {
    return dpm_step(z, eps, x0_prev, (bf16_t*)zin, c_total, c_off, coef, step_ptr, n, c, d, h, w, nonfinite, stream);
}
extern "C" int ctsi_dpm_step_f32(float* z, const float* eps, float* x0_prev, float* zin, int c_total, int c_off,
                                 const float* coef, const int* step_ptr, int n, int c, int d, int h, int w,
                                 int* nonfinite, void* stream) {
    return dpm_step(z, eps, x0_prev, zin, c_total, c_off, coef, step_ptr, n, c, d, h, w, nonfinite, stream);
}

extern "C" int ctsi_heun_step(float* z, const float* eps, float* d1, const float* noise, void* zin, int c_total,
                              int c_off, const float* coef, const int* step_ptr, int n, int c, int d, int h, int w,
                              int* nonfinite, void* stream) {
    return heun_step(z, eps, d1, noise, (bf16_t*)zin, c_total, c_off, coef, step_ptr, n, c, d, h, w, nonfinite,
                     stream);
}
extern "C" int ctsi_heun_step_f32(float* z, const float* eps, float* d1, const float* noise, float* zin, int c_total,
                                  int c_off, const float* coef, const int* step_ptr, int n, int c, int d, int h, int w,
                                  int* nonfinite, void* stream) {
    return heun_step(z, eps, d1, noise, zin, c_total, c_off, coef, step_ptr, n, c, d, h, w, nonfinite, stream);
}
