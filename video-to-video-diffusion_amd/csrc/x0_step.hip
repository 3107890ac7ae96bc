// x0-form sampler update: the DDIM, DDPM and DPM-Solver++ updates of a v-prediction model written on the
// data prediction, so that nothing is divided by alpha = sqrt(abar) (0 at the last step of a zero-terminal-SNR schedule).
// One pass over the latent per step.  It reads z, the network's raw v output, the coefficient row at *step_ptr, and -- only
// where the row uses them -- the history and the noise; it writes z, the z slice of the U-Net input and the history.
//   row  = {alpha, sigma, a, b, c, s, clip, 0}                 (float64 on the host, rounded once; sampler.x0_coef_rows)
//   X    = clamp(nan_to_num(fma(alpha, z, -sigma v)), -clip, clip)          (clip = 0: no clamp)
//   z'   = a z + b X + c hist + s noise
//   hist <- X
// hist is read only by rows with c != 0 and written whenever it is given; noise (fp32 NCDHW) is read only by rows with
// s != 0.  nonfinite: as ctsi_ddim_step -- row *step_ptr counts {v NaN, Inf, X NaN, Inf, z' NaN, Inf}; v is sanitised before
// use and z' before it is stored.  HBM-bound: 16-byte fp32 accesses when the channel count and the pointers allow, one
// element per thread otherwise; the grid is capped and strides.
#include "ctsi_internal.h"

namespace {

constexpr int X0_MAX_BLOCKS = 2048;        // 256 CUs x 8 blocks of 256 threads

struct X0Coef {
    float alpha, sigma, a, b, c, s, clip;
    bool use_hist, use_noise;
};

__device__ __forceinline__ X0Coef x0_coef(const float* cf, const float* hist, const float* noise) {
    X0Coef k;
    k.alpha = cf[0], k.sigma = cf[1], k.a = cf[2], k.b = cf[3], k.c = cf[4], k.s = cf[5], k.clip = cf[6];
    k.use_hist = hist != nullptr && k.c != 0.0f;
    k.use_noise = noise != nullptr && k.s != 0.0f;
    return k;
}

__device__ __forceinline__ void count_nf(float v, int& n_nan, int& n_inf) {
    n_nan += (v != v) ? 1 : 0;
    n_inf += (v == __builtin_inff() || v == -__builtin_inff()) ? 1 : 0;
}

// returns z'; X in x_out.  h and nz are 0 where the row does not use them (the fma then adds an exact 0)
__device__ __forceinline__ float x0_elem(float zt, float v, float h, float nz, const X0Coef& k, float& x_out, int* cnt) {
    count_nf(v, cnt[0], cnt[1]);
    v = nan_to_num_f(v);
    float x = fmaf(k.alpha, zt, -(k.sigma * v));
    count_nf(x, cnt[2], cnt[3]);
    x = nan_to_num_f(x);
    if (k.clip > 0.0f) x = fminf(fmaxf(x, -k.clip), k.clip);
    float zn = fmaf(k.b, x, k.a * zt);
    if (k.use_hist) zn = fmaf(k.c, h, zn);
    if (k.use_noise) zn = fmaf(k.s, nz, zn);
    count_nf(zn, cnt[4], cnt[5]);
    x_out = x;
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
x0_step_vec4_kernel(float* __restrict__ z, const float* __restrict__ vout, float* __restrict__ hist,
                    const float* __restrict__ noise, ZT* __restrict__ zin, int c_total, int c_off,
                    const float* __restrict__ coef, const int* __restrict__ step_ptr, int c, long long vox,
                    long long total4, int* __restrict__ nonfinite) {
    const int step = step_ptr ? *step_ptr : 0;
    const X0Coef k = x0_coef(coef + (long long)step * 8, hist, noise);
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total4; q += (long long)gridDim.x * 256) {
        const long long e = q * 4;
        const long long nv = e / c;
        const int ch = (int)(e - nv * c);
        const float4 zt = reinterpret_cast<const float4*>(z)[q];
        const float4 vv = reinterpret_cast<const float4*>(vout)[q];
        const float4 h = k.use_hist ? reinterpret_cast<const float4*>(hist)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (k.use_noise) {     // NCDHW: the 4 channels are vox apart (coalesced across the wave's voxels)
            const long long nb = nv / vox, v = nv - nb * vox;
            const float* np = noise + (nb * c + ch) * vox + v;
#pragma unroll
            for (int j = 0; j < 4; ++j) nz[j] = np[j * vox];
        }
        float zn[4], x[4];
        zn[0] = x0_elem(zt.x, vv.x, h.x, nz[0], k, x[0], cnt);
        zn[1] = x0_elem(zt.y, vv.y, h.y, nz[1], k, x[1], cnt);
        zn[2] = x0_elem(zt.z, vv.z, h.z, nz[2], k, x[2], cnt);
        zn[3] = x0_elem(zt.w, vv.w, h.w, nz[3], k, x[3], cnt);
        reinterpret_cast<float4*>(z)[q] = make_float4(zn[0], zn[1], zn[2], zn[3]);
        if (hist) reinterpret_cast<float4*>(hist)[q] = make_float4(x[0], x[1], x[2], x[3]);
        if (zin) store4(zin + nv * c_total + c_off + ch, zn);
    }
    flush_counts(cnt, nonfinite, step);
}

// any channel count / alignment: one element per thread and iteration
template <typename ZT>
__global__ void __launch_bounds__(256)
x0_step_scalar_kernel(float* __restrict__ z, const float* __restrict__ vout, float* __restrict__ hist,
                      const float* __restrict__ noise, ZT* __restrict__ zin, int c_total, int c_off,
                      const float* __restrict__ coef, const int* __restrict__ step_ptr, int c, long long vox,
                      long long total, int* __restrict__ nonfinite) {
    const int step = step_ptr ? *step_ptr : 0;
    const X0Coef k = x0_coef(coef + (long long)step * 8, hist, noise);
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long nv = e / c;
        const int ch = (int)(e - nv * c);
        const float h = k.use_hist ? hist[e] : 0.0f;
        float nz = 0.0f;
        if (k.use_noise) {
            const long long nb = nv / vox, v = nv - nb * vox;
            nz = noise[(nb * c + ch) * vox + v];
        }
        float x;
        const float zn = x0_elem(z[e], vout[e], h, nz, k, x, cnt);
        z[e] = zn;
        if (hist) hist[e] = x;
        if (zin) store1(zin + nv * c_total + c_off + ch, zn);
    }
    flush_counts(cnt, nonfinite, step);
}

inline bool aligned(const void* p, unsigned bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

template <typename ZT>
int x0_step(float* z, const float* v, float* hist, const float* noise, ZT* zin, int c_total, int c_off, const float* coef,
            const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite, void* stream) {
    CTSI_CHECK_ARG(z && v && coef, "ctsi_x0_step: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_x0_step: bad shape n=%d c=%d d=%d h=%d w=%d", n, c, d,
                   h, w);
    CTSI_CHECK_ARG(!zin || (c_off >= 0 && c_off + c <= c_total), "ctsi_x0_step: bad channel slice");
    const long long vox = (long long)d * h * w, total = (long long)n * c * vox;
    const bool vec = (c % 4) == 0 && aligned(z, 16) && aligned(v, 16) && aligned(hist, 16) &&
                     (!zin || ((c_total | c_off) % 4 == 0 && aligned(zin, 4 * sizeof(ZT))));
    const long long work = vec ? total / 4 : total;
    long long blocks = (work + 255) / 256;
    if (blocks > X0_MAX_BLOCKS) blocks = X0_MAX_BLOCKS;
    if (vec)
        hipLaunchKernelGGL((x0_step_vec4_kernel<ZT>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, v,
                           hist, noise, zin, c_total, c_off, coef, step_ptr, c, vox, work, nonfinite);
    else
        hipLaunchKernelGGL((x0_step_scalar_kernel<ZT>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, v,
                           hist, noise, zin, c_total, c_off, coef, step_ptr, c, vox, work, nonfinite);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

}  // namespace

extern "C" int ctsi_x0_step(float* z, const float* v, float* hist, const float* noise, void* zin, int c_total, int c_off,
                            const float* coef, const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite,
                            void* stream) {
    return x0_step(z, v, hist, noise, (bf16_t*)zin, c_total, c_off, coef, step_ptr, n, c, d, h, w, nonfinite, stream);
}
extern "C" int ctsi_x0_step_f32(float* z, const float* v, float* hist, const float* noise, float* zin, int c_total,
                                int c_off, const float* coef, const int* step_ptr, int n, int c, int d, int h, int w,
                                int* nonfinite, void* stream) {
    return x0_step(z, v, hist, noise, zin, c_total, c_off, coef, step_ptr, n, c, d, h, w, nonfinite, stream);
}
