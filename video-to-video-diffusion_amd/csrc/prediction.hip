// v-prediction (Salimans & Ho 2022): v = sqrt(abar) eps - sqrt(1 - abar) z_0.
//   pred_to_eps   between the U-Net and everything that reads eps (guidance, update, counters): the network's v output becomes
//                 eps in place,  out[b] <- a out[b] + b0 z[b % z_rows] + b1 hist[b % z_rows],  {a, b0, b1, 0} = row
//                 *step_ptr * rows_per_step + b % rows_per_step of a device table: one captured graph serves every step.
//                 With z the network's input z_t, {sqrt(abar), sqrt(1 - abar), 0} is eps = sqrt(abar) v + sqrt(1 - abar) z_t;
//                 the Heun corrector's input c4 zhat + c5 D1 is not stored, so its row is {alpha, beta c4, beta c5} on
//                 z = zhat, hist = D1.
//   q_sample_v    the training inputs: ctsi_q_sample's z_t slice (the same expression: the same bits) and the fp32 target
//                 v = sqrt_ac[t] noise - sqrt_1mac[t] z0 from one pass over z0 and noise.
// Both stream once over the latent: HBM-bound.  pred_to_eps: 16-byte accesses when the sizes and pointers allow, grid capped
// at 2048 blocks with a grid-stride loop.  z / hist are loaded only by the rows whose coefficient is not 0 (block-uniform).
#include "ctsi_internal.h"

namespace {

constexpr int PRED_MAX_BLOCKS = 2048;        // 256 CUs x 8 blocks of 256 threads

struct PredRow {
    float a, b0, b1;
};

__device__ __forceinline__ PredRow pred_row(const float* __restrict__ rows, const int* __restrict__ step_ptr,
                                            int rows_per_step, int b) {
    const int step = step_ptr ? *step_ptr : 0;
    const float* r = rows + ((long long)step * rows_per_step + (b % rows_per_step)) * 4;
    return PredRow{r[0], r[1], r[2]};
}

// a v (+ b0 z) (+ b1 h): one product, then one fma per term that is present
template <bool Z, bool H>
__device__ __forceinline__ float to_eps(float v, float z, float h, const PredRow& r) {
    float e = r.a * v;
    if (Z) e = fmaf(r.b0, z, e);
    if (H) e = fmaf(r.b1, h, e);
    return e;
}

// grid (x, n): output row blockIdx.y; T = float4 (per_sample % 4 == 0, 16-byte aligned rows) or float
template <typename T, bool Z, bool H>
__device__ __forceinline__ void pred_rows_loop(T* __restrict__ po, const T* __restrict__ pz, const T* __restrict__ ph,
                                               long long count, const PredRow& r) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < count; q += (long long)gridDim.x * 256) {
        T v = po[q], z = v, h = v;
        if (Z) z = pz[q];
        if (H) h = ph[q];
        if constexpr (sizeof(T) == 16) {
            v.x = to_eps<Z, H>(v.x, z.x, h.x, r);
            v.y = to_eps<Z, H>(v.y, z.y, h.y, r);
            v.z = to_eps<Z, H>(v.z, z.z, h.z, r);
            v.w = to_eps<Z, H>(v.w, z.w, h.w, r);
        } else {
            v = to_eps<Z, H>(v, z, h, r);
        }
        po[q] = v;
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
pred_to_eps_kernel(float* __restrict__ out, const float* __restrict__ z, const float* __restrict__ hist,
                   const float* __restrict__ rows, const int* __restrict__ step_ptr, int rows_per_step, int z_rows,
                   long long per_sample) {
    const int b = blockIdx.y;
    const PredRow r = pred_row(rows, step_ptr, rows_per_step, b);
    const long long zb = b % z_rows;
    T* po = reinterpret_cast<T*>(out + (long long)b * per_sample);
    const T* pz = reinterpret_cast<const T*>(z + zb * per_sample);
    const T* ph = reinterpret_cast<const T*>(hist ? hist + zb * per_sample : nullptr);
    const long long count = per_sample / (long long)(sizeof(T) / sizeof(float));
    const bool use_z = r.b0 != 0.0f, use_h = r.b1 != 0.0f && hist != nullptr;      // block-uniform
    if (use_z && use_h)
        pred_rows_loop<T, true, true>(po, pz, ph, count, r);
    else if (use_z)
        pred_rows_loop<T, true, false>(po, pz, ph, count, r);
    else if (use_h)
        pred_rows_loop<T, false, true>(po, pz, ph, count, r);
    else
        pred_rows_loop<T, false, false>(po, pz, ph, count, r);
}

// z_t exactly as q_sample_kernel (train_ops.hip) forms it, and the v target of the same elements
__global__ void __launch_bounds__(256)
q_sample_v_kernel(const float* __restrict__ z0, const float* __restrict__ noise, const float* __restrict__ sqrt_ac,
                  const float* __restrict__ sqrt_1mac, const int* __restrict__ t, bf16_t* __restrict__ dst,
                  float* __restrict__ v_target, int c, long long vox, int c_total, int c_off, long long total /* n*vox */) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long nb = e / vox, v = e - nb * vox;
        const int tt = t[nb];
        const float a = sqrt_ac[tt], s = sqrt_1mac[tt];
        for (int ch = 0; ch < c; ++ch) {
            const long long i = (nb * c + ch) * vox + v;
            const float x = z0[i], ns = noise[i];
            dst[e * c_total + c_off + ch] = f32_to_bf16(fmaf(a, x, s * ns));      // how hipcc contracts a * z0 + s * noise there
            v_target[i] = fmaf(a, ns, -(s * x));
        }
    }
}

}  // namespace

extern "C" int ctsi_pred_to_eps(float* out, const float* z, const float* hist, const float* rows, const int* step_ptr,
                                int rows_per_step, int n, int z_rows, long long per_sample, void* stream) {
    CTSI_CHECK_ARG(out && z && rows, "ctsi_pred_to_eps: null argument");
    CTSI_CHECK_ARG(n > 0 && n <= 65535 && z_rows > 0 && z_rows <= n && per_sample > 0,
                   "ctsi_pred_to_eps: bad shape n=%d z_rows=%d per_sample=%lld", n, z_rows, per_sample);
    CTSI_CHECK_ARG(rows_per_step > 0 && rows_per_step <= n, "ctsi_pred_to_eps: bad rows_per_step=%d (n=%d)", rows_per_step,
                   n);
    const bool vec = (per_sample % 4) == 0 && aligned16(out) && aligned16(z) && aligned16(hist);
    const long long work = vec ? per_sample / 4 : per_sample;
    long long blocks = (work + 255) / 256;
    const long long cap = PRED_MAX_BLOCKS / n > 0 ? PRED_MAX_BLOCKS / n : 1;
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks, (unsigned)n);
    if (vec)
        hipLaunchKernelGGL((pred_to_eps_kernel<float4>), grid, dim3(256), 0, (hipStream_t)stream, out, z, hist, rows,
                           step_ptr, rows_per_step, z_rows, per_sample);
    else
        hipLaunchKernelGGL((pred_to_eps_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, out, z, hist, rows,
                           step_ptr, rows_per_step, z_rows, per_sample);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_q_sample_v(const float* z0, const float* noise, const float* sqrt_ac, const float* sqrt_1mac,
                               const int* t, void* dst, float* v_target, int n, int c, int d, int h, int w, int c_total,
                               int c_off, void* stream) {
    CTSI_CHECK_ARG(z0 && noise && sqrt_ac && sqrt_1mac && t && dst && v_target, "ctsi_q_sample_v: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0 && c_off >= 0 && c_off + c <= c_total,
                   "ctsi_q_sample_v: bad shape n=%d c=%d d=%d h=%d w=%d c_total=%d c_off=%d", n, c, d, h, w, c_total, c_off);
    const long long vox = (long long)d * h * w, total = vox * n;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(q_sample_v_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z0, noise, sqrt_ac,
                       sqrt_1mac, t, (bf16_t*)dst, v_target, c, vox, c_total, c_off, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
