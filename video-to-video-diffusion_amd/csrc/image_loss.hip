// Image-space loss terms of the diffusion stage: the two joints between the training step's loss head and
// an autograd loss on the decoded prediction.
//   z0_pred       the predicted clean latent from the training program's own buffers, fp32 NCDHW:
//                   z_t = sqrt_ac[t] z0 + sqrt_1mac[t] noise          (the expression of q_sample_kernel)
//                   epsilon:  z0^ = (z_t - sqrt_1mac[t] eps^) / sqrt_ac[t]     (= sqrt_recip_ac z_t - sqrt_recipm1_ac eps^, the
//                             arithmetic of ctsi_ddpm_posterior, i.e. of _predict_z_0_from_noise)
//                   v:        z0^ = sqrt_ac[t] z_t - sqrt_1mac[t] v^            (_predict_z_0_from_v: no division)
//                 rows with active[b] == 0 are written as z0 itself (no NaN, no 1 / sqrt_ac garbage at t -> T).
//   loss_bwd_z0   mse_loss_bwd_kernel's expression plus the gradient that came back through z0^,
//                   d_pred = gscale 2 norm[b] mask (pred - target) + active[b] coef[b] g_z0,   coef = d z0^ / d pred,
//                 formed in fp32 and rounded ONCE to the bf16 NDHWC gradient buffer.
// Both stream once over the latent (HBM-bound).  z0_pred turns NDHWC into NCDHW: a thread of the 16-byte form owns four
// consecutive voxels, reads the prediction as one float4 per voxel and channel quad and z0 / noise as one float4 per channel,
// and writes one float4 per channel (a 4 x 4 transpose in registers); the element-wise form is ctsi_ndhwc_f32_to_ncdhw_f32's
// loop (one voxel per thread).
#include "ctsi_internal.h"

namespace {

constexpr int Z0_MAX_BLOCKS = 8192;

struct Z0Row {
    float a, s;
    bool active;
};

template <bool V>
__device__ __forceinline__ float z0_hat(float x, float ns, float p, const Z0Row& r) {
    const float zt = fmaf(r.a, x, r.s * ns);
    if (V) return fmaf(-r.s, p, r.a * zt);
    return fmaf(-r.s, p, zt) / r.a;
}

// one voxel per thread, channels in a loop (any c, any c_stride >= c, any alignment)
template <bool V>
__global__ void __launch_bounds__(256)
z0_pred_kernel(const float* __restrict__ z0, const float* __restrict__ noise, const float* __restrict__ pred,
               const float* __restrict__ sqrt_ac, const float* __restrict__ sqrt_1mac, const int* __restrict__ t,
               const int* __restrict__ active, float* __restrict__ out, int c, int c_stride, long long vox,
               long long total /* n * vox */) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long nb = e / vox, v = e - nb * vox;
        const int tt = t[nb];
        const Z0Row r{sqrt_ac[tt], sqrt_1mac[tt], active[nb] != 0};
        for (int ch = 0; ch < c; ++ch) {
            const long long i = (nb * c + ch) * vox + v;
            const float x = z0[i];
            out[i] = r.active ? z0_hat<V>(x, noise[i], pred[e * c_stride + ch], r) : x;
        }
    }
}

// four consecutive voxels of one sample per thread: c % 4 == 0, c_stride % 4 == 0, vox % 4 == 0, 16-byte aligned pointers
template <bool V>
__global__ void __launch_bounds__(256)
z0_pred_vec_kernel(const float* __restrict__ z0, const float* __restrict__ noise, const float* __restrict__ pred,
                   const float* __restrict__ sqrt_ac, const float* __restrict__ sqrt_1mac, const int* __restrict__ t,
                   const int* __restrict__ active, float* __restrict__ out, int c, int c_stride, long long vox,
                   long long quads /* n * vox / 4 */) {
    const long long vq = vox >> 2;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long long)gridDim.x * 256) {
        const long long nb = q / vq, v = (q - nb * vq) << 2;
        const int tt = t[nb];
        const Z0Row r{sqrt_ac[tt], sqrt_1mac[tt], active[nb] != 0};
        const float* pr = pred + (nb * vox + v) * c_stride;
        for (int c0 = 0; c0 < c; c0 += 4) {
            float4 p[4], x[4], ns[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long i = (nb * c + c0 + k) * vox + v;
                x[k] = *reinterpret_cast<const float4*>(z0 + i);
                if (r.active) {
                    ns[k] = *reinterpret_cast<const float4*>(noise + i);
                    p[k] = *reinterpret_cast<const float4*>(pr + (long long)k * c_stride + c0);     // voxel v + k, channels c0..c0+3
                }
            }
            if (r.active) {
                // x[k] / ns[k]: channel c0 + k at voxels v..v+3; p[j]: voxel v + j at channels c0..c0+3
                const float pt[4][4] = {{p[0].x, p[1].x, p[2].x, p[3].x}, {p[0].y, p[1].y, p[2].y, p[3].y},
                                        {p[0].z, p[1].z, p[2].z, p[3].z}, {p[0].w, p[1].w, p[2].w, p[3].w}};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    x[k].x = z0_hat<V>(x[k].x, ns[k].x, pt[k][0], r);
                    x[k].y = z0_hat<V>(x[k].y, ns[k].y, pt[k][1], r);
                    x[k].z = z0_hat<V>(x[k].z, ns[k].z, pt[k][2], r);
                    x[k].w = z0_hat<V>(x[k].w, ns[k].w, pt[k][3], r);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) *reinterpret_cast<float4*>(out + (nb * c + c0 + k) * vox + v) = x[k];
        }
    }
}

// mse_loss_bwd_kernel (train_ops.hip) with the second term: the same first expression, so that g_z0 == 0 gives its bits
__global__ void __launch_bounds__(256)
loss_bwd_z0_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ mask,
                   const float* __restrict__ norm, const float* __restrict__ gscale, const float* __restrict__ g_z0,
                   const int* __restrict__ active, const float* __restrict__ coef, int c, long long vox, long long hw, int d,
                   bf16_t* __restrict__ dpred, int c_stride, long long total /* n*vox*c_stride */) {
    const float gs = gscale ? gscale[0] : 1.0f;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int ch = (int)(e % c_stride);
        const long long nv = e / c_stride;
        const long long nb = nv / vox, v = nv - nb * vox;
        float out = 0.0f;
        if (ch < c) {
            const long long i = (nb * c + ch) * vox + v;
            const float df = pred[nv * c + ch] - target[i];
            float m = 1.0f;
            if (mask) m = mask[(nb * c + ch) * d + (v / hw)];
            out = 2.0f * norm[nb] * m * df * gs;
            if (active[nb] != 0) {
                const float g = g_z0[i];
                if (g != 0.0f) out = fmaf(coef[nb], g, out);      // (a zero gradient leaves the first term's bits, its -0 included)
            }
        }
        dpred[e] = f32_to_bf16(out);
    }
}

}  // namespace

extern "C" int ctsi_z0_pred(const float* z0, const float* noise, const float* pred, int c_stride, const float* sqrt_ac,
                            const float* sqrt_1mac, const int* t, const int* active, int v_prediction, int n, int c, int d,
                            int h, int w, float* out, void* stream) {
    CTSI_CHECK_ARG(z0 && noise && pred && sqrt_ac && sqrt_1mac && t && active && out, "ctsi_z0_pred: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_z0_pred: bad shape n=%d c=%d d=%d h=%d w=%d", n, c, d, h,
                   w);
    CTSI_CHECK_ARG(c_stride >= c, "ctsi_z0_pred: bad channel stride %d (c=%d)", c_stride, c);
    const long long vox = (long long)d * h * w, total = vox * n;
    const bool vec = (c % 4) == 0 && (c_stride % 4) == 0 && (vox % 4) == 0 && aligned16(z0) && aligned16(noise) &&
                     aligned16(pred) && aligned16(out);
    const long long work = vec ? total / 4 : total;
    long long blocks = (work + 255) / 256;
    if (blocks > Z0_MAX_BLOCKS) blocks = Z0_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks);
    if (vec) {
        if (v_prediction)
            hipLaunchKernelGGL((z0_pred_vec_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, z0, noise, pred, sqrt_ac,
                               sqrt_1mac, t, active, out, c, c_stride, vox, work);
        else
            hipLaunchKernelGGL((z0_pred_vec_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, z0, noise, pred, sqrt_ac,
                               sqrt_1mac, t, active, out, c, c_stride, vox, work);
    } else {
        if (v_prediction)
            hipLaunchKernelGGL((z0_pred_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, z0, noise, pred, sqrt_ac,
                               sqrt_1mac, t, active, out, c, c_stride, vox, work);
        else
            hipLaunchKernelGGL((z0_pred_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, z0, noise, pred, sqrt_ac,
                               sqrt_1mac, t, active, out, c, c_stride, vox, work);
    }
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_loss_bwd_z0(const float* pred, const float* target, const float* mask, const float* norm,
                                const float* gscale, const float* g_z0, const int* active, const float* coef, int n, int c,
                                int d, int h, int w, void* dpred, int c_stride, void* stream) {
    CTSI_CHECK_ARG(pred && target && norm && g_z0 && active && coef && dpred, "ctsi_loss_bwd_z0: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_loss_bwd_z0: bad shape n=%d c=%d d=%d h=%d w=%d", n, c, d,
                   h, w);
    CTSI_CHECK_ARG(c_stride >= c, "ctsi_loss_bwd_z0: bad channel stride %d (c=%d)", c_stride, c);
    const long long hw = (long long)h * w, vox = hw * d, total = vox * n * c_stride;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(loss_bwd_z0_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred, target, mask, norm,
                       gscale, g_z0, active, coef, c, vox, hw, d, (bf16_t*)dpred, c_stride, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
