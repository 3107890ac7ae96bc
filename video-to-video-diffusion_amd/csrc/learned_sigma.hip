// Learned reverse variance and the respaced ancestral step (Nichol & Dhariwal 2021, "Improved DDPM").
// A U-Net built with learn_sigma=True ends in a head of 2L channels: [0, L) the prediction (eps or v), [L, 2L) the raw variance
// channels v.  The reverse log-variance is f log(beta) + (1 - f) log(beta~), f = (v + 1) / 2 -- not clamped, as in the paper.
//   ctsi_sigma_split        the head's fp32 NDHWC 2L-channel output -> the packed L-channel eps buffer every other kernel
//                           reads (+ the variance channels of the first n_keep rows), one pass
//   ctsi_ddpm_lv_step[_f32] the ancestral update on a (respaced) chain with the learned or the fixed-small variance
//   ctsi_ddpm_posterior_lv  the same step on fp32 NCDHW tensors with one coefficient row per sample (p_mean_variance / p_sample)
//   ctsi_hybrid_loss_fwd/_bwd  L_simple + lambda L_vb of a 2L-channel prediction and its gradient (the training step)
// All HBM-bound: 16-byte fp32 accesses when the channel count and the pointers allow, one element per thread otherwise; capped
// grids that stride.  The only reduction (the loss) adds fp64 partials in a fixed order; no atomics anywhere.
#include "ctsi_internal.h"
#include <math.h>

namespace {

constexpr int LS_MAX_BLOCKS = 2048;        // 256 CUs x 8 blocks of 256 threads

inline unsigned grid_for(long long work) {
    long long blocks = (work + 255) / 256;
    return (unsigned)(blocks > LS_MAX_BLOCKS ? LS_MAX_BLOCKS : blocks);
}

// ---- split -----------------------------------------------------------------------------------------------------------
// one float4 of the 2L-channel row per thread and iteration: group g of voxel-row nv goes to eps (g < L/4) or vraw
__global__ void __launch_bounds__(256)
sigma_split_vec4_kernel(const float4* __restrict__ out2, float4* __restrict__ eps, float4* __restrict__ vraw, int l4,
                        long long total4, long long keep_rows) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total4; q += (long long)gridDim.x * 256) {
        const long long nv = q / (2 * l4);
        const int g = (int)(q - nv * (2 * l4));
        if (g < l4) eps[nv * l4 + g] = out2[q];
        else if (vraw != nullptr && nv < keep_rows) vraw[nv * l4 + (g - l4)] = out2[q];
    }
}

__global__ void __launch_bounds__(256)
sigma_split_scalar_kernel(const float* __restrict__ out2, float* __restrict__ eps, float* __restrict__ vraw, int L,
                          long long total, long long keep_rows) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long nv = e / (2 * L);
        const int ch = (int)(e - nv * (2 * L));
        if (ch < L) eps[nv * L + ch] = out2[e];
        else if (vraw != nullptr && nv < keep_rows) vraw[nv * L + (ch - L)] = out2[e];
    }
}

// ---- step ------------------------------------------------------------------------------------------------------------
// row = {sqrt(1 - abar), sqrt(abar), coef1', coef2', log beta', log beta~' (clipped), s, clip}
// s = [not the last step] * exp(log beta~' / 2) is the fixed-small noise scale, formed on the host (on the full chain it is the
// fp32 value ctsi_ddpm_step's row holds).  The learned scale is s * exp(f (c4 - c5) / 2) = [not last] * exp(lv / 2).
struct LvCoef {
    float c0, c1, c2, c3, c4, c5, c6, clip;
};

__device__ __forceinline__ LvCoef lv_coef(const float* cf) {
    LvCoef k;
    k.c0 = cf[0], k.c1 = cf[1], k.c2 = cf[2], k.c3 = cf[3], k.c4 = cf[4], k.c5 = cf[5], k.c6 = cf[6], k.clip = cf[7];
    return k;
}

// the posterior mean from z_t and eps, with the roundings of sampler_step_kernel<DDPM> spelled out so that the two agree bit
// for bit whatever the compiler contracts: z - c0 eps fused, the two products of the mean rounded separately (the sibling's
// are one packed multiply), the noise term fused onto it (lv_add_noise).  The nan_to_num guards are the identity on finite
// values.
__device__ __forceinline__ float lv_mean(float zt, float ep, const LvCoef& k) {
#pragma clang fp contract(off)      // only the fmaf below fuses
    ep = nan_to_num_f(ep);
    float z0 = fmaf(-k.c0, ep, zt) / k.c1;
    z0 = nan_to_num_f(z0);
    if (k.clip > 0.0f) z0 = fminf(fmaxf(z0, -k.clip), k.clip);
    const float a = k.c2 * z0, b = k.c3 * zt;
    return a + b;
}

__device__ __forceinline__ float lv_add_noise(float mean, float scale, float nz) { return fmaf(scale, nz, mean); }

__device__ __forceinline__ float lv_logvar(float v, const LvCoef& k) {
    const float f = (v + 1.0f) * 0.5f;
    return f * k.c4 + (1.0f - f) * k.c5;
}

// exp(lv / 2) = exp(c5 / 2) exp(f (c4 - c5) / 2): the first factor is in c6
__device__ __forceinline__ float lv_scale(float v, const LvCoef& k) {
    const float f = (v + 1.0f) * 0.5f;
    return k.c6 * expf(0.5f * (f * (k.c4 - k.c5)));
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

// 4 consecutive channels of one voxel per thread and iteration (c % 4 == 0, 16-byte aligned fp32 tensors)
template <typename ZT>
__global__ void __launch_bounds__(256)
ddpm_lv_step_vec4_kernel(float* __restrict__ z, const float* __restrict__ eps, const float* __restrict__ vraw,
                         const float* __restrict__ noise, ZT* __restrict__ zin, int c_total, int c_off,
                         const float* __restrict__ coef, const int* __restrict__ step_ptr, int c, long long vox,
                         long long total4) {
    const int step = step_ptr ? *step_ptr : 0;
    const LvCoef k = lv_coef(coef + (long long)step * 8);
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total4; q += (long long)gridDim.x * 256) {
        const long long e = q * 4;
        const long long nv = e / c;
        const int ch = (int)(e - nv * c);
        const float4 zt4 = reinterpret_cast<const float4*>(z)[q];
        const float4 ep4 = reinterpret_cast<const float4*>(eps)[q];
        const float zt[4] = {zt4.x, zt4.y, zt4.z, zt4.w}, ep[4] = {ep4.x, ep4.y, ep4.z, ep4.w};
        float sc[4] = {k.c6, k.c6, k.c6, k.c6};
        if (vraw) {
            const float4 v4 = reinterpret_cast<const float4*>(vraw)[q];
            sc[0] = lv_scale(v4.x, k), sc[1] = lv_scale(v4.y, k), sc[2] = lv_scale(v4.z, k), sc[3] = lv_scale(v4.w, k);
        }
        float zn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) zn[j] = lv_mean(zt[j], ep[j], k);
        if (noise) {       // NCDHW: the 4 channels are vox apart (coalesced across the wave's voxels)
            const long long nb = nv / vox, v = nv - nb * vox;
            const float* np = noise + (nb * c + ch) * vox + v;
#pragma unroll
            for (int j = 0; j < 4; ++j) zn[j] = lv_add_noise(zn[j], sc[j], np[j * vox]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) zn[j] = nan_to_num_f(zn[j]);
        reinterpret_cast<float4*>(z)[q] = make_float4(zn[0], zn[1], zn[2], zn[3]);
        if (zin) store4(zin + nv * c_total + c_off + ch, zn);
    }
}

// any channel count / alignment: one element per thread and iteration
template <typename ZT>
__global__ void __launch_bounds__(256)
ddpm_lv_step_scalar_kernel(float* __restrict__ z, const float* __restrict__ eps, const float* __restrict__ vraw,
                           const float* __restrict__ noise, ZT* __restrict__ zin, int c_total, int c_off,
                           const float* __restrict__ coef, const int* __restrict__ step_ptr, int c, long long vox,
                           long long total) {
    const int step = step_ptr ? *step_ptr : 0;
    const LvCoef k = lv_coef(coef + (long long)step * 8);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long nv = e / c;
        const int ch = (int)(e - nv * c);
        float zn = lv_mean(z[e], eps[e], k);
        if (noise) {
            const long long nb = nv / vox, v = nv - nb * vox;
            const float sc = vraw ? lv_scale(vraw[e], k) : k.c6;
            zn = lv_add_noise(zn, sc, noise[(nb * c + ch) * vox + v]);
        }
        zn = nan_to_num_f(zn);
        z[e] = zn;
        if (zin) store1(zin + nv * c_total + c_off + ch, zn);
    }
}

template <typename ZT>
int ddpm_lv_step(float* z, const float* eps, const float* vraw, const float* noise, ZT* zin, int c_total, int c_off,
                 const float* coef, const int* step_ptr, int n, int c, int d, int h, int w, void* stream) {
    CTSI_CHECK_ARG(z && eps && coef, "ctsi_ddpm_lv_step: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_ddpm_lv_step: bad shape n=%d c=%d d=%d h=%d w=%d", n, c,
                   d, h, w);
    CTSI_CHECK_ARG(!zin || (c_off >= 0 && c_off + c <= c_total), "ctsi_ddpm_lv_step: bad channel slice");
    const long long vox = (long long)d * h * w, total = (long long)n * c * vox;
    const bool vec = (c % 4) == 0 && aligned16(z) && aligned16(eps) && aligned16(vraw) &&
                     (!zin || ((c_total | c_off) % 4 == 0 && ((uintptr_t)zin & (4 * sizeof(ZT) - 1)) == 0));
    const long long work = vec ? total / 4 : total;
    if (vec)
        hipLaunchKernelGGL((ddpm_lv_step_vec4_kernel<ZT>), dim3(grid_for(work)), dim3(256), 0, (hipStream_t)stream, z, eps,
                           vraw, noise, zin, c_total, c_off, coef, step_ptr, c, vox, work);
    else
        hipLaunchKernelGGL((ddpm_lv_step_scalar_kernel<ZT>), dim3(grid_for(work)), dim3(256), 0, (hipStream_t)stream, z, eps,
                           vraw, noise, zin, c_total, c_off, coef, step_ptr, c, vox, work);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- per-sample rows, fp32 NCDHW (the single-step API) ----------------------------------------------------------------------
__global__ void __launch_bounds__(256)
ddpm_posterior_lv_kernel(const float* __restrict__ z, const float* __restrict__ eps, const float* __restrict__ vraw,
                         const float* __restrict__ noise, float* __restrict__ out, float* __restrict__ logvar_out,
                         const float* __restrict__ coef, long long per_sample, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const float* cf = coef + (e / per_sample) * 8;
        const LvCoef k = lv_coef(cf);
        const float lv = vraw ? lv_logvar(vraw[e], k) : k.c5;
        if (logvar_out) logvar_out[e] = lv;
        if (out) {
            float m = lv_mean(z[e], eps[e], k);
            if (noise) m = lv_add_noise(m, vraw ? lv_scale(vraw[e], k) : k.c6, noise[e]);
            out[e] = nan_to_num_f(m);
        }
    }
}

// ---- hybrid loss -------------------------------------------------------------------------------------------------------
// pred2: fp32 NDHWC, 2L channels: [0, L) the prediction p (eps, or v when v_pred), [L, 2L) the variance channels v.  z0, noise:
// fp32 NCDHW.  sched: one row per TIMESTEP {sqrt(abar), sqrt(1 - abar), coef1, coef2, log beta, log beta~ (clipped), log beta - log beta~, 0};
// sample b reads row t[b].  Per element, in registers:
//   z_t = a z0 + s noise;   target = noise | a noise - s z0;   z0_pred = (z_t - s p) / a | a z_t - s p   (not clipped)
//   mse term = (p - target)^2
//   lv = f c4 + (1 - f) c5,  f = (v + 1) / 2
//   t > 0:  vb term = 1/2 (-1 + lv - c5 + e^(c5 - lv) + (c1 (z0 - z0_pred))^2 e^-lv)           KL(q(z_{t-1}|z_t,z_0) || p_theta)
//   t = 0:  vb term = 1/2 (ln 2 pi + lv + (z0 - c1 z0_pred - c2 z_t)^2 e^-lv)                   continuous Gaussian NLL, nats
// The host folds the batch / element / mask normalisation (and lambda / ln 2 of the bound) into norm[b] and norm_vb[b].
constexpr int HL_BLOCKS = 64;                       // partial sums per sample and term
constexpr float HL_LN_2PI = 1.8378770664093453f;

struct HlRow {
    float a, s, c1, c2, c4, c5, d45;
    bool t0;
};

__device__ __forceinline__ HlRow hl_row(const float* sched, const int* t, int timesteps, long long nb) {
    int tt = t[nb];
    tt = tt < 0 ? 0 : (tt >= timesteps ? timesteps - 1 : tt);       // (validated on the host; never read beside the table)
    const float* r = sched + (long long)tt * 8;
    HlRow k;
    k.a = r[0], k.s = r[1], k.c1 = r[2], k.c2 = r[3], k.c4 = r[4], k.c5 = r[5], k.d45 = r[6];
    k.t0 = tt == 0;
    return k;
}

struct HlElem {
    float dp;        // p - target
    float vb;        // the bound's element term (nats)
    float dvb_dv;    // its derivative with respect to the variance channel
};

__device__ __forceinline__ HlElem hl_elem(float p, float v, float z0e, float nz, const HlRow& k, int v_pred) {
    // z0 - z0_pred = s (p - target) in the v form and s (p - target) / a in the eps form, exactly: taken from the prediction
    // error instead of subtracting two numbers of z0's size
    const float zt = k.a * z0e + k.s * nz;
    const float target = v_pred ? k.a * nz - k.s * z0e : nz;
    const float dz0 = v_pred ? k.s * (p - target) : k.s * (p - target) / k.a;
    // lv = c5 + delta with delta = f (c4 - c5): where beta and beta~ nearly agree (large t) the terms of the bound are
    // differences of order delta, so they are formed from delta itself, not from lv - c5
    const float f = (v + 1.0f) * 0.5f;
    const float d45 = k.d45;      // log beta - log beta~ from the host's float64: the fp32 difference of c4 and c5 has lost it
    const float delta = f * d45;
    const float lv = k.c5 + delta;
    const float inv = expf(-lv);
    HlElem o;
    o.dp = p - target;
    float dlv;
    if (k.t0) {
        const float r = (1.0f - k.c1) * z0e + k.c1 * dz0 - k.c2 * zt;      // z0 - c1 z0_pred - c2 z_t
        o.vb = 0.5f * (HL_LN_2PI + lv + r * r * inv);
        dlv = 0.5f * (1.0f - r * r * inv);
    } else {
        const float dmu = k.c1 * dz0;
        const float em1 = expm1f(-delta);            // e^(c5 - lv) - 1
        o.vb = 0.5f * ((delta + em1) + dmu * dmu * inv);
        dlv = 0.5f * (-em1 - dmu * dmu * inv);
    }
    o.dvb_dv = dlv * (0.5f * d45);
    return o;
}

__global__ void __launch_bounds__(256)
hybrid_loss_partial_kernel(const float* __restrict__ pred2, const float* __restrict__ z0, const float* __restrict__ noise,
                           const int* __restrict__ t, const float* __restrict__ sched, int timesteps, int v_pred,
                           const float* __restrict__ mask, int L, long long vox, long long hw, int d,
                           double* __restrict__ partial) {
    __shared__ double s_mse[256], s_vb[256];
    const long long nb = blockIdx.y;
    const HlRow k = hl_row(sched, t, timesteps, nb);
    const long long total = vox * L;
    double acc_mse = 0.0, acc_vb = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int ch = (int)(e % L);
        const long long v = e / L;
        const float* row = pred2 + (nb * vox + v) * 2 * L;
        const long long i = (nb * L + ch) * vox + v;
        const HlElem o = hl_elem(row[ch], row[L + ch], z0[i], noise[i], k, v_pred);
        float m = 1.0f;
        if (mask) m = mask[(nb * L + ch) * d + (v / hw)];
        acc_mse += (double)(m * o.dp * o.dp);
        acc_vb += (double)(m * o.vb);
    }
    s_mse[threadIdx.x] = acc_mse;
    s_vb[threadIdx.x] = acc_vb;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            s_mse[threadIdx.x] += s_mse[threadIdx.x + s];
            s_vb[threadIdx.x] += s_vb[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[(nb * HL_BLOCKS + blockIdx.x) * 2 + 0] = s_mse[0];
        partial[(nb * HL_BLOCKS + blockIdx.x) * 2 + 1] = s_vb[0];
    }
}

// loss_out = {total, mse, vb, mse sums[n], vb sums[n]}: mse = sum_b norm[b] S_b, vb = sum_b norm_vb[b] V_b, total = mse + vb
__global__ void hybrid_loss_final_kernel(const double* __restrict__ partial, const float* __restrict__ norm,
                                         const float* __restrict__ norm_vb, int n, float* __restrict__ loss_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double mse = 0.0, vb = 0.0;
    for (int b = 0; b < n; ++b) {
        double s = 0.0, u = 0.0;
        for (int j = 0; j < HL_BLOCKS; ++j) {
            s += partial[((long long)b * HL_BLOCKS + j) * 2 + 0];
            u += partial[((long long)b * HL_BLOCKS + j) * 2 + 1];
        }
        loss_out[3 + b] = (float)s;
        loss_out[3 + n + b] = (float)u;
        mse += (double)norm[b] * s;
        vb += (double)norm_vb[b] * u;
    }
    loss_out[0] = (float)(mse + vb);
    loss_out[1] = (float)mse;
    loss_out[2] = (float)vb;
}

// d_pred: bf16 NDHWC, c_stride >= 2L channels per voxel, the padding channels zero
__global__ void __launch_bounds__(256)
hybrid_loss_bwd_kernel(const float* __restrict__ pred2, const float* __restrict__ z0, const float* __restrict__ noise,
                       const int* __restrict__ t, const float* __restrict__ sched, int timesteps, int v_pred,
                       const float* __restrict__ mask, const float* __restrict__ norm, const float* __restrict__ norm_vb,
                       const float* __restrict__ gscale, int L, long long vox, long long hw, int d,
                       bf16_t* __restrict__ dpred, int c_stride, long long total /* n * vox * L */) {
    const float gs = gscale ? gscale[0] : 1.0f;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int ch = (int)(e % L);
        const long long nv = e / L;
        const long long nb = nv / vox, v = nv - nb * vox;
        const HlRow k = hl_row(sched, t, timesteps, nb);
        const float* row = pred2 + nv * 2 * L;
        const long long i = (nb * L + ch) * vox + v;
        const HlElem o = hl_elem(row[ch], row[L + ch], z0[i], noise[i], k, v_pred);
        float m = 1.0f;
        if (mask) m = mask[(nb * L + ch) * d + (v / hw)];
        bf16_t* out = dpred + nv * c_stride;
        out[ch] = f32_to_bf16(2.0f * norm[nb] * m * o.dp * gs);
        out[L + ch] = f32_to_bf16(norm_vb[nb] * m * o.dvb_dv * gs);
        if (ch == 0)
            for (int pc = 2 * L; pc < c_stride; ++pc) out[pc] = 0;
    }
}

}  // namespace

extern "C" size_t ctsi_hybrid_loss_workspace_doubles(int n) { return n > 0 ? (size_t)n * HL_BLOCKS * 2 : 0; }

extern "C" int ctsi_hybrid_loss_fwd(const float* pred2, const float* z0, const float* noise, const int* t, const float* sched,
                                    int timesteps, int v_pred, const float* mask, const float* norm, const float* norm_vb,
                                    int n, int L, int d, int h, int w, double* workspace, float* loss_out, void* stream) {
    CTSI_CHECK_ARG(pred2 && z0 && noise && t && sched && norm && norm_vb && workspace && loss_out,
                   "ctsi_hybrid_loss_fwd: null argument");
    CTSI_CHECK_ARG(n > 0 && L > 0 && d > 0 && h > 0 && w > 0 && timesteps > 0 && (v_pred == 0 || v_pred == 1),
                   "ctsi_hybrid_loss_fwd: bad sizes n=%d L=%d d=%d h=%d w=%d timesteps=%d v_pred=%d", n, L, d, h, w, timesteps,
                   v_pred);
    const long long hw = (long long)h * w, vox = hw * d;
    hipLaunchKernelGGL(hybrid_loss_partial_kernel, dim3(HL_BLOCKS, n), dim3(256), 0, (hipStream_t)stream, pred2, z0, noise, t,
                       sched, timesteps, v_pred, mask, L, vox, hw, d, workspace);
    CTSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(hybrid_loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, workspace, norm, norm_vb, n,
                       loss_out);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_hybrid_loss_bwd(const float* pred2, const float* z0, const float* noise, const int* t, const float* sched,
                                    int timesteps, int v_pred, const float* mask, const float* norm, const float* norm_vb,
                                    const float* gscale, int n, int L, int d, int h, int w, void* dpred, int c_stride,
                                    void* stream) {
    CTSI_CHECK_ARG(pred2 && z0 && noise && t && sched && norm && norm_vb && dpred, "ctsi_hybrid_loss_bwd: null argument");
    CTSI_CHECK_ARG(n > 0 && L > 0 && d > 0 && h > 0 && w > 0 && timesteps > 0 && (v_pred == 0 || v_pred == 1) &&
                       c_stride >= 2 * L,
                   "ctsi_hybrid_loss_bwd: bad sizes n=%d L=%d d=%d h=%d w=%d timesteps=%d v_pred=%d c_stride=%d", n, L, d, h,
                   w, timesteps, v_pred, c_stride);
    const long long hw = (long long)h * w, vox = hw * d, total = vox * n * L;
    hipLaunchKernelGGL(hybrid_loss_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, pred2, z0, noise, t,
                       sched, timesteps, v_pred, mask, norm, norm_vb, gscale, L, vox, hw, d, (bf16_t*)dpred, c_stride, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_sigma_split(const float* out2, float* eps, float* vraw, int n, int n_keep, int L, int d, int h, int w,
                                void* stream) {
    CTSI_CHECK_ARG(out2 && eps, "ctsi_sigma_split: null argument");
    CTSI_CHECK_ARG(n > 0 && L > 0 && d > 0 && h > 0 && w > 0, "ctsi_sigma_split: bad shape n=%d L=%d d=%d h=%d w=%d", n, L, d,
                   h, w);
    CTSI_CHECK_ARG(n_keep >= 0 && n_keep <= n && (vraw == nullptr || n_keep > 0),
                   "ctsi_sigma_split: n_keep=%d outside [%d, n=%d]", n_keep, vraw ? 1 : 0, n);
    const long long vox = (long long)d * h * w, total = (long long)n * vox * 2 * L, keep_rows = (long long)n_keep * vox;
    if (L % 4 == 0 && aligned16(out2) && aligned16(eps) && aligned16(vraw))
        hipLaunchKernelGGL(sigma_split_vec4_kernel, dim3(grid_for(total / 4)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4*>(out2), reinterpret_cast<float4*>(eps),
                           reinterpret_cast<float4*>(vraw), L / 4, total / 4, keep_rows);
    else
        hipLaunchKernelGGL(sigma_split_scalar_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, out2, eps,
                           vraw, L, total, keep_rows);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_ddpm_lv_step(float* z, const float* eps, const float* vraw, const float* noise, void* zin, int c_total,
                                 int c_off, const float* coef, const int* step_ptr, int n, int c, int d, int h, int w,
                                 void* stream) {
    return ddpm_lv_step(z, eps, vraw, noise, (bf16_t*)zin, c_total, c_off, coef, step_ptr, n, c, d, h, w, stream);
}
extern "C" int ctsi_ddpm_lv_step_f32(float* z, const float* eps, const float* vraw, const float* noise, float* zin,
                                     int c_total, int c_off, const float* coef, const int* step_ptr, int n, int c, int d,
                                     int h, int w, void* stream) {
    return ddpm_lv_step(z, eps, vraw, noise, zin, c_total, c_off, coef, step_ptr, n, c, d, h, w, stream);
}

extern "C" int ctsi_ddpm_posterior_lv(const float* z, const float* eps, const float* vraw, const float* noise, float* out,
                                      float* logvar_out, const float* coef, int n, long long per_sample, void* stream) {
    CTSI_CHECK_ARG(z && eps && coef && (out || logvar_out) && (!logvar_out || vraw),
                   "ctsi_ddpm_posterior_lv: null argument (logvar_out needs vraw)");
    CTSI_CHECK_ARG(n > 0 && per_sample > 0, "ctsi_ddpm_posterior_lv: bad sizes n=%d per_sample=%lld", n, per_sample);
    const long long total = per_sample * n;
    hipLaunchKernelGGL(ddpm_posterior_lv_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, z, eps, vraw,
                       noise, out, logvar_out, coef, per_sample, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
