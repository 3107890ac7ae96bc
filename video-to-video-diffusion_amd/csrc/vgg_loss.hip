// The VGG-19 perceptual loss (reference models/losses.py:22-146) around its planar 3x3 convolutions: the input transform and
// its backward, 2 x 2 max pooling and its backward, the per-layer feature distance with its two-stage fixed-order reduction,
// and the one elementwise pass per layer boundary of the backward (loss term + ReLU mask).  All HBM-bound: 16-byte accesses on
// bf16 channels-last images [image][h][w][c], c a multiple of 8.  Every entry takes plain pointers and sizes, allocates
// nothing, keeps no state between calls and is capture-safe; no float atomics anywhere, so results are bit-stable.
#include "feat_common.h"

// ---- input transform ------------------------------------------------------------------------------------------------------
// image i = b * num + s <- slice slices[s] of sample b (fp32 NCDHW, C = 1); channel c = ((x + 1) / 2 - mean_c) / std_c for
// c < 3, channels 3-7 zero (the engine's 8-channel form of a few-channel input)
__global__ void __launch_bounds__(256)
vgg_prep_kernel(const float* __restrict__ x, const int* __restrict__ slices, const float* __restrict__ norm,
                bf16_t* __restrict__ dst, int d, int num, long long hw, long long total) {
    const float m0 = norm[0], m1 = norm[1], m2 = norm[2], s0 = norm[3], s1 = norm[4], s2 = norm[5];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long img = e / hw, pix = e - img * hw;
        const long long bb = img / num;
        const int s = (int)(img - bb * num);
        const float v = (x[(bb * d + slices[s]) * hw + pix] + 1.0f) / 2.0f;
        uint4 pk;
        pk.x = pack_bf16x2((v - m0) / s0, (v - m1) / s1);
        pk.y = pack_bf16x2((v - m2) / s2, 0.0f);
        pk.z = 0u;
        pk.w = 0u;
        *reinterpret_cast<uint4*>(dst + e * 8) = pk;
    }
}

extern "C" int ctsi_vgg_prep(const float* x, const int* slices, const float* norm, void* dst, int b, int d, int num, int h,
                             int w, void* stream) {
    CTSI_CHECK_ARG(x && slices && norm && dst && b > 0 && d > 0 && num > 0 && num <= d && h > 0 && w > 0,
                   "ctsi_vgg_prep: bad arguments (b=%d d=%d num=%d h=%d w=%d)", b, d, num, h, w);
    const long long hw = (long long)h * w, total = hw * b * num;
    hipLaunchKernelGGL(vgg_prep_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, slices, norm,
                       (bf16_t*)dst, d, num, hw, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// grad_pred[b, 0, slices[s]] = sum_c g_c / (2 std_c); every other slice stays zero
__global__ void __launch_bounds__(256)
vgg_prep_bwd_kernel(const bf16_t* __restrict__ g, const int* __restrict__ slices, const float* __restrict__ norm,
                    float* __restrict__ grad, int d, int num, long long hw, long long total) {
    const float r0 = 1.0f / (2.0f * norm[3]), r1 = 1.0f / (2.0f * norm[4]), r2 = 1.0f / (2.0f * norm[5]);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long img = e / hw, pix = e - img * hw;
        const long long bb = img / num;
        const int s = (int)(img - bb * num);
        const uint2 pk = *reinterpret_cast<const uint2*>(g + e * 8);
        grad[(bb * d + slices[s]) * hw + pix] = bf_lo(pk.x) * r0 + bf_hi(pk.x) * r1 + bf_lo(pk.y) * r2;
    }
}

extern "C" int ctsi_vgg_prep_bwd(const void* g, const int* slices, const float* norm, float* grad_pred, int b, int d, int num,
                                 int h, int w, void* stream) {
    CTSI_CHECK_ARG(g && slices && norm && grad_pred && b > 0 && d > 0 && num > 0 && num <= d && h > 0 && w > 0,
                   "ctsi_vgg_prep_bwd: bad arguments (b=%d d=%d num=%d h=%d w=%d)", b, d, num, h, w);
    const long long hw = (long long)h * w, total = hw * b * num;
    if (num < d) CTSI_HIP(hipMemsetAsync(grad_pred, 0, (size_t)b * d * hw * sizeof(float), (hipStream_t)stream));
    hipLaunchKernelGGL(vgg_prep_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)g,
                       slices, norm, grad_pred, d, num, hw, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- 2 x 2 / stride 2 max pooling -------------------------------------------------------------------------------------------
// one thread per (output pixel, 8 channels): four 16-byte loads, one 16-byte store
__device__ __forceinline__ uint32_t max_pair(uint32_t a, uint32_t b) {
    const uint32_t lo = bf_lo(b) > bf_lo(a) ? (b & 0xffffu) : (a & 0xffffu);
    const uint32_t hi = bf_hi(b) > bf_hi(a) ? (b & 0xffff0000u) : (a & 0xffff0000u);
    return lo | hi;
}
__device__ __forceinline__ uint4 max_u4(uint4 a, uint4 b) {
    return uint4{max_pair(a.x, b.x), max_pair(a.y, b.y), max_pair(a.z, b.z), max_pair(a.w, b.w)};
}

__global__ void __launch_bounds__(256)
maxpool2_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int h, int w, int c8, long long total) {
    const int ho = h / 2, wo = w / 2;
    const long long row = (long long)w * c8;                 // one input row, in 16-byte units
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int cg = (int)(e % c8);
        long long r = e / c8;
        const int ow = (int)(r % wo);
        r /= wo;
        const long long img = r / ho;
        const int oh = (int)(r - img * ho);                  // an odd last row / column takes part in no window (torch's floor)
        const uint4* src = reinterpret_cast<const uint4*>(x) + (img * h + 2 * oh) * row + (long long)(2 * ow) * c8 + cg;
        uint4 m = max_u4(src[0], src[c8]);                   // (h, w) row-major: the first maximum wins a tie
        m = max_u4(m, src[row]);
        m = max_u4(m, src[row + c8]);
        reinterpret_cast<uint4*>(y)[e] = m;
    }
}

extern "C" int ctsi_maxpool2_fwd(const void* x, void* y, int n, int h, int w, int c, void* stream) {
    CTSI_CHECK_ARG(x && y && n > 0 && h >= 2 && w >= 2 && c > 0 && c % 8 == 0,
                   "ctsi_maxpool2_fwd: bad arguments (n=%d h=%d w=%d c=%d; h, w at least 2, c a multiple of 8)", n, h, w, c);
    const long long total = (long long)n * (h / 2) * (w / 2) * (c / 8);
    hipLaunchKernelGGL(maxpool2_fwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (bf16_t*)y, h, w, c / 8, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// gx = gy at the first maximum of each window in (h, w) row-major order (torch's rule), 0 at the other three positions
__device__ __forceinline__ void route_pair(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t g, uint32_t* oa,
                                           uint32_t* ob, uint32_t* oc, uint32_t* od) {
    uint32_t out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const float va = half ? bf_hi(a) : bf_lo(a), vb = half ? bf_hi(b) : bf_lo(b);
        const float vc = half ? bf_hi(c) : bf_lo(c), vd = half ? bf_hi(d) : bf_lo(d);
        int k = 0;
        float m = va;
        if (vb > m) { m = vb; k = 1; }
        if (vc > m) { m = vc; k = 2; }
        if (vd > m) { m = vd; k = 3; }
        const uint32_t gg = half ? (g & 0xffff0000u) : (g & 0xffffu);
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] |= (q == k) ? gg : 0u;
    }
    *oa = out[0]; *ob = out[1]; *oc = out[2]; *od = out[3];
}

__global__ void __launch_bounds__(256)
maxpool2_bwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ gy, bf16_t* __restrict__ gx, int h, int w,
                    int c8, long long total) {
    const int ho = h / 2, wo = w / 2;
    const long long row = (long long)w * c8;
    const uint4 zero = uint4{0u, 0u, 0u, 0u};
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int cg = (int)(e % c8);
        long long r = e / c8;
        const int ow = (int)(r % wo);
        r /= wo;
        const long long img = r / ho;
        const int oh = (int)(r - img * ho);
        const long long base = (img * h + 2 * oh) * row + (long long)(2 * ow) * c8 + cg;
        const uint4* src = reinterpret_cast<const uint4*>(x) + base;
        uint4* dst = reinterpret_cast<uint4*>(gx) + base;
        const uint4 a = src[0], b = src[c8], c = src[row], d = src[row + c8], g = reinterpret_cast<const uint4*>(gy)[e];
        uint4 oa, ob, oc, od;
        route_pair(a.x, b.x, c.x, d.x, g.x, &oa.x, &ob.x, &oc.x, &od.x);
        route_pair(a.y, b.y, c.y, d.y, g.y, &oa.y, &ob.y, &oc.y, &od.y);
        route_pair(a.z, b.z, c.z, d.z, g.z, &oa.z, &ob.z, &oc.z, &od.z);
        route_pair(a.w, b.w, c.w, d.w, g.w, &oa.w, &ob.w, &oc.w, &od.w);
        dst[0] = oa;
        dst[c8] = ob;
        dst[row] = oc;
        dst[row + c8] = od;
        // an odd last column / row belongs to no window: its gradient is zero, written by the window beside it
        const bool edge_w = (w & 1) && ow == wo - 1, edge_h = (h & 1) && oh == ho - 1;
        if (edge_w) {
            dst[2 * c8] = zero;
            dst[row + 2 * c8] = zero;
        }
        if (edge_h) {
            dst[2 * row] = zero;
            dst[2 * row + c8] = zero;
            if (edge_w) dst[2 * row + 2 * c8] = zero;
        }
    }
}

extern "C" int ctsi_maxpool2_bwd(const void* x, const void* gy, void* gx, int n, int h, int w, int c, void* stream) {
    CTSI_CHECK_ARG(x && gy && gx && n > 0 && h >= 2 && w >= 2 && c > 0 && c % 8 == 0,
                   "ctsi_maxpool2_bwd: bad arguments (n=%d h=%d w=%d c=%d; h, w at least 2, c a multiple of 8)", n, h, w, c);
    const long long total = (long long)n * (h / 2) * (w / 2) * (c / 8);
    hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (const bf16_t*)gy, (bf16_t*)gx, h, w, c / 8, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- in-place ReLU ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t relu_pair(uint32_t u) {
    return ((u & 0x8000u) ? 0u : (u & 0xffffu)) | ((u & 0x80000000u) ? 0u : (u & 0xffff0000u));
}
__global__ void __launch_bounds__(256) relu_bf16_kernel(bf16_t* __restrict__ x, long long units) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < units; e += (long long)gridDim.x * 256) {
        uint4 v = reinterpret_cast<uint4*>(x)[e];
        v.x = relu_pair(v.x); v.y = relu_pair(v.y); v.z = relu_pair(v.z); v.w = relu_pair(v.w);
        reinterpret_cast<uint4*>(x)[e] = v;
    }
}
extern "C" int ctsi_relu_bf16(void* x, long long count, void* stream) {
    CTSI_CHECK_ARG(x && count > 0 && count % 8 == 0, "ctsi_relu_bf16: bad arguments (count=%lld, a positive multiple of 8)", count);
    hipLaunchKernelGGL(relu_bf16_kernel, dim3(grid_for(count / 8)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, count / 8);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- feature distance -------------------------------------------------------------------------------------------------------
// Stage 1: CTSI_FEAT_LOSS_BLOCKS blocks, each over a fixed strided share of the 8-element units, write one fp64 partial sum
// each (0 for a block without work); stage 2 (ctsi_feat_loss_finalize) adds them in a fixed tree.  Nothing depends on the
// order in which blocks run.
#define FEAT_BLOCKS 256
extern "C" int ctsi_feat_loss_blocks() { return FEAT_BLOCKS; }

__device__ __forceinline__ float dist_pair(uint32_t p, uint32_t t, bool sq) {
    const float a = bf_lo(p) - bf_lo(t), b = bf_hi(p) - bf_hi(t);
    return sq ? __builtin_fmaf(b, b, a * a) : __builtin_fabsf(a) + __builtin_fabsf(b);
}

__global__ void __launch_bounds__(256)
feat_loss_kernel(const bf16_t* __restrict__ p, const bf16_t* __restrict__ t, long long units, int sq, double* __restrict__ partials) {
    __shared__ double s_part[4];
    double acc = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < units; e += (long long)FEAT_BLOCKS * 256) {
        const uint4 a = reinterpret_cast<const uint4*>(p)[e], b = reinterpret_cast<const uint4*>(t)[e];
        const float s = (dist_pair(a.x, b.x, sq) + dist_pair(a.y, b.y, sq)) + (dist_pair(a.z, b.z, sq) + dist_pair(a.w, b.w, sq));
        acc += (double)s;
    }
    const double total = block_sum_256(acc, s_part);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

extern "C" int ctsi_feat_loss_fwd(const void* pred, const void* target, long long count, int squared, double* partials,
                                  void* stream) {
    CTSI_CHECK_ARG(pred && target && partials && count > 0 && count % 8 == 0,
                   "ctsi_feat_loss_fwd: bad arguments (count=%lld, a positive multiple of 8)", count);
    hipLaunchKernelGGL(feat_loss_kernel, dim3(FEAT_BLOCKS), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)pred,
                       (const bf16_t*)target, count / 8, squared ? 1 : 0, partials);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// out[1 + l] = mean of layer l = (sum of its FEAT_BLOCKS partials) / counts[l]; out[0] = the average of the layer means
__global__ void __launch_bounds__(256)
feat_loss_finalize_kernel(const double* __restrict__ partials, const long long* __restrict__ counts, int layers,
                          float* __restrict__ out) {
    __shared__ double s_part[4];
    double acc = 0.0;
    for (int l = 0; l < layers; ++l) {
        const double total = block_sum_256(partials[(long long)l * FEAT_BLOCKS + threadIdx.x], s_part);
        if (threadIdx.x == 0) {
            const double mean = total / (double)counts[l];
            out[1 + l] = (float)mean;
            acc += mean;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(acc / (double)layers);
}

extern "C" int ctsi_feat_loss_finalize(const double* partials, const long long* counts, int layers, float* out, void* stream) {
    CTSI_CHECK_ARG(partials && counts && out && layers > 0 && layers <= 64, "ctsi_feat_loss_finalize: bad arguments (layers=%d)", layers);
    hipLaunchKernelGGL(feat_loss_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, counts, layers, out);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- one pass per layer boundary of the backward ------------------------------------------------------------------------------
// g_out = (g_in + coef * grad_loss * dist'(y - t)) * [y > 0]: dist' = sign (kind 1) or 2 (y - t) (kind 2); kind 0: no loss
// term (t unused); g_in may be NULL (the deepest compared feature); relu 0: no mask.  y is the stored activation of the pred
// half (post-ReLU where the mask applies: no mask is stored).  g_out may alias g_in.
__device__ __forceinline__ uint32_t grad_pair(uint32_t g, uint32_t y, uint32_t t, float scale, int kind, int relu) {
    float v[2] = {bf_lo(g), bf_hi(g)};
    const float yy[2] = {bf_lo(y), bf_hi(y)}, tt[2] = {bf_lo(t), bf_hi(t)};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (kind) {
            const float df = yy[k] - tt[k];
            v[k] += kind == 1 ? (df > 0.0f ? scale : (df < 0.0f ? -scale : 0.0f)) : 2.0f * scale * df;
        }
        if (relu && !(yy[k] > 0.0f)) v[k] = 0.0f;
    }
    return pack_bf16x2(v[0], v[1]);
}

__global__ void __launch_bounds__(256)
feat_grad_relu_bwd_kernel(const bf16_t* __restrict__ g_in, const bf16_t* __restrict__ y, const bf16_t* __restrict__ t,
                          bf16_t* __restrict__ g_out, long long units, float coef, int kind, int relu,
                          const float* __restrict__ grad_loss) {
    const float scale = kind ? coef * grad_loss[0] : 0.0f;
    const uint4 zero = uint4{0u, 0u, 0u, 0u};
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < units; e += (long long)gridDim.x * 256) {
        const uint4 g = g_in ? reinterpret_cast<const uint4*>(g_in)[e] : zero;
        const uint4 a = reinterpret_cast<const uint4*>(y)[e];
        const uint4 b = kind ? reinterpret_cast<const uint4*>(t)[e] : zero;
        uint4 o;
        o.x = grad_pair(g.x, a.x, b.x, scale, kind, relu);
        o.y = grad_pair(g.y, a.y, b.y, scale, kind, relu);
        o.z = grad_pair(g.z, a.z, b.z, scale, kind, relu);
        o.w = grad_pair(g.w, a.w, b.w, scale, kind, relu);
        reinterpret_cast<uint4*>(g_out)[e] = o;
    }
}

extern "C" int ctsi_feat_grad_relu_bwd(const void* g_in, const void* y, const void* target, void* g_out, long long count,
                                       float coef, int kind, int relu, const float* grad_loss, void* stream) {
    CTSI_CHECK_ARG(y && g_out && count > 0 && count % 8 == 0 && kind >= 0 && kind <= 2 && (kind == 0 || (target && grad_loss)) &&
                       (kind != 0 || g_in),
                   "ctsi_feat_grad_relu_bwd: bad arguments (count=%lld kind=%d)", count, kind);
    hipLaunchKernelGGL(feat_grad_relu_bwd_kernel, dim3(grid_for(count / 8)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)g_in, (const bf16_t*)y, (const bf16_t*)target, (bf16_t*)g_out, count / 8, coef, kind,
                       relu ? 1 : 0, grad_loss);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
