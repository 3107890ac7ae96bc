// The LPIPS perceptual distance (lpips 0.1.x, net = 'vgg') around the VGG-16 stack that vgg_loss.hip and
// the planar (1, 3, 3) conv plans already run: the scaling-layer input transform and its backward, the per-tap distance
// sum_c w_c (y_c / (|y| + eps) - t_c / (|t| + eps))^2 with its fixed-order per-image reduction, and the one pass per tap of the
// backward (the derivative through the unit normalisation + the ReLU mask).  A ROW is the C channels of one position of a bf16
// channels-last image [image][h][w][c]: C / 8 lanes of one 16-byte load each (8, 16, 32 or 64 lanes), reduced with cross-lane
// operations inside the wave.  All arithmetic is fp32, the partial sums fp64.  Every entry takes plain pointers and sizes,
// allocates nothing, keeps no state and is capture-safe; no float atomics anywhere, so results are bit-stable.
#include "feat_common.h"

#define LPIPS_BLOCKS 512        // partial sums per (tap, image): enough blocks to fill the device from ONE image
#define LPIPS_EPS 1e-10f
static_assert(LPIPS_BLOCKS == 512, "lpips_finalize_kernel adds two partial sums per thread");
extern "C" int ctsi_lpips_blocks() { return LPIPS_BLOCKS; }

// ---- scaling layer -------------------------------------------------------------------------------------------------------
// image n of x (fp32 NCHW, C = 1: the grey value in all three channels) -> 8-channel bf16: (v - shift_c) / scale_c for c < 3,
// channels 3-7 zero; normalize: v = 2 x - 1 first
__constant__ float LPIPS_SHIFT[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float LPIPS_SCALE[3] = {0.458f, 0.448f, 0.450f};

__global__ void __launch_bounds__(256)
lpips_prep_kernel(const float* __restrict__ x, bf16_t* __restrict__ dst, int c, int normalize, long long hw, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long img = e / hw, pix = e - img * hw;
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float s = x[(img * c + (c == 3 ? k : 0)) * hw + pix];
            v[k] = ((normalize ? 2.0f * s - 1.0f : s) - LPIPS_SHIFT[k]) / LPIPS_SCALE[k];
        }
        uint4 pk;
        pk.x = pack_bf16x2(v[0], v[1]);
        pk.y = pack_bf16x2(v[2], 0.0f);
        pk.z = 0u;
        pk.w = 0u;
        *reinterpret_cast<uint4*>(dst + e * 8) = pk;
    }
}

extern "C" int ctsi_lpips_prep(const float* x, void* dst, int n, int c, int h, int w, int normalize, void* stream) {
    CTSI_CHECK_ARG(x && dst && n > 0 && (c == 1 || c == 3) && h > 0 && w > 0,
                   "ctsi_lpips_prep: bad arguments (n=%d c=%d h=%d w=%d; c is 1 or 3)", n, c, h, w);
    const long long hw = (long long)h * w, total = hw * n;
    hipLaunchKernelGGL(lpips_prep_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)dst, c,
                       normalize ? 1 : 0, hw, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// grad[n, c] = k g_c / scale_c (k = 2 with normalize); C = 1: the sum of the three
__global__ void __launch_bounds__(256)
lpips_prep_bwd_kernel(const bf16_t* __restrict__ g, float* __restrict__ grad, int c, int normalize, long long hw, long long total) {
    const float k = normalize ? 2.0f : 1.0f;
    const float r0 = k / LPIPS_SCALE[0], r1 = k / LPIPS_SCALE[1], r2 = k / LPIPS_SCALE[2];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long img = e / hw, pix = e - img * hw;
        const uint2 pk = *reinterpret_cast<const uint2*>(g + e * 8);
        const float g0 = bf_lo(pk.x) * r0, g1 = bf_hi(pk.x) * r1, g2 = bf_lo(pk.y) * r2;
        if (c == 3) {
            float* o = grad + img * 3 * hw + pix;
            o[0] = g0;
            o[hw] = g1;
            o[2 * hw] = g2;
        } else {
            grad[e] = g0 + g1 + g2;
        }
    }
}

extern "C" int ctsi_lpips_prep_bwd(const void* g, float* grad, int n, int c, int h, int w, int normalize, void* stream) {
    CTSI_CHECK_ARG(g && grad && n > 0 && (c == 1 || c == 3) && h > 0 && w > 0,
                   "ctsi_lpips_prep_bwd: bad arguments (n=%d c=%d h=%d w=%d; c is 1 or 3)", n, c, h, w);
    const long long hw = (long long)h * w, total = hw * n;
    hipLaunchKernelGGL(lpips_prep_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)g, grad,
                       c, normalize ? 1 : 0, hw, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- rows ----------------------------------------------------------------------------------------------------------------
// the sum of one value per lane over the LANES lanes of a row, the same bits in every lane (an xor butterfly below LANES
// never leaves the row's aligned lane group)
template <int LANES>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
    for (int off = LANES / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ void unpack8(uint4 u, float* f) {
    f[0] = bf_lo(u.x); f[1] = bf_hi(u.x); f[2] = bf_lo(u.y); f[3] = bf_hi(u.y);
    f[4] = bf_lo(u.z); f[5] = bf_hi(u.z); f[6] = bf_lo(u.w); f[7] = bf_hi(u.w);
}
__device__ __forceinline__ float sumsq8(const float* f) {
    float s = f[0] * f[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) s = __builtin_fmaf(f[k], f[k], s);
    return s;
}
static bool lpips_row_ok(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

// ---- distance of one tap ----------------------------------------------------------------------------------------------------
// grid (LPIPS_BLOCKS, images); a block takes ROWS = 256 / LANES rows per round, rounds strided by LPIPS_BLOCKS.  Every lane of
// the block walks the same number of rounds (a row past the end loads zeros and adds 0), so the cross-lane sums never meet an
// inactive lane.  partials[image][block] <- the block's fp64 sum of sum_c w_c (u_c - v_c)^2 (0 for a block without rows).
template <int LANES>
__global__ void __launch_bounds__(256)
lpips_dist_kernel(const bf16_t* __restrict__ y, const bf16_t* __restrict__ t, const float* __restrict__ w, long long positions,
                  double* __restrict__ partials) {
#pragma clang fp contract(off)      // u - v must be exactly 0 where y == t: no fma may see one unrounded product (the sums are explicit fmas)
    __shared__ double s_part[4];
    constexpr int ROWS = 256 / LANES;
    const int lane = threadIdx.x % LANES, sub = threadIdx.x / LANES;
    const long long base = (long long)blockIdx.y * positions * LANES + lane;      // in 16-byte units
    const uint4* yp = reinterpret_cast<const uint4*>(y) + base;
    const uint4* tp = reinterpret_cast<const uint4*>(t) + base;
    float wv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wv[k] = w[lane * 8 + k];
    const uint4 zero = uint4{0u, 0u, 0u, 0u};
    double acc = 0.0;
    for (long long r0 = (long long)blockIdx.x * ROWS; r0 < positions; r0 += (long long)LPIPS_BLOCKS * ROWS) {
        const long long r = r0 + sub;
        const bool ok = r < positions;
        float yy[8], tt[8];
        unpack8(ok ? yp[r * LANES] : zero, yy);
        unpack8(ok ? tp[r * LANES] : zero, tt);
        const float sy = row_sum<LANES>(sumsq8(yy)), st = row_sum<LANES>(sumsq8(tt));
        const float ia = 1.0f / (__builtin_sqrtf(sy) + LPIPS_EPS), ib = 1.0f / (__builtin_sqrtf(st) + LPIPS_EPS);
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float d = yy[k] * ia - tt[k] * ib;
            s = __builtin_fmaf(wv[k] * d, d, s);
        }
        acc += (double)s;          // the rest of the row's sum is taken in fp64 by the block sum below
    }
    const double total = block_sum_256(acc, s_part);
    if (threadIdx.x == 0) partials[(long long)blockIdx.y * LPIPS_BLOCKS + blockIdx.x] = total;
}

extern "C" int ctsi_lpips_dist_fwd(const void* y, const void* target, const float* w, int images, long long positions, int c,
                                   double* partials, void* stream) {
    CTSI_CHECK_ARG(y && target && w && partials && images > 0 && images <= 65535 && positions > 0 && c > 0 && c % 8 == 0 &&
                       lpips_row_ok(c),
                   "ctsi_lpips_dist_fwd: bad arguments (images=%d positions=%lld c=%d; c is 64, 128, 256 or 512)", images,
                   positions, c);
    const dim3 grid(LPIPS_BLOCKS, images), block(256);
    const bf16_t *yp = (const bf16_t*)y, *tp = (const bf16_t*)target;
    hipStream_t s = (hipStream_t)stream;
    switch (c / 8) {
    case 8: hipLaunchKernelGGL(lpips_dist_kernel<8>, grid, block, 0, s, yp, tp, w, positions, partials); break;
    case 16: hipLaunchKernelGGL(lpips_dist_kernel<16>, grid, block, 0, s, yp, tp, w, positions, partials); break;
    case 32: hipLaunchKernelGGL(lpips_dist_kernel<32>, grid, block, 0, s, yp, tp, w, positions, partials); break;
    default: hipLaunchKernelGGL(lpips_dist_kernel<64>, grid, block, 0, s, yp, tp, w, positions, partials); break;
    }
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// partials: [tap][image][LPIPS_BLOCKS].  out[i] = sum over taps of (image i's sum) / positions[tap]; tap_means[tap] = the mean
// of that quotient over the images.  One block; every sum in a fixed order.
__global__ void __launch_bounds__(256)
lpips_finalize_kernel(const double* __restrict__ partials, const long long* __restrict__ positions, int taps, int images,
                      float* __restrict__ out, float* __restrict__ tap_means) {
    __shared__ double s_part[4];
    __shared__ double s_tap[16];
    if (threadIdx.x < 16) s_tap[threadIdx.x] = 0.0;
    __syncthreads();
    for (int i = 0; i < images; ++i) {
        double acc = 0.0;
        for (int l = 0; l < taps; ++l) {
            const double* p = partials + ((long long)l * images + i) * LPIPS_BLOCKS + threadIdx.x;
            const double v = p[0] + p[256];
            const double total = block_sum_256(v, s_part);
            if (threadIdx.x == 0) {
                const double d = total / (double)positions[l];
                acc += d;
                s_tap[l] += d;
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) out[i] = (float)acc;
    }
    if (threadIdx.x < taps) tap_means[threadIdx.x] = (float)(s_tap[threadIdx.x] / (double)images);
}

extern "C" int ctsi_lpips_finalize(const double* partials, const long long* positions, int taps, int images, float* out,
                                   float* tap_means, void* stream) {
    CTSI_CHECK_ARG(partials && positions && out && tap_means && taps > 0 && taps <= 16 && images > 0,
                   "ctsi_lpips_finalize: bad arguments (taps=%d images=%d)", taps, images);
    hipLaunchKernelGGL(lpips_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, positions, taps, images, out,
                       tap_means);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- one pass per tap of the backward ----------------------------------------------------------------------------------------
// g_out = (g_in + grad_out[image] / positions * dy) * [y > 0] with r = 2 w (u - v) and
//     dy = r / (a + eps) - y (y . r) / (a (a + eps)^2) = r / (a + eps) - u (u . r) / a       (y = u (a + eps)),
// the second form bounded by |r| / a however small a is.  a = 0: every y of the row is 0 and the mask writes exact zeros (an
// assignment, not a product: nothing non-finite survives it).  1 / (a + eps) and 1 / (b + eps) are recomputed from the rows
// this pass loads anyway; nothing is stored by the forward.  g_in may be NULL; g_out may alias g_in (a lane reads its own 16
// bytes before it writes them).
template <int LANES>
__global__ void __launch_bounds__(256)
lpips_grad_kernel(const bf16_t* g_in, const bf16_t* __restrict__ y, const bf16_t* __restrict__ t, const float* __restrict__ w,
                  bf16_t* g_out, long long positions, float inv_positions, const float* __restrict__ grad_out) {
#pragma clang fp contract(off)      // as in the forward: identical inputs give an exactly zero gradient
    constexpr int ROWS = 256 / LANES;
    const int lane = threadIdx.x % LANES, sub = threadIdx.x / LANES;
    const long long base = (long long)blockIdx.y * positions * LANES + lane;
    const uint4* yp = reinterpret_cast<const uint4*>(y) + base;
    const uint4* tp = reinterpret_cast<const uint4*>(t) + base;
    const uint4* gp = g_in ? reinterpret_cast<const uint4*>(g_in) + base : nullptr;
    uint4* op = reinterpret_cast<uint4*>(g_out) + base;
    float w2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w2[k] = 2.0f * w[lane * 8 + k];
    const float scale = grad_out[blockIdx.y] * inv_positions;
    const uint4 zero = uint4{0u, 0u, 0u, 0u};
    for (long long r0 = (long long)blockIdx.x * ROWS; r0 < positions; r0 += (long long)gridDim.x * ROWS) {
        const long long r = r0 + sub;
        const bool ok = r < positions;
        float yy[8], tt[8], gg[8], uu[8], rr[8];
        unpack8(ok ? yp[r * LANES] : zero, yy);
        unpack8(ok ? tp[r * LANES] : zero, tt);
        unpack8(ok && gp ? gp[r * LANES] : zero, gg);
        const float sy = row_sum<LANES>(sumsq8(yy)), st = row_sum<LANES>(sumsq8(tt));
        const float a = __builtin_sqrtf(sy);
        const float ia = 1.0f / (a + LPIPS_EPS), ib = 1.0f / (__builtin_sqrtf(st) + LPIPS_EPS);
        float ur = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            uu[k] = yy[k] * ia;
            rr[k] = w2[k] * (uu[k] - tt[k] * ib);
            ur = __builtin_fmaf(uu[k], rr[k], ur);
        }
        ur = row_sum<LANES>(ur);
        const float proj = a > 0.0f ? ur / a : 0.0f;
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float dy = rr[k] * ia - uu[k] * proj;
            o[k] = yy[k] > 0.0f ? gg[k] + scale * dy : 0.0f;
        }
        if (ok) op[r * LANES] = uint4{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
    }
}

extern "C" int ctsi_lpips_grad_relu_bwd(const void* g_in, const void* y, const void* target, const float* w, void* g_out,
                                        int images, long long positions, int c, const float* grad_out, void* stream) {
    CTSI_CHECK_ARG(y && target && w && g_out && grad_out && images > 0 && images <= 65535 && positions > 0 && c > 0 &&
                       c % 8 == 0 && lpips_row_ok(c),
                   "ctsi_lpips_grad_relu_bwd: bad arguments (images=%d positions=%lld c=%d; c is 64, 128, 256 or 512)", images,
                   positions, c);
    const int lanes = c / 8, rows = 256 / lanes;
    long long bx = (positions + rows - 1) / rows;
    const long long cap = images >= 8192 ? 1 : 8192 / images;
    if (bx > cap) bx = cap;
    const dim3 grid((unsigned)bx, images), block(256);
    const bf16_t *gp = (const bf16_t*)g_in, *yp = (const bf16_t*)y, *tp = (const bf16_t*)target;
    bf16_t* op = (bf16_t*)g_out;
    const float inv = 1.0f / (float)positions;
    hipStream_t s = (hipStream_t)stream;
    switch (lanes) {
    case 8: hipLaunchKernelGGL(lpips_grad_kernel<8>, grid, block, 0, s, gp, yp, tp, w, op, positions, inv, grad_out); break;
    case 16: hipLaunchKernelGGL(lpips_grad_kernel<16>, grid, block, 0, s, gp, yp, tp, w, op, positions, inv, grad_out); break;
    case 32: hipLaunchKernelGGL(lpips_grad_kernel<32>, grid, block, 0, s, gp, yp, tp, w, op, positions, inv, grad_out); break;
    default: hipLaunchKernelGGL(lpips_grad_kernel<64>, grid, block, 0, s, gp, yp, tp, w, op, positions, inv, grad_out); break;
    }
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
