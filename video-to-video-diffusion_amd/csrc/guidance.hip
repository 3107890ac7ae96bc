// Classifier-free guidance on the sampler step graph.
// A guided U-Net evaluation runs the network at batch 2n: rows [0, n) see the conditioning, rows [n, 2n) the null
// conditioning (the all-zero latent).  Between the network and the unchanged sampler update:
//   combine   eps[b] <- m_b * (eps_u + s (eps_c - eps_u)),  eps_c = eps[b], eps_u = eps[n + b]     (in place, rows [0, n))
//             m_b = phi * std_b(eps_c) / std_b(eps_g) + (1 - phi)   (guidance rescale; 1 without the statistics pass)
//   stats     per-sample fp64 sums of eps_c, eps_c^2, eps_g, eps_g^2: block partials, then one block per sample adds them
//             in a fixed order (no atomics: the same bits on every run, as ctsi_grad_norm_multi / _finalize)
//   mirror    after the update: the new z of rows [0, n) of the network input copied to rows [n, 2n)
// {s, phi} is row *step_ptr of a device table, so one captured graph serves every scale.  All three stream once over the
// latent: HBM-bound, 16-byte accesses when the sizes allow, grid capped at 2048 blocks with a grid-stride loop.
#include "ctsi_internal.h"

namespace {

constexpr int CFG_MAX_BLOCKS = 2048;        // 256 CUs x 8 blocks of 256 threads
constexpr int CFG_STATS_MAX_BPS = 512;      // statistics blocks per sample
constexpr long long CFG_STATS_CHUNK = 4096; // ... at least this many elements each

inline bool aligned(const void* p, unsigned bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

__device__ __forceinline__ float guide(float c, float u, float s) { return fmaf(s, c - u, u); }

// the rescale factor of sample b (1 when the program holds no statistics pass or phi == 0)
__device__ __forceinline__ float rescale_factor(const double* stats, int b, float phi) {
    if (stats == nullptr || phi == 0.0f) return 1.0f;
    const double ratio = stats[b * 4 + 2];
    return (float)((double)phi * ratio + (1.0 - (double)phi));
}

// grid (x, n): sample blockIdx.y, 4 consecutive elements per thread and iteration (per_sample % 4 == 0)
__global__ void __launch_bounds__(256)
cfg_combine_vec4_kernel(float* __restrict__ eps, const float* __restrict__ scale, const int* __restrict__ step_ptr,
                        const double* __restrict__ stats, int n, long long per4) {
    const int step = step_ptr ? *step_ptr : 0;
    const float s = scale[step * 2], phi = scale[step * 2 + 1];
    const int b = blockIdx.y;
    const float m = rescale_factor(stats, b, phi);
    float4* pc = reinterpret_cast<float4*>(eps) + (long long)b * per4;
    const float4* pu = reinterpret_cast<const float4*>(eps) + (long long)(n + b) * per4;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < per4; q += (long long)gridDim.x * 256) {
        const float4 c = pc[q], u = pu[q];
        float4 g;
        g.x = guide(c.x, u.x, s) * m;
        g.y = guide(c.y, u.y, s) * m;
        g.z = guide(c.z, u.z, s) * m;
        g.w = guide(c.w, u.w, s) * m;
        pc[q] = g;
    }
}

// any size / alignment: one element per thread and iteration
__global__ void __launch_bounds__(256)
cfg_combine_scalar_kernel(float* __restrict__ eps, const float* __restrict__ scale, const int* __restrict__ step_ptr,
                          const double* __restrict__ stats, int n, long long per) {
    const int step = step_ptr ? *step_ptr : 0;
    const float s = scale[step * 2], phi = scale[step * 2 + 1];
    const int b = blockIdx.y;
    const float m = rescale_factor(stats, b, phi);
    float* pc = eps + (long long)b * per;
    const float* pu = eps + (long long)(n + b) * per;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long long)gridDim.x * 256)
        pc[e] = guide(pc[e], pu[e], s) * m;
}

// ---- statistics ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void acc_stats(float c, float u, double s, double* a) {
    const double dc = (double)c, du = (double)u;
    const double g = du + s * (dc - du);
    a[0] += dc;
    a[1] += dc * dc;
    a[2] += g;
    a[3] += g * g;
}

// every thread ends with the block's four sums (fixed shuffle tree, then the 4 wave sums in index order)
__device__ __forceinline__ void block_sum4_f64(double* a, double* red /* [4][4] in LDS */) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double s = a[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((threadIdx.x & 63) == 0) red[k * 4 + (threadIdx.x >> 6)] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = (red[k * 4] + red[k * 4 + 1]) + (red[k * 4 + 2] + red[k * 4 + 3]);
}

// grid (bps, n): block (x, b) strides over sample b; partials[(b * bps + x) * 4 ..] = its four sums
template <bool VEC>
__global__ void __launch_bounds__(256)
cfg_stats_kernel(const float* __restrict__ eps, const float* __restrict__ scale, const int* __restrict__ step_ptr,
                 double* __restrict__ partials, int n, long long per) {
    __shared__ double red[16];
    const int step = step_ptr ? *step_ptr : 0;
    const double s = (double)scale[step * 2];
    const int b = blockIdx.y;
    const float* pc = eps + (long long)b * per;
    const float* pu = eps + (long long)(n + b) * per;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (VEC) {
        const long long per4 = per >> 2;
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < per4; q += (long long)gridDim.x * 256) {
            const float4 c = reinterpret_cast<const float4*>(pc)[q], u = reinterpret_cast<const float4*>(pu)[q];
            acc_stats(c.x, u.x, s, a);
            acc_stats(c.y, u.y, s, a);
            acc_stats(c.z, u.z, s, a);
            acc_stats(c.w, u.w, s, a);
        }
    } else {
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long long)gridDim.x * 256)
            acc_stats(pc[e], pu[e], s, a);
    }
    block_sum4_f64(a, red);
    if (threadIdx.x == 0) {
        double* out = partials + ((long long)b * gridDim.x + blockIdx.x) * 4;
        out[0] = a[0], out[1] = a[1], out[2] = a[2], out[3] = a[3];
    }
}

// one block per sample: thread t adds its contiguous run of partials in index order, thread 0 the 256 runs in index order
__global__ void __launch_bounds__(256)
cfg_stats_finalize_kernel(const double* __restrict__ partials, double* __restrict__ stats, int bps, double count) {
    __shared__ double part[4][256];
    const int b = blockIdx.x;
    const double* p = partials + (long long)b * bps * 4;
    const int per = (bps + 255) / 256;
    const int i0 = threadIdx.x * per;
    const int i1 = i0 + per < bps ? i0 + per : bps;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = i0; i < i1; ++i)
        for (int k = 0; k < 4; ++k) a[k] += p[i * 4 + k];
    for (int k = 0; k < 4; ++k) part[k][threadIdx.x] = a[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < 256; ++i)
            for (int k = 0; k < 4; ++k) t[k] += part[k][i];
        // unbiased (torch.std's default); a rounding-negative variance reads as 0
        double vc = (t[1] - t[0] * t[0] / count) / (count - 1.0);
        double vg = (t[3] - t[2] * t[2] / count) / (count - 1.0);
        vc = vc < 0.0 ? 0.0 : vc;
        vg = vg < 0.0 ? 0.0 : vg;
        const double sc = sqrt(vc), sg = sqrt(vg);
        stats[b * 4 + 0] = sc;
        stats[b * 4 + 1] = sg;
        stats[b * 4 + 2] = sg == 0.0 ? 1.0 : sc / sg;
        stats[b * 4 + 3] = count;
    }
}

// ---- mirror ---------------------------------------------------------------------------------------------------------
// rows of `row_units` units at a pitch of `stride_units` units, copied from src to dst (same pitch)
template <typename U>
__global__ void __launch_bounds__(256)
cfg_mirror_kernel(const U* __restrict__ src, U* __restrict__ dst, long long total, int row_units, int stride_units) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / row_units;
        const long long o = r * stride_units + (i - r * row_units);
        dst[o] = src[o];
    }
}

template <typename U>
void mirror_launch(const void* src, void* dst, long long rows, int row_bytes, int stride_bytes, void* stream) {
    const int ru = row_bytes / (int)sizeof(U), su = stride_bytes / (int)sizeof(U);
    const long long total = rows * ru;
    long long blocks = (total + 255) / 256;
    if (blocks > CFG_MAX_BLOCKS) blocks = CFG_MAX_BLOCKS;
    hipLaunchKernelGGL((cfg_mirror_kernel<U>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const U*)src,
                       (U*)dst, total, ru, su);
}

inline long long per_sample_of(int c, int d, int h, int w) { return (long long)c * d * h * w; }

inline unsigned grid_x(long long work, int n) {
    long long blocks = (work + 255) / 256;
    const long long cap = CFG_MAX_BLOCKS / n > 0 ? CFG_MAX_BLOCKS / n : 1;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

extern "C" int ctsi_cfg_stats_blocks(long long per_sample) {
    if (per_sample <= 0) return 0;
    const long long b = (per_sample + CFG_STATS_CHUNK - 1) / CFG_STATS_CHUNK;
    return (int)(b > CFG_STATS_MAX_BPS ? CFG_STATS_MAX_BPS : b);
}

extern "C" int ctsi_cfg_combine(float* eps, const float* scale, const int* step_ptr, const double* stats, int n, int c,
                                int d, int h, int w, void* stream) {
    CTSI_CHECK_ARG(eps && scale, "ctsi_cfg_combine: null argument");
    CTSI_CHECK_ARG(n > 0 && n <= 32767 && c > 0 && d > 0 && h > 0 && w > 0,
                   "ctsi_cfg_combine: bad shape n=%d c=%d d=%d h=%d w=%d", n, c, d, h, w);
    const long long per = per_sample_of(c, d, h, w);
    if ((per % 4) == 0 && aligned(eps, 16))
        hipLaunchKernelGGL(cfg_combine_vec4_kernel, dim3(grid_x(per / 4, n), (unsigned)n), dim3(256), 0,
                           (hipStream_t)stream, eps, scale, step_ptr, stats, n, per / 4);
    else
        hipLaunchKernelGGL(cfg_combine_scalar_kernel, dim3(grid_x(per, n), (unsigned)n), dim3(256), 0,
                           (hipStream_t)stream, eps, scale, step_ptr, stats, n, per);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_cfg_stats(const float* eps, const float* scale, const int* step_ptr, double* partials, int n, int c,
                              int d, int h, int w, void* stream) {
    CTSI_CHECK_ARG(eps && scale && partials, "ctsi_cfg_stats: null argument");
    CTSI_CHECK_ARG(n > 0 && n <= 32767 && c > 0 && d > 0 && h > 0 && w > 0,
                   "ctsi_cfg_stats: bad shape n=%d c=%d d=%d h=%d w=%d", n, c, d, h, w);
    const long long per = per_sample_of(c, d, h, w);
    const dim3 grid((unsigned)ctsi_cfg_stats_blocks(per), (unsigned)n);
    if ((per % 4) == 0 && aligned(eps, 16))
        hipLaunchKernelGGL((cfg_stats_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, eps, scale, step_ptr,
                           partials, n, per);
    else
        hipLaunchKernelGGL((cfg_stats_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, eps, scale, step_ptr,
                           partials, n, per);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_cfg_stats_finalize(const double* partials, double* stats, int n, int c, int d, int h, int w,
                                       void* stream) {
    CTSI_CHECK_ARG(partials && stats, "ctsi_cfg_stats_finalize: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0,
                   "ctsi_cfg_stats_finalize: bad shape n=%d c=%d d=%d h=%d w=%d", n, c, d, h, w);
    const long long per = per_sample_of(c, d, h, w);
    hipLaunchKernelGGL(cfg_stats_finalize_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, partials, stats,
                       ctsi_cfg_stats_blocks(per), (double)per);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_cfg_mirror(const void* src, void* dst, long long rows, int row_bytes, int stride_bytes,
                               void* stream) {
    CTSI_CHECK_ARG(src && dst, "ctsi_cfg_mirror: null argument");
    CTSI_CHECK_ARG(rows >= 0 && row_bytes > 0 && stride_bytes >= row_bytes && (row_bytes % 2) == 0 &&
                       (stride_bytes % 2) == 0,
                   "ctsi_cfg_mirror: bad sizes rows=%lld row_bytes=%d stride_bytes=%d", rows, row_bytes, stride_bytes);
    CTSI_CHECK_ARG(aligned(src, 2) && aligned(dst, 2), "ctsi_cfg_mirror: pointers must be 2-byte aligned");
    if (rows == 0) return CTSI_OK;
    const int both = row_bytes | stride_bytes;
    if ((both % 16) == 0 && aligned(src, 16) && aligned(dst, 16))
        mirror_launch<uint4>(src, dst, rows, row_bytes, stride_bytes, stream);
    else if ((both % 4) == 0 && aligned(src, 4) && aligned(dst, 4))
        mirror_launch<uint32_t>(src, dst, rows, row_bytes, stride_bytes, stream);
    else
        mirror_launch<uint16_t>(src, dst, rows, row_bytes, stride_bytes, stream);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
