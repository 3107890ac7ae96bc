// Ensemble statistics: per-voxel running mean and sum of squared deviations over the members of an
// ensemble of fp32 volumes, folded in one streaming pass per group of members, and the tables read from them.
//   accumulate   x [rows][count] fp32, state (mean, m2) [count] fp32 over the `seen` members before this call.  Per element
//                the state is read once (not at all when seen == 0), the sequential Welford recurrence runs over the rows in
//                order -- k = seen + r + 1, d = x - mean, mean += d / k, m2 += d (x - mean), each operation rounded on its
//                own (no contraction) -- and the state is written once.  The recurrence does not know where a call ends, so
//                any split of the members over calls gives the same bits.  Member 1 sets mean = x, m2 = 0.
//                HBM streaming: a capped grid with a grid-stride loop over vectors of V = 4, 2 or 1 floats -- the widest
//                that x, every row of x, mean and m2 are all aligned to after the same number of scalar head elements --
//                with the head and tail elements (at most 2 (V - 1)) taken by the first threads of block 0.
//   finalize     std = sqrt(max(m2, 0) / (members - unbiased)) into a buffer of its own (the state stays valid), and per plane
//                of `plane` voxels the fp64 sum of std, sum of std^2 and max of std.
//   calibration  per plane the fp64 sum of (mean - target)^2, the sum of std^2 and the counts of |mean - target| <= std and
//                <= 2 std, all decided in fp64 on the fp32 values (differences and doublings of fp32 values are exact there).
// The two tables go through fixed_reduce.h: one block owns ENS_CHUNK consecutive voxels of one plane and writes one slot of
// partials (std >= 0, so 0 is the identity of the maximum too); a second launch, one block per plane, folds the plane's slots.
// No atomics, every slot written by exactly one block: the same bits on every run.
#include "fixed_reduce.h"
#include <limits.h>

namespace {

constexpr int ENS_THREADS = 256;
constexpr int ENS_MAX_BLOCKS = 2048;         // accumulate: 256 CUs x 8 blocks, the rest by the grid-stride loop
constexpr int ENS_CHUNK = 4096;              // tables: voxels of one plane per block (four 16-byte loads per thread)
constexpr int ENS_SLOT = 4;                  // doubles per partial slot (finalize fills three)

template <int V>
struct alignas(4 * V) Pack {
    float v[V];
};

__device__ __forceinline__ void welford(float x, float kf, float& mean, float& m2) {
#pragma clang fp contract(off)
    const float d = x - mean;
    mean = mean + d / kf;
    m2 = m2 + d * (x - mean);
}

template <int V, bool FIRST>
__global__ void __launch_bounds__(ENS_THREADS)
ensemble_accumulate_kernel(const float* __restrict__ x, int rows, long long count, int seen, float* __restrict__ mean,
                           float* __restrict__ m2, int head, long long nvec, int tail) {
    // scalar head and tail elements: [0, head) and [head + nvec V, count)
    if (blockIdx.x == 0 && (int)threadIdx.x < head + tail) {
        const int t = threadIdx.x;
        const long long e = t < head ? (long long)t : (long long)head + nvec * V + (t - head);
        float mu, s;
        int r = 0;
        if (FIRST) {
            mu = x[e], s = 0.0f, r = 1;
        } else {
            mu = mean[e], s = m2[e];
        }
        for (; r < rows; ++r) welford(x[(long long)r * count + e], (float)(seen + r + 1), mu, s);
        mean[e] = mu, m2[e] = s;
    }
    using P = Pack<V>;
    const float* xb = x + head;
    P* mv = reinterpret_cast<P*>(mean + head);
    P* sv = reinterpret_cast<P*>(m2 + head);
    const long long stride = (long long)gridDim.x * ENS_THREADS;
    for (long long i = (long long)blockIdx.x * ENS_THREADS + threadIdx.x; i < nvec; i += stride) {
        P mu, s;
        int r = 0;
        if (FIRST) {
            mu = *reinterpret_cast<const P*>(xb + i * V);
#pragma unroll
            for (int j = 0; j < V; ++j) s.v[j] = 0.0f;
            r = 1;
        } else {
            mu = mv[i], s = sv[i];
        }
        // four rows' loads are issued before the first use: the recurrence is a dependent chain, the loads are not
        for (; r + 4 <= rows; r += 4) {
            P t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = *reinterpret_cast<const P*>(xb + (long long)(r + u) * count + i * V);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float kf = (float)(seen + r + u + 1);
#pragma unroll
                for (int j = 0; j < V; ++j) welford(t[u].v[j], kf, mu.v[j], s.v[j]);
            }
        }
        for (; r < rows; ++r) {
            const P t = *reinterpret_cast<const P*>(xb + (long long)r * count + i * V);
            const float kf = (float)(seen + r + 1);
#pragma unroll
            for (int j = 0; j < V; ++j) welford(t.v[j], kf, mu.v[j], s.v[j]);
        }
        mv[i] = mu, sv[i] = s;
    }
}

template <int V>
void accumulate_launch(const float* x, int rows, long long count, int seen, float* mean, float* m2, int head, void* stream) {
    if ((long long)head > count) head = (int)count;
    const long long nvec = (count - head) / V;
    const int tail = (int)(count - head - nvec * V);
    long long blocks = (nvec + ENS_THREADS - 1) / ENS_THREADS;
    blocks = blocks < 1 ? 1 : (blocks > ENS_MAX_BLOCKS ? ENS_MAX_BLOCKS : blocks);
    if (seen == 0)
        hipLaunchKernelGGL((ensemble_accumulate_kernel<V, true>), dim3((unsigned)blocks), dim3(ENS_THREADS), 0,
                           (hipStream_t)stream, x, rows, count, seen, mean, m2, head, nvec, tail);
    else
        hipLaunchKernelGGL((ensemble_accumulate_kernel<V, false>), dim3((unsigned)blocks), dim3(ENS_THREADS), 0,
                           (hipStream_t)stream, x, rows, count, seen, mean, m2, head, nvec, tail);
}

__device__ __forceinline__ float std_of(float m2, float denom) {
#pragma clang fp contract(off)
    if (denom <= 0.0f) return 0.0f;                // one member
    const float c = m2 < 0.0f ? 0.0f : m2;         // (a NaN stays a NaN)
    return sqrtf(c / denom);
}

__device__ __forceinline__ void std_stats(float s, double* v) {
    const double d = (double)s;
    v[0] += d;
    v[1] = fma(d, d, v[1]);
    v[2] = d > v[2] ? d : v[2];
}

// grid planes * slots_pp: block b owns voxels [slot ENS_CHUNK, ...) of plane b / slots_pp
template <bool VEC>
__global__ void __launch_bounds__(ENS_THREADS)
ensemble_finalize_kernel(const float* __restrict__ m2, float* __restrict__ sd, float denom, long long plane, int slots_pp,
                         double* __restrict__ partials) {
    __shared__ double red[3 * FR_WAVES];
    const int slot = blockIdx.x % slots_pp;
    const long long p0 = (long long)slot * ENS_CHUNK;
    const long long base = (long long)(blockIdx.x / slots_pp) * plane + p0;
    const int n = plane - p0 < ENS_CHUNK ? (int)(plane - p0) : ENS_CHUNK;
    double v[3] = {0.0, 0.0, 0.0};
    if (VEC) {                                      // plane % 4 == 0: n is a multiple of 4
        float4 t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = (u * ENS_THREADS + threadIdx.x) * 4;
            if (j < n) t[u] = *reinterpret_cast<const float4*>(m2 + base + j);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = (u * ENS_THREADS + threadIdx.x) * 4;
            if (j < n) {
                const float4 o = make_float4(std_of(t[u].x, denom), std_of(t[u].y, denom), std_of(t[u].z, denom),
                                             std_of(t[u].w, denom));
                *reinterpret_cast<float4*>(sd + base + j) = o;
                std_stats(o.x, v), std_stats(o.y, v), std_stats(o.z, v), std_stats(o.w, v);
            }
        }
    } else {
        for (int j = threadIdx.x; j < n; j += ENS_THREADS) {
            const float o = std_of(m2[base + j], denom);
            sd[base + j] = o;
            std_stats(o, v);
        }
    }
    block_reduce<3, 0x4u>(v, red);
    if (threadIdx.x == 0) {
        double* out = partials + (long long)blockIdx.x * ENS_SLOT;
        out[0] = v[0], out[1] = v[1], out[2] = v[2];
    }
}

__device__ __forceinline__ void calibration_stats(float mean, float sd, float target, double* v) {
    const double e = (double)mean - (double)target, s = (double)sd;
    const double a = e < 0.0 ? -e : e;
    v[0] = fma(e, e, v[0]);
    v[1] = fma(s, s, v[1]);
    if (a <= s) v[2] += 1.0;
    if (a <= 2.0 * s) v[3] += 1.0;
}

template <bool VEC>
__global__ void __launch_bounds__(ENS_THREADS)
ensemble_calibration_kernel(const float* __restrict__ mean, const float* __restrict__ sd, const float* __restrict__ target,
                            long long plane, int slots_pp, double* __restrict__ partials) {
    __shared__ double red[4 * FR_WAVES];
    const int slot = blockIdx.x % slots_pp;
    const long long p0 = (long long)slot * ENS_CHUNK;
    const long long base = (long long)(blockIdx.x / slots_pp) * plane + p0;
    const int n = plane - p0 < ENS_CHUNK ? (int)(plane - p0) : ENS_CHUNK;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (VEC) {
        float4 a[4], b[4], c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = (u * ENS_THREADS + threadIdx.x) * 4;
            if (j < n) {
                a[u] = *reinterpret_cast<const float4*>(mean + base + j);
                b[u] = *reinterpret_cast<const float4*>(sd + base + j);
                c[u] = *reinterpret_cast<const float4*>(target + base + j);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = (u * ENS_THREADS + threadIdx.x) * 4;
            if (j < n) {
                calibration_stats(a[u].x, b[u].x, c[u].x, v), calibration_stats(a[u].y, b[u].y, c[u].y, v);
                calibration_stats(a[u].z, b[u].z, c[u].z, v), calibration_stats(a[u].w, b[u].w, c[u].w, v);
            }
        }
    } else {
        for (int j = threadIdx.x; j < n; j += ENS_THREADS) calibration_stats(mean[base + j], sd[base + j], target[base + j], v);
    }
    block_reduce<4, 0x0u>(v, red);
    if (threadIdx.x == 0) {
        double* out = partials + (long long)blockIdx.x * ENS_SLOT;
        out[0] = v[0], out[1] = v[1], out[2] = v[2], out[3] = v[3];
    }
}

inline long long slots_per_plane(long long plane) { return (plane + ENS_CHUNK - 1) / ENS_CHUNK; }

}  // namespace

extern "C" int ctsi_ensemble_accumulate(const float* x, int rows, long long count, int seen, float* mean, float* m2,
                                        void* stream) {
    CTSI_CHECK_ARG(x && mean && m2, "ctsi_ensemble_accumulate: null argument");
    CTSI_CHECK_ARG(rows >= 1 && count >= 1 && seen >= 0, "ctsi_ensemble_accumulate: bad sizes rows=%d count=%lld seen=%d", rows,
                   count, seen);
    CTSI_CHECK_ARG((long long)seen + rows <= (long long)INT_MAX,
                   "ctsi_ensemble_accumulate: seen=%d + rows=%d exceeds INT_MAX", seen, rows);
    CTSI_CHECK_ARG(count <= LLONG_MAX / 4 / rows, "ctsi_ensemble_accumulate: rows=%d x count=%lld overflows", rows, count);
    CTSI_CHECK_ARG(aligned_to(x, 4) && aligned_to(mean, 4) && aligned_to(m2, 4),
                   "ctsi_ensemble_accumulate: pointers must be 4-byte aligned: x=%p mean=%p m2=%p", (const void*)x,
                   (const void*)mean, (const void*)m2);
    // the widest vector that x, its rows, mean and m2 all reach after the same number of head elements
    const auto fits = [&](unsigned bytes) {
        const uintptr_t a = (uintptr_t)mean & (bytes - 1);
        return ((uintptr_t)m2 & (bytes - 1)) == a && ((uintptr_t)x & (bytes - 1)) == a && (rows == 1 || count % (bytes / 4) == 0);
    };
    const auto head_of = [&](unsigned bytes) { return (int)(((bytes - ((uintptr_t)mean & (bytes - 1))) & (bytes - 1)) / 4); };
    if (fits(16))
        accumulate_launch<4>(x, rows, count, seen, mean, m2, head_of(16), stream);
    else if (fits(8))
        accumulate_launch<2>(x, rows, count, seen, mean, m2, head_of(8), stream);
    else
        accumulate_launch<1>(x, rows, count, seen, mean, m2, 0, stream);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_ensemble_blocks(int planes, long long plane) {
    if (planes < 1 || plane < 1) return 0;
    const long long spp = slots_per_plane(plane);
    if (spp > INT_MAX / planes) return 0;
    return (int)(spp * planes);
}

#define ENS_CHECK_PLANES(fn, planes, plane)                                                                       \
    CTSI_CHECK_ARG((planes) >= 1 && (plane) >= 1, fn ": bad sizes planes=%d plane=%lld", (planes), (plane));      \
    CTSI_CHECK_ARG(ctsi_ensemble_blocks((planes), (plane)) > 0, fn ": planes=%d plane=%lld give too many blocks", \
                   (planes), (plane))

extern "C" int ctsi_ensemble_finalize(const float* m2, float* std_out, int members, int unbiased, int planes,
                                      long long plane, double* partials, double* stats, void* stream) {
    CTSI_CHECK_ARG(m2 && std_out && partials && stats, "ctsi_ensemble_finalize: null argument");
    CTSI_CHECK_ARG(members >= 1, "ctsi_ensemble_finalize: members=%d must be >= 1", members);
    ENS_CHECK_PLANES("ctsi_ensemble_finalize", planes, plane);
    CTSI_CHECK_ARG(aligned_to(m2, 4) && aligned_to(std_out, 4),
                   "ctsi_ensemble_finalize: pointers must be 4-byte aligned: m2=%p std=%p", (const void*)m2, (const void*)std_out);
    const int spp = (int)slots_per_plane(plane);
    const unsigned blocks = (unsigned)ctsi_ensemble_blocks(planes, plane);
    const float denom = members == 1 ? 0.0f : (float)(members - (unbiased ? 1 : 0));
    if (plane % 4 == 0 && aligned_to(m2, 16) && aligned_to(std_out, 16))
        hipLaunchKernelGGL((ensemble_finalize_kernel<true>), dim3(blocks), dim3(ENS_THREADS), 0, (hipStream_t)stream, m2,
                           std_out, denom, plane, spp, partials);
    else
        hipLaunchKernelGGL((ensemble_finalize_kernel<false>), dim3(blocks), dim3(ENS_THREADS), 0, (hipStream_t)stream, m2,
                           std_out, denom, plane, spp, partials);
    CTSI_LAUNCH_CHECK();
    hipLaunchKernelGGL((fold_slots_kernel<3, 0x4u>), dim3((unsigned)planes), dim3(FR_THREADS), 0, (hipStream_t)stream,
                       partials, stats, (long long)spp, ENS_SLOT);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_ensemble_calibration(const float* mean, const float* std_in, const float* target, int planes,
                                         long long plane, double* partials, double* stats, void* stream) {
    CTSI_CHECK_ARG(mean && std_in && target && partials && stats, "ctsi_ensemble_calibration: null argument");
    ENS_CHECK_PLANES("ctsi_ensemble_calibration", planes, plane);
    CTSI_CHECK_ARG(aligned_to(mean, 4) && aligned_to(std_in, 4) && aligned_to(target, 4),
                   "ctsi_ensemble_calibration: pointers must be 4-byte aligned: mean=%p std=%p target=%p", (const void*)mean,
                   (const void*)std_in, (const void*)target);
    const int spp = (int)slots_per_plane(plane);
    const unsigned blocks = (unsigned)ctsi_ensemble_blocks(planes, plane);
    if (plane % 4 == 0 && aligned_to(mean, 16) && aligned_to(std_in, 16) && aligned_to(target, 16))
        hipLaunchKernelGGL((ensemble_calibration_kernel<true>), dim3(blocks), dim3(ENS_THREADS), 0, (hipStream_t)stream, mean,
                           std_in, target, plane, spp, partials);
    else
        hipLaunchKernelGGL((ensemble_calibration_kernel<false>), dim3(blocks), dim3(ENS_THREADS), 0, (hipStream_t)stream, mean,
                           std_in, target, plane, spp, partials);
    CTSI_LAUNCH_CHECK();
    hipLaunchKernelGGL((fold_slots_kernel<4, 0x0u>), dim3((unsigned)planes), dim3(FR_THREADS), 0, (hipStream_t)stream,
                       partials, stats, (long long)spp, ENS_SLOT);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
