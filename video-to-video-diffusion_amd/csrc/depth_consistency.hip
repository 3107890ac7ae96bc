// Data consistency along depth: the slice-profile operator y = W x of a thin volume x, its adjoint, and
// the projection x <- x + P (y - W x), P = W^T (W W^T)^-1, onto the volumes that reproduce the acquired thick slices y.
// All tensors are fp32 NCDHW contiguous; a "column" is the depth vector at one (plane = n c, position = h w).
//   W      [d_in][d_out] fp32, rows sum to 1          band_w [d_in][2]  first / last non-zero column of each row of W
//   P      [d_out][d_in] fp32                         band_p [d_out][2] first / last non-zero column of each row of P
// measure / measure_adj stream: one thread per output element (four with 16-byte accesses), the band of W bounds the sum.
// project is the hot kernel, written against the column-tile frame (depth_tile.h): the tile in LDS is xs[d_out][TILE],
// ys[d_in][TILE], rs[d_in][TILE], so x is read from HBM once and written once whatever `iters` is.  The waves split the k rows
// in the residual phase and the j rows in the update phase.  Sums run over the band supports only, ascending, one fma per term.
// Statistics (partials != NULL): the residual of the input and of the output, re-evaluated in fp64 from the fp32 values the
// kernel holds (products of two fp32 are exact in fp64; the sum runs ascending over the band), reduced per block and folded per
// plane by ctsi_depth_project_finalize in the fixed order of fixed_reduce.h.
#include "depth_tile.h"

namespace {

// the column tile, its copy of y and the residual rows
inline size_t project_lds(int d_in, int d_out, int tile) { return (size_t)(d_out + 2 * d_in) * tile * sizeof(float); }

// ---- measure: y[plane][k][p] = sum_j W[k][j] x[plane][j][p] --------------------------------------------------------
// grid (ceil(hw / (256 V)), d_in, planes)
template <int V>
__global__ void __launch_bounds__(256)
depth_measure_kernel(const float* __restrict__ x, const float* __restrict__ W, const int* __restrict__ band,
                     float* __restrict__ y, int d_in, int d_out, int hw) {
    const int k = blockIdx.y;
    const long long plane = blockIdx.z;
    const int p = (blockIdx.x * 256 + threadIdx.x) * V;
    if (p >= hw) return;
    int lo, hi;
    band_of(band, k, d_out, lo, hi);
    const float* xp = x + plane * d_out * (long long)hw + p;
    const float* wk = W + (long long)k * d_out;
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0f;
    for (int j = lo; j <= hi; ++j) {
        const float w = wk[j];
        if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(xp + (long long)j * hw);
            acc[0] = fmaf(w, t.x, acc[0]);
            acc[1] = fmaf(w, t.y, acc[1]);
            acc[2] = fmaf(w, t.z, acc[2]);
            acc[3] = fmaf(w, t.w, acc[3]);
        } else {
            acc[0] = fmaf(w, xp[(long long)j * hw], acc[0]);
        }
    }
    float* yp = y + (plane * d_in + k) * (long long)hw + p;
    if constexpr (V == 4)
        *reinterpret_cast<float4*>(yp) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else
        yp[0] = acc[0];
}

// ---- adjoint: g_x[plane][j][p] (+)= scale sum_k W[k][j] g_y[plane][k][p] ---------------------------------------------
// grid (ceil(hw / (256 V)), d_out, planes); row k takes part when j lies inside its band (a block-uniform test)
template <int V>
__global__ void __launch_bounds__(256)
depth_measure_adj_kernel(const float* __restrict__ gy, const float* __restrict__ W, const int* __restrict__ band,
                         float* __restrict__ gx, float scale, int accumulate, int d_in, int d_out, int hw) {
    const int j = blockIdx.y;
    const long long plane = blockIdx.z;
    const int p = (blockIdx.x * 256 + threadIdx.x) * V;
    if (p >= hw) return;
    const float* gp = gy + plane * d_in * (long long)hw + p;
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0f;
    for (int k = 0; k < d_in; ++k) {
        if (j < band[2 * k] || j > band[2 * k + 1]) continue;
        const float w = W[(long long)k * d_out + j];
        if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(gp + (long long)k * hw);
            acc[0] = fmaf(w, t.x, acc[0]);
            acc[1] = fmaf(w, t.y, acc[1]);
            acc[2] = fmaf(w, t.z, acc[2]);
            acc[3] = fmaf(w, t.w, acc[3]);
        } else {
            acc[0] = fmaf(w, gp[(long long)k * hw], acc[0]);
        }
    }
    float* xp = gx + (plane * d_out + j) * (long long)hw + p;
    if constexpr (V == 4) {
        float4 o = make_float4(scale * acc[0], scale * acc[1], scale * acc[2], scale * acc[3]);
        if (accumulate) {
            const float4 t = *reinterpret_cast<const float4*>(xp);
            o.x += t.x, o.y += t.y, o.z += t.z, o.w += t.w;
        }
        *reinterpret_cast<float4*>(xp) = o;
    } else {
        const float o = scale * acc[0];
        xp[0] = accumulate ? xp[0] + o : o;
    }
}

// ---- project -----------------------------------------------------------------------------------------------------------
struct ProjectArgs {
    float* x;
    const float* y;
    const float* W;
    const float* P;
    const int* band_w;
    const int* band_p;
    double* partials;
    int iters, clamp_mode;
    float lo, hi;
    int d_in, d_out, hw;
    int tiles_pp, slots_pp;       // tiles and partial slots per plane
};

// fp64 residual of the tile in LDS: thread-local sum of r^2 and max |r| over this thread's (row, position) pairs.  `live`
// is false for a position past the plane's end: its staged zeros may have been clamped to a bound that excludes 0
template <int TILE>
__device__ __forceinline__ void residual_stats(const float* xs, const float* ys, const ProjectArgs& a, int row0, int pos,
                                               bool live, double& sum, double& mx) {
    if (!live) return;
    constexpr int STRIDE = DT_WAVES * (64 / TILE);
    for (int k = row0; k < a.d_in; k += STRIDE) {
        int lo, hi;
        band_of(a.band_w, k, a.d_out, lo, hi);
        const float* wk = a.W + (long long)k * a.d_out;
        double acc = 0.0;
        for (int j = lo; j <= hi; ++j) acc = fma((double)wk[j], (double)xs[j * TILE + pos], acc);
        const double r = (double)ys[k * TILE + pos] - acc;
        sum = fma(r, r, sum);
        const double m = r < 0.0 ? -r : r;
        mx = m > mx ? m : mx;
    }
}

// the five statistics: sums for 0, 1, 4, maxima for 2, 3
constexpr unsigned DC_STAT_MAX = 0b01100;

template <int TILE, bool VEC>
__global__ void __launch_bounds__(DT_THREADS)
depth_project_kernel(const ProjectArgs a) {
    extern __shared__ __align__(16) float dc_lds[];
    __shared__ double red[5 * DT_WAVES];
    const DepthTile<TILE, VEC> t(a.tiles_pp, a.hw);
    constexpr int STRIDE = DepthTile<TILE, VEC>::STRIDE;
    float* xs = dc_lds;                          // [d_out][TILE]
    float* ys = xs + a.d_out * TILE;             // [d_in][TILE]
    float* rs = ys + a.d_in * TILE;              // [d_in][TILE]
    float* xg = a.x + t.plane * a.d_out * (long long)a.hw + t.p0;
    const float* yg = a.y + t.plane * a.d_in * (long long)a.hw + t.p0;
    t.stage_rows(xs, xg, yg, a.d_out, a.d_in, a.hw);
    __syncthreads();

    const int pos = t.pos(), row0 = t.row0();
    const bool stats = a.partials != nullptr;
    double st[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (stats) residual_stats<TILE>(xs, ys, a, row0, pos, pos < t.valid, st[0], st[2]);

    for (int it = 0; it < a.iters; ++it) {
        // residual: rs[k] = ys[k] - sum_j W[k][j] xs[j]
        for (int k = row0; k < a.d_in; k += STRIDE) {
            int lo, hi;
            band_of(a.band_w, k, a.d_out, lo, hi);
            const float* wk = a.W + (long long)k * a.d_out;
            float acc = 0.0f;
            for (int j = lo; j <= hi; ++j) acc = fmaf(wk[j], xs[j * TILE + pos], acc);
            rs[k * TILE + pos] = ys[k * TILE + pos] - acc;
        }
        __syncthreads();
        // update: xs[j] += sum_k P[j][k] rs[k], then the clamp between iterations (and after the last one in mode 2)
        const bool clamp = a.clamp_mode != 0 && (it + 1 < a.iters || a.clamp_mode == 2);
        for (int j = row0; j < a.d_out; j += STRIDE) {
            int lo, hi;
            band_of(a.band_p, j, a.d_in, lo, hi);
            const float* pj = a.P + (long long)j * a.d_in;
            float acc = 0.0f;
            for (int k = lo; k <= hi; ++k) acc = fmaf(pj[k], rs[k * TILE + pos], acc);
            float v = xs[j * TILE + pos] + acc;
            if (clamp) {
                const float c = fminf(fmaxf(v, a.lo), a.hi);
                if (c != v && pos < t.valid) st[4] += 1.0;
                v = c;
            }
            xs[j * TILE + pos] = v;
        }
        __syncthreads();
    }

    if (stats) residual_stats<TILE>(xs, ys, a, row0, pos, pos < t.valid, st[1], st[3]);
    t.store_rows(xg, xs, a.d_out, a.hw);
    if (stats) {
        block_reduce<5, DC_STAT_MAX>(st, red);
        if (threadIdx.x == 0) t.template write_slot<5>(a.partials, a.slots_pp, st);
    }
}

struct ProjectKernel {
    template <int TILE, bool VEC>
    static auto get() { return depth_project_kernel<TILE, VEC>; }
};

}  // namespace

extern "C" int ctsi_depth_measure(const float* x, const float* W, const int* band, float* y_out, int planes, int d_in,
                                  int d_out, int hw, void* stream) {
    CTSI_CHECK_ARG(x && W && band && y_out, "ctsi_depth_measure: null argument");
    CTSI_CHECK_ARG(planes > 0 && planes <= 65535 && d_in > 0 && d_out > 0 && hw > 0,
                   "ctsi_depth_measure: bad sizes planes=%d d_in=%d d_out=%d hw=%d", planes, d_in, d_out, hw);
    DT_CHECK_DEPTHS("ctsi_depth_measure", d_in, d_out);
    if ((hw % 4) == 0 && aligned16(x) && aligned16(y_out))
        hipLaunchKernelGGL((depth_measure_kernel<4>), dim3((unsigned)ceil_div(hw, 1024), (unsigned)d_in, (unsigned)planes),
                           dim3(256), 0, (hipStream_t)stream, x, W, band, y_out, d_in, d_out, hw);
    else
        hipLaunchKernelGGL((depth_measure_kernel<1>), dim3((unsigned)ceil_div(hw, 256), (unsigned)d_in, (unsigned)planes),
                           dim3(256), 0, (hipStream_t)stream, x, W, band, y_out, d_in, d_out, hw);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_depth_measure_adj(const float* g_y, const float* W, const int* band, float* g_x, float scale,
                                      int accumulate, int planes, int d_in, int d_out, int hw, void* stream) {
    CTSI_CHECK_ARG(g_y && W && band && g_x, "ctsi_depth_measure_adj: null argument");
    CTSI_CHECK_ARG(planes > 0 && planes <= 65535 && d_in > 0 && d_out > 0 && hw > 0,
                   "ctsi_depth_measure_adj: bad sizes planes=%d d_in=%d d_out=%d hw=%d", planes, d_in, d_out, hw);
    DT_CHECK_DEPTHS("ctsi_depth_measure_adj", d_in, d_out);
    if ((hw % 4) == 0 && aligned16(g_y) && aligned16(g_x))
        hipLaunchKernelGGL((depth_measure_adj_kernel<4>), dim3((unsigned)ceil_div(hw, 1024), (unsigned)d_out, (unsigned)planes),
                           dim3(256), 0, (hipStream_t)stream, g_y, W, band, g_x, scale, accumulate, d_in, d_out, hw);
    else
        hipLaunchKernelGGL((depth_measure_adj_kernel<1>), dim3((unsigned)ceil_div(hw, 256), (unsigned)d_out, (unsigned)planes),
                           dim3(256), 0, (hipStream_t)stream, g_y, W, band, g_x, scale, accumulate, d_in, d_out, hw);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_depth_project_blocks(int planes, int hw) {
    if (planes <= 0 || hw <= 0) return 0;
    const long long n = (long long)planes * slots_per_plane(hw);
    return n < (1ll << 31) ? (int)n : 0;
}

extern "C" int ctsi_depth_project(float* x, const float* y, const float* W, const float* P, const int* band_w,
                                  const int* band_p, int iters, float clamp_lo, float clamp_hi, int clamp_mode,
                                  double* partials, int planes, int d_in, int d_out, int hw, void* stream) {
    CTSI_CHECK_ARG(x && y && W && P && band_w && band_p, "ctsi_depth_project: null argument");
    CTSI_CHECK_ARG(planes > 0 && d_in > 0 && d_out > 0 && hw > 0,
                   "ctsi_depth_project: bad sizes planes=%d d_in=%d d_out=%d hw=%d", planes, d_in, d_out, hw);
    DT_CHECK_DEPTHS("ctsi_depth_project", d_in, d_out);
    CTSI_CHECK_ARG(iters >= 1, "ctsi_depth_project: iters=%d must be >= 1", iters);
    CTSI_CHECK_ARG(clamp_mode >= 0 && clamp_mode <= 2, "ctsi_depth_project: clamp_mode=%d must be 0, 1 or 2", clamp_mode);
    CTSI_CHECK_ARG(clamp_mode == 0 || clamp_lo <= clamp_hi, "ctsi_depth_project: clamp_lo=%g > clamp_hi=%g",
                   (double)clamp_lo, (double)clamp_hi);
    const int tile = tile_for(project_lds(d_in, d_out, 64));
    const int tiles_pp = ceil_div(hw, tile);
    const long long blocks = (long long)planes * tiles_pp;
    CTSI_CHECK_ARG(blocks < (1ll << 31) && ctsi_depth_project_blocks(planes, hw) > 0,
                   "ctsi_depth_project: planes=%d hw=%d give too many tiles", planes, hw);
    const ProjectArgs a = {x, y, W, P, band_w, band_p, partials, iters, clamp_mode, clamp_lo, clamp_hi,
                           d_in, d_out, hw, tiles_pp, slots_per_plane(hw)};
    const bool vec = (hw % 4) == 0 && aligned16(x) && aligned16(y);
    launch_tiled<ProjectKernel>(a, tile, vec, blocks, project_lds(d_in, d_out, tile), stream);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_depth_project_finalize(const double* partials, double* stats, int planes, int hw, int d_in,
                                           void* stream) {
    CTSI_CHECK_ARG(partials && stats, "ctsi_depth_project_finalize: null argument");
    CTSI_CHECK_ARG(planes > 0 && hw > 0 && d_in > 0 && ctsi_depth_project_blocks(planes, hw) > 0,
                   "ctsi_depth_project_finalize: bad sizes planes=%d hw=%d d_in=%d", planes, hw, d_in);
    CTSI_CHECK_ARG(d_in <= DT_MAX_D_IN, "ctsi_depth_project_finalize: d_in=%d exceeds the limit %d", d_in, DT_MAX_D_IN);
    hipLaunchKernelGGL((fold_slots_kernel<5, DC_STAT_MAX>), dim3((unsigned)planes), dim3(FR_THREADS), 0, (hipStream_t)stream,
                       partials, stats, (long long)slots_per_plane(hw), 5);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
