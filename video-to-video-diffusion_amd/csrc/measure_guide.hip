// Measurement guidance: the three device passes a guided sampler evaluation adds around the decoder tape.
//   ctsi_guide_z0            the predicted clean latent of the evaluation, from the state the update read and the prediction it
//                            used: fp32 NDHWC in, fp32 NCDHW out (the layout vae.decode_with_grad takes)
//   ctsi_depth_residual_adj  g_x = -W^T (y - W x) and per-sample sum r^2 in one pass over the decoded volume x
//   ctsi_guide_apply         z += c_b g_z (and the data-prediction history, and the bf16 U-Net input slice), c_b from the
//                            per-sample sum r^2 in device memory
// ctsi_depth_residual_adj is the one with structure, written against the column-tile frame (depth_tile.h): the tile in LDS is
// xs[d_out][TILE], rs[d_in][TILE] (y first, then the residual in its place), so x is read from HBM once and g_x written once;
// measure -> subtract -> measure_adj would be three passes and a y-sized temporary.  The waves split the k rows in the residual
// phase and the j rows in the adjoint phase (a register sum over the rows k whose band holds j, their range found once per
// block).  Sums run over the band supports only, ascending, one fma per term.  sum r^2: the residual re-evaluated in fp64 from
// the fp32 values in LDS (products of two fp32 are exact in fp64; ascending over the band), reduced per block into the slots of
// ctsi_depth_project_blocks and folded per sample in the fixed order of fixed_reduce.h.
#include "depth_tile.h"

namespace {

constexpr int MG_MAX_BLOCKS = 2048;          // streaming passes: 256 CUs x 8 blocks of 256 threads

// the column tile, the residual rows and the adjoint's [d_out][2] row table
inline size_t residual_lds(int d_in, int d_out, int tile) {
    return (size_t)(d_out + d_in) * tile * sizeof(float) + (size_t)d_out * 2 * sizeof(int);
}

struct ResidualArgs {
    const float* x;
    const float* y;
    const float* W;
    const int* band;
    float* gx;
    double* partials;
    int d_in, d_out, hw;
    int tiles_pp, slots_pp;       // tiles and partial slots per plane
};

template <int TILE, bool VEC>
__global__ void __launch_bounds__(DT_THREADS)
depth_residual_adj_kernel(const ResidualArgs a) {
    extern __shared__ __align__(16) float mg_lds[];
    __shared__ double red[DT_WAVES];
    const DepthTile<TILE, VEC> t(a.tiles_pp, a.hw);
    constexpr int STRIDE = DepthTile<TILE, VEC>::STRIDE;
    float* xs = mg_lds;                          // [d_out][TILE]: x, then g_x in its place
    float* rs = xs + a.d_out * TILE;             // [d_in][TILE]:  y, then r in its place
    int* kb = reinterpret_cast<int*>(rs + a.d_in * TILE);      // [d_out][2]: the first / last row k whose band holds column j
    const float* xg = a.x + t.plane * a.d_out * (long long)a.hw + t.p0;
    const float* yg = a.y + t.plane * a.d_in * (long long)a.hw + t.p0;
    float* gg = a.gx + t.plane * a.d_out * (long long)a.hw + t.p0;

    // the adjoint's table, from the band table of W: column j is read by the rows kb[j][0] .. kb[j][1] ((0, -1): by none)
    for (int j = threadIdx.x; j < a.d_out; j += DT_THREADS) {
        int klo = 0, khi = -1;
        for (int k = a.d_in - 1; k >= 0; --k)
            if (j >= a.band[2 * k] && j <= a.band[2 * k + 1]) {
                klo = k;
                khi = khi < 0 ? k : khi;
            }
        kb[2 * j] = klo, kb[2 * j + 1] = khi;
    }
    t.stage_rows(xs, xg, yg, a.d_out, a.d_in, a.hw);
    __syncthreads();

    const int pos = t.pos(), row0 = t.row0();
    const bool live = pos < t.valid;

    // residual: rs[k] = y[k] - sum_j W[k][j] xs[j] in fp32 (what the adjoint reads), and the same sum in fp64 for sum r^2
    double sum = 0.0;
    for (int k = row0; k < a.d_in; k += STRIDE) {
        int lo, hi;
        band_of(a.band, k, a.d_out, lo, hi);
        const float* wk = a.W + (long long)k * a.d_out;
        float acc = 0.0f;
        double acc64 = 0.0;
        for (int j = lo; j <= hi; ++j) {
            const float w = wk[j], v = xs[j * TILE + pos];
            acc = fmaf(w, v, acc);
            acc64 = fma((double)w, (double)v, acc64);
        }
        const float yv = rs[k * TILE + pos];
        rs[k * TILE + pos] = yv - acc;
        if (live) {
            const double r = (double)yv - acc64;
            sum = fma(r, r, sum);
        }
    }
    __syncthreads();

    // adjoint: xs[j] = -sum_k W[k][j] rs[k] over the rows kb[j] found above, ascending, in a register: one LDS read per term.
    // W[k][j] is 0 for a row of the range whose band does not hold j (a profile whose bands are not monotone), an exact no-op.
    // (Row j of xs is read by nobody any more: the residual phase is over.)
    for (int j = row0; j < a.d_out; j += STRIDE) {
        const int klo = kb[2 * j], khi = kb[2 * j + 1];
        const float* wj = a.W + j;
        float acc = 0.0f;
        for (int k = klo; k <= khi; ++k) acc = fmaf(wj[(long long)k * a.d_out], rs[k * TILE + pos], acc);
        xs[j * TILE + pos] = -acc;
    }
    __syncthreads();

    t.store_rows(gg, xs, a.d_out, a.hw);
    block_reduce<1, 0u>(&sum, red);
    if (threadIdx.x == 0) t.template write_slot<1>(a.partials, a.slots_pp, &sum);
}

struct ResidualKernel {
    template <int TILE, bool VEC>
    static auto get() { return depth_residual_adj_kernel<TILE, VEC>; }
};

// ---- z0 ------------------------------------------------------------------------------------------------------------------
struct Z0Row {
    float alpha, sigma, clip;
    int mode;
};

__device__ __forceinline__ float z0_elem(float zt, float ep, const Z0Row& r) {
    ep = nan_to_num_f(ep);
    float x = r.mode == 0 ? (zt - r.sigma * ep) / r.alpha : fmaf(r.alpha, zt, -(r.sigma * ep));
    x = nan_to_num_f(x);
    if (r.clip > 0.0f) x = fminf(fmaxf(x, -r.clip), r.clip);
    return x;
}

// one voxel per thread and iteration, its channels four at a time (c % 4 == 0, 16-byte aligned inputs): a wave reads 64
// voxels' contiguous channels and its stores, `vox` apart per channel, are 64 consecutive floats each
__global__ void __launch_bounds__(256)
guide_z0_vec4_kernel(const float* __restrict__ zt, const float* __restrict__ eps, float* __restrict__ out, Z0Row r, int c,
                     long long vox, long long nvox) {
    for (long long nv = (long long)blockIdx.x * 256 + threadIdx.x; nv < nvox; nv += (long long)gridDim.x * 256) {
        const long long nb = nv / vox, v = nv - nb * vox;
        float* op = out + nb * c * vox + v;
        for (int ch = 0; ch < c; ch += 4) {
            const float4 z4 = *reinterpret_cast<const float4*>(zt + nv * c + ch);
            const float4 e4 = *reinterpret_cast<const float4*>(eps + nv * c + ch);
            op[ch * vox] = z0_elem(z4.x, e4.x, r);
            op[(ch + 1) * vox] = z0_elem(z4.y, e4.y, r);
            op[(ch + 2) * vox] = z0_elem(z4.z, e4.z, r);
            op[(ch + 3) * vox] = z0_elem(z4.w, e4.w, r);
        }
    }
}

__global__ void __launch_bounds__(256)
guide_z0_scalar_kernel(const float* __restrict__ zt, const float* __restrict__ eps, float* __restrict__ out, Z0Row r, int c,
                       long long vox, long long total) {
    // one output element per thread, in NCDHW order (coalesced stores; the loads are c floats apart)
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long long)gridDim.x * 256) {
        const long long v = o % vox, nc = o / vox;
        const long long nb = nc / c;
        const int ch = (int)(nc - nb * c);
        const long long e = (nb * vox + v) * c + ch;
        out[o] = z0_elem(zt[e], eps[e], r);
    }
}

// ---- apply ---------------------------------------------------------------------------------------------------------------
struct ApplyArgs {
    float* z;
    float* hist;
    const float* g;
    const double* sumsq;
    bf16_t* zin;
    float coef_z, coef_hist;
    int normalize, c, c_total, c_off;
    long long vox;
};

// the per-sample factors {c_z, c_hist}; false: the sample is left as it is (sum r^2 == 0, or not finite)
__device__ __forceinline__ bool apply_factors(const ApplyArgs& a, long long nb, float& cz, float& ch) {
    double s = 1.0;
    if (a.normalize) {
        const double q = a.sumsq[nb];
        if (!(q > 0.0) || q == __builtin_inf()) return false;
        s = 1.0 / sqrt(q);
    }
    cz = (float)((double)a.coef_z * s);
    ch = (float)((double)a.coef_hist * s);
    return true;
}

// one voxel per thread and iteration, its channels four at a time (as guide_z0_vec4_kernel: the g_z loads coalesce across the
// wave's voxels, the NDHWC side is contiguous per lane)
__global__ void __launch_bounds__(256)
guide_apply_vec4_kernel(const ApplyArgs a, long long nvox) {
    for (long long nv = (long long)blockIdx.x * 256 + threadIdx.x; nv < nvox; nv += (long long)gridDim.x * 256) {
        const long long nb = nv / a.vox, v = nv - nb * a.vox;
        float cz, ch;
        const bool on = apply_factors(a, nb, cz, ch);
        const float* gp = a.g + nb * a.c * a.vox + v;
        for (int c0 = 0; c0 < a.c; c0 += 4) {
            const long long e = nv * a.c + c0;
            const float4 z4 = *reinterpret_cast<const float4*>(a.z + e);
            float zz[4] = {z4.x, z4.y, z4.z, z4.w};
            if (on) {
                float gv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) gv[j] = gp[(c0 + j) * a.vox];
#pragma unroll
                for (int j = 0; j < 4; ++j) zz[j] = nan_to_num_f(fmaf(cz, gv[j], zz[j]));
                *reinterpret_cast<float4*>(a.z + e) = make_float4(zz[0], zz[1], zz[2], zz[3]);
                if (a.hist) {
                    float4 h4 = *reinterpret_cast<const float4*>(a.hist + e);
                    h4.x = nan_to_num_f(fmaf(ch, gv[0], h4.x));
                    h4.y = nan_to_num_f(fmaf(ch, gv[1], h4.y));
                    h4.z = nan_to_num_f(fmaf(ch, gv[2], h4.z));
                    h4.w = nan_to_num_f(fmaf(ch, gv[3], h4.w));
                    *reinterpret_cast<float4*>(a.hist + e) = h4;
                }
            }
            if (a.zin) {
                uint2 pk;
                pk.x = pack_bf16x2(zz[0], zz[1]);
                pk.y = pack_bf16x2(zz[2], zz[3]);
                *reinterpret_cast<uint2*>(a.zin + nv * a.c_total + a.c_off + c0) = pk;
            }
        }
    }
}

__global__ void __launch_bounds__(256)
guide_apply_scalar_kernel(const ApplyArgs a, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long nv = e / a.c;
        const int ch_i = (int)(e - nv * a.c);
        const long long nb = nv / a.vox, v = nv - nb * a.vox;
        float zz = a.z[e];
        float cz, ch;
        if (apply_factors(a, nb, cz, ch)) {
            const float gv = a.g[(nb * a.c + ch_i) * a.vox + v];
            zz = nan_to_num_f(fmaf(cz, gv, zz));
            a.z[e] = zz;
            if (a.hist) a.hist[e] = nan_to_num_f(fmaf(ch, gv, a.hist[e]));
        }
        if (a.zin) a.zin[nv * a.c_total + a.c_off + ch_i] = f32_to_bf16(zz);
    }
}

inline unsigned stream_blocks(long long work) {
    long long blocks = (work + 255) / 256;
    return (unsigned)(blocks > MG_MAX_BLOCKS ? MG_MAX_BLOCKS : blocks);
}

}  // namespace

extern "C" int ctsi_guide_z0(const float* z_t, const float* eps, float alpha, float sigma, int mode, float clip, float* z0_out,
                             int n, int c, int d, int h, int w, void* stream) {
    CTSI_CHECK_ARG(z_t && eps && z0_out, "ctsi_guide_z0: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_guide_z0: bad shape n=%d c=%d d=%d h=%d w=%d", n, c, d, h,
                   w);
    CTSI_CHECK_ARG(mode == 0 || mode == 1, "ctsi_guide_z0: mode=%d must be 0 (eps form) or 1 (x0 form)", mode);
    CTSI_CHECK_ARG(mode == 1 || alpha != 0.0f, "ctsi_guide_z0: alpha=0 has no eps form (mode 0 divides by it)");
    CTSI_CHECK_ARG(clip >= 0.0f, "ctsi_guide_z0: clip=%g must be >= 0 (0: no clip)", (double)clip);
    const long long vox = (long long)d * h * w, total = (long long)n * c * vox;
    const Z0Row r = {alpha, sigma, clip, mode};
    if ((c % 4) == 0 && aligned16(z_t) && aligned16(eps))
        hipLaunchKernelGGL(guide_z0_vec4_kernel, dim3(stream_blocks(n * vox)), dim3(256), 0, (hipStream_t)stream, z_t, eps,
                           z0_out, r, c, vox, n * vox);
    else
        hipLaunchKernelGGL(guide_z0_scalar_kernel, dim3(stream_blocks(total)), dim3(256), 0, (hipStream_t)stream, z_t, eps,
                           z0_out, r, c, vox, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_depth_residual_adj(const float* x, const float* y, const float* W, const int* band, float* g_x,
                                       double* partials, double* sumsq, int n, int c, int d_in, int d_out, int hw,
                                       void* stream) {
    CTSI_CHECK_ARG(x && y && W && band && g_x && partials && sumsq, "ctsi_depth_residual_adj: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d_in > 0 && d_out > 0 && hw > 0,
                   "ctsi_depth_residual_adj: bad sizes n=%d c=%d d_in=%d d_out=%d hw=%d", n, c, d_in, d_out, hw);
    DT_CHECK_DEPTHS("ctsi_depth_residual_adj", d_in, d_out);
    const long long planes = (long long)n * c;
    const int tile = tile_for(residual_lds(d_in, d_out, 64));
    const int tiles_pp = ceil_div(hw, tile);
    const long long blocks = planes * tiles_pp, slots = planes * slots_per_plane(hw);
    CTSI_CHECK_ARG(blocks < (1ll << 31) && slots < (1ll << 31), "ctsi_depth_residual_adj: n=%d c=%d hw=%d give too many tiles", n,
                   c, hw);
    const ResidualArgs a = {x, y, W, band, g_x, partials, d_in, d_out, hw, tiles_pp, slots_per_plane(hw)};
    const bool vec = (hw % 4) == 0 && aligned16(x) && aligned16(y) && aligned16(g_x);
    launch_tiled<ResidualKernel>(a, tile, vec, blocks, residual_lds(d_in, d_out, tile), stream);
    CTSI_LAUNCH_CHECK();
    // one block per sample folds the slots of the sample's c planes
    hipLaunchKernelGGL((fold_slots_kernel<1, 0u>), dim3((unsigned)n), dim3(FR_THREADS), 0, (hipStream_t)stream, partials, sumsq,
                       (long long)c * slots_per_plane(hw), 1);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_guide_apply(float* z, float* hist, const float* g_z, const double* sumsq, float coef_z, float coef_hist,
                                int normalize, void* zin, int c_total, int c_off, int n, int c, int d, int h, int w,
                                void* stream) {
    CTSI_CHECK_ARG(z && g_z, "ctsi_guide_apply: null argument");
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_guide_apply: bad shape n=%d c=%d d=%d h=%d w=%d", n, c, d,
                   h, w);
    CTSI_CHECK_ARG(normalize == 0 || normalize == 1, "ctsi_guide_apply: normalize=%d must be 0 or 1", normalize);
    CTSI_CHECK_ARG(!normalize || sumsq, "ctsi_guide_apply: normalize=1 needs the per-sample sum r^2 (null argument)");
    CTSI_CHECK_ARG(!zin || (c_off >= 0 && c_off + c <= c_total), "ctsi_guide_apply: bad channel slice c_off=%d c=%d c_total=%d",
                   c_off, c, c_total);
    const long long vox = (long long)d * h * w, total = (long long)n * c * vox;
    const ApplyArgs a = {z, hist, g_z, sumsq, (bf16_t*)zin, coef_z, coef_hist, normalize, c, c_total, c_off, vox};
    const bool vec = (c % 4) == 0 && aligned16(z) && aligned16(hist) &&
                     (!zin || ((c_total | c_off) % 4 == 0 && ((uintptr_t)zin & 7) == 0));
    if (vec)
        hipLaunchKernelGGL(guide_apply_vec4_kernel, dim3(stream_blocks(n * vox)), dim3(256), 0, (hipStream_t)stream, a, n * vox);
    else
        hipLaunchKernelGGL(guide_apply_scalar_kernel, dim3(stream_blocks(total)), dim3(256), 0, (hipStream_t)stream, a, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
