// Multi-planar and 3-D SSIM / PSNR tables of two fp32 (n, c, d, h, w) volumes.  One kernel, parameterised
// by a window-radius triple (Rd, Rh, Rw) and the axis whose indices the tables are kept for:
//   axial (0, R, R) per d      coronal (R, 0, R) per h      sagittal (R, R, 0) per w      volumetric (Rd, R, R) per d
// The volumes are read in place: a block owns a (TD, TH, TW) tile of outputs, loads the tile with its halo of a and b into LDS
// as w-contiguous rows (zeros outside the volume: "same" zero padding, the zeros count in the window, as ctsi_slice_metrics
// and avg_pool2d(padding = window / 2) have it), and takes the window of each moment field -- a, b, a^2, b^2, ab -- as three
// separable passes inside LDS, w then h then d, one field at a time: T1 [HD][HH][TW] after w, T2 [HD][TH][TW] after h, the d
// pass into registers.  A pass of radius 0 is skipped and the next one reads its source.  Weights: gd, gh, gw (2R + 1 floats
// each, normalised by the caller), or all three NULL for the box window, which adds the taps unweighted and scales the sums
// once by 1 / ((2Rd+1)(2Rh+1)(2Rw+1)) as slice_metrics_kernel does.  SSIM per voxel is slice_metrics_kernel's formula.
// Reduction (fixed_reduce.h, no atomics): for every index of `axis` that its tile covers a block writes one slot of four fp64
// values -- sum of squared differences, sum of SSIM, NaN count of a, NaN count of b -- and fold_slots_kernel adds the slots of
// an index in a fixed order: out[axis_len][4] holds SUMS over the index's slice; the same bits on every run.
// The block index is linear (no grid dimension caps d, h or w) and every global offset is 64-bit.
#include "fixed_reduce.h"
#include <limits.h>

namespace {

constexpr int VM_RMAX = 7;                   // largest radius (window 15)
constexpr int VM_TAPS = 2 * VM_RMAX + 1;
constexpr int VM_VPT = 4;                    // tile voxels per thread: tiles hold at most 4 * 256 voxels
constexpr int VM_LDS_MAX = 160 * 1024;

struct VmTile {
    int ltd, lth, ltw;                       // log2 of the tile edges
};

// The tile of a radius triple: flat along a direction the window does not extend in, so that a planar mode pays no halo
// there.  LDS at R = 7: 31 KB axial / coronal, 77 KB sagittal, 133 KB volumetric.
inline VmTile vm_tile(int rd, int rh, int rw) {
    if (rd == 0) return {0, 4, 6};           //  1 x 16 x 64
    if (rh == 0) return {4, 0, 6};           // 16 x  1 x 64
    if (rw == 0) return {3, 3, 4};           //  8 x  8 x 16
    return {2, 3, 4};                        //  4 x  8 x 16
}

struct VmArgs {
    const float* a;
    const float* b;
    const float* gd;                         // NULL (all three): box
    const float* gh;
    const float* gw;
    double* partial;
    int d, h, w;
    int rd, rh, rw;
    int ltd, lth, ltw;
    int tiles_d, tiles_h, tiles_w;
    int axis;
    float scale, c1, c2;
};

inline long long vm_lds_floats(const VmTile& t, int rd, int rh, int rw) {
    const long long TD = 1 << t.ltd, TH = 1 << t.lth, TW = 1 << t.ltw;
    const long long HD = TD + 2 * rd, HH = TH + 2 * rh, HWp = TW + 2 * rw + 1;
    return 2 * HD * HH * HWp + (rw > 0 ? HD * HH * TW : 0) + (rh > 0 ? HD * TH * TW : 0);
}

template <int F>
__device__ __forceinline__ float vm_field(float va, float vb) {
    return F == 0 ? va : F == 1 ? vb : F == 2 ? va * va : F == 3 ? vb * vb : va * vb;
}

// sum over `taps` weighted values `stride` apart from `base` on: of field F of the halo tiles (raw) or of a pass buffer
template <int F>
__device__ __forceinline__ float vm_taps(bool raw, const float* sa, const float* sb, const float* buf, int base, int stride,
                                         const float* g, int taps) {
    float acc = 0.0f;
    if (raw) {
        for (int i = 0; i < taps; ++i) {
            const float va = (F != 1 && F != 3) ? sa[base + i * stride] : 0.0f;
            const float vb = (F != 0 && F != 2) ? sb[base + i * stride] : 0.0f;
            acc = fmaf(g[i], vm_field<F>(va, vb), acc);
        }
    } else {
        for (int i = 0; i < taps; ++i) acc = fmaf(g[i], buf[base + i * stride], acc);
    }
    return acc;
}

// the three passes of one moment field; m[j] = the windowed field at tile voxel threadIdx.x + 256 j
template <int F>
__device__ __forceinline__ void vm_moment(const VmArgs& p, const float* sa, const float* sb, float* t1, float* t2,
                                          const float* sg, int HD, int HH, int HWp, float* m) {
    const int TW = 1 << p.ltw, TH = 1 << p.lth, vox = 1 << (p.ltd + p.lth + p.ltw);
    const bool w_on = p.rw > 0, h_on = p.rh > 0;
    if (w_on) {
        const int n = HD * HH * TW;
        for (int e = threadIdx.x; e < n; e += FR_THREADS) {
            const int x = e & (TW - 1), row = e >> p.ltw;
            t1[e] = vm_taps<F>(true, sa, sb, nullptr, row * HWp + x, 1, sg + 2 * VM_TAPS, 2 * p.rw + 1);
        }
        __syncthreads();
    }
    const int w1 = w_on ? TW : HWp;                    // row length of the h pass's source
    if (h_on) {
        const int n = HD * TH * TW;
        for (int e = threadIdx.x; e < n; e += FR_THREADS) {
            const int x = e & (TW - 1), y = (e >> p.ltw) & (TH - 1), zd = e >> (p.ltw + p.lth);
            t2[e] = vm_taps<F>(!w_on, sa, sb, t1, (zd * HH + y) * w1 + x, w1, sg + VM_TAPS, 2 * p.rh + 1);
        }
        __syncthreads();
    }
    const int w2 = h_on ? TW : w1;                     // the d pass's source has TH rows per plane either way
    const float* src = h_on ? t2 : t1;
#pragma unroll
    for (int j = 0; j < VM_VPT; ++j) {
        const int e = threadIdx.x + j * FR_THREADS;
        if (e < vox) {
            const int x = e & (TW - 1), y = (e >> p.ltw) & (TH - 1), z = e >> (p.ltw + p.lth);
            m[j] = vm_taps<F>(!w_on && !h_on, sa, sb, src, (z * TH + y) * w2 + x, TH * w2, sg, 2 * p.rd + 1);
        }
    }
    __syncthreads();                                   // the next field overwrites t1 / t2
}

__global__ void __launch_bounds__(FR_THREADS) volume_metrics_kernel(VmArgs p) {
    extern __shared__ float vm_lds[];
    __shared__ float sg[3 * VM_TAPS];                  // gd | gh | gw
    __shared__ double red[4 * FR_WAVES];
    const int TD = 1 << p.ltd, TH = 1 << p.lth, TW = 1 << p.ltw, vox = TD * TH * TW;
    const int HD = TD + 2 * p.rd, HH = TH + 2 * p.rh, HW = TW + 2 * p.rw, HWp = HW + 1;
    float* sa = vm_lds;
    float* sb = sa + HD * HH * HWp;
    float* t1 = sb + HD * HH * HWp;
    float* t2 = t1 + (p.rw > 0 ? HD * HH * TW : 0);

    // block -> (volume, tile): w tiles fastest
    long long blk = blockIdx.x;
    const int tw = (int)(blk % p.tiles_w); blk /= p.tiles_w;
    const int th = (int)(blk % p.tiles_h); blk /= p.tiles_h;
    const int td = (int)(blk % p.tiles_d); blk /= p.tiles_d;
    const long long vol = blk;                         // n * c index
    const int z0 = td << p.ltd, y0 = th << p.lth, x0 = tw << p.ltw;

    if (threadIdx.x < 3 * VM_TAPS) {
        const int k = threadIdx.x / VM_TAPS, i = threadIdx.x - k * VM_TAPS;
        const float* g = k == 0 ? p.gd : k == 1 ? p.gh : p.gw;
        const int taps = 2 * (k == 0 ? p.rd : k == 1 ? p.rh : p.rw) + 1;
        sg[threadIdx.x] = i < taps ? (g ? g[i] : 1.0f) : 0.0f;
    }
    const float* pa = p.a + vol * p.d * p.h * p.w;
    const float* pb = p.b + vol * p.d * p.h * p.w;
    const int nload = HD * HH * HW;
    for (int e = threadIdx.x; e < nload; e += FR_THREADS) {
        const int row = e / HW, col = e - row * HW;
        const int zd = row / HH, zh = row - zd * HH;
        const int z = z0 + zd - p.rd, y = y0 + zh - p.rh, x = x0 + col - p.rw;
        const bool in = z >= 0 && z < p.d && y >= 0 && y < p.h && x >= 0 && x < p.w;
        const long long off = ((long long)z * p.h + y) * p.w + x;
        sa[row * HWp + col] = in ? pa[off] : 0.0f;
        sb[row * HWp + col] = in ? pb[off] : 0.0f;
    }
    __syncthreads();

    float m0[VM_VPT], m1[VM_VPT], m2[VM_VPT], m3[VM_VPT], m4[VM_VPT];
    vm_moment<0>(p, sa, sb, t1, t2, sg, HD, HH, HWp, m0);
    vm_moment<1>(p, sa, sb, t1, t2, sg, HD, HH, HWp, m1);
    vm_moment<2>(p, sa, sb, t1, t2, sg, HD, HH, HWp, m2);
    vm_moment<3>(p, sa, sb, t1, t2, sg, HD, HH, HWp, m3);
    vm_moment<4>(p, sa, sb, t1, t2, sg, HD, HH, HWp, m4);

    // per voxel: SSIM (slice_metrics_kernel's formula), squared difference and NaN flags of the centre values
    double sq[VM_VPT], ss[VM_VPT], na[VM_VPT], nb[VM_VPT];
    int ax[VM_VPT];                                    // index along `axis` inside the tile, -1: outside the volume
#pragma unroll
    for (int j = 0; j < VM_VPT; ++j) {
        const int e = threadIdx.x + j * FR_THREADS;
        ax[j] = -1;
        sq[j] = ss[j] = na[j] = nb[j] = 0.0;
        if (e >= vox) continue;
        const int lx = e & (TW - 1), ly = (e >> p.ltw) & (TH - 1), lz = e >> (p.ltw + p.lth);
        if (z0 + lz >= p.d || y0 + ly >= p.h || x0 + lx >= p.w) continue;
        const float mu1 = m0[j] * p.scale, mu2 = m1[j] * p.scale;
        float v1 = m2[j] * p.scale - mu1 * mu1, v2 = m3[j] * p.scale - mu2 * mu2;
        const float v12 = m4[j] * p.scale - mu1 * mu2;
        v1 = fmaxf(v1, 0.0f);
        v2 = fmaxf(v2, 0.0f);
        const float num = (2.0f * mu1 * mu2 + p.c1) * (2.0f * v12 + p.c2);
        const float den = (mu1 * mu1 + mu2 * mu2 + p.c1) * (v1 + v2 + p.c2) + 1e-8f;
        const float s = fminf(fmaxf(num / den, 0.0f), 1.0f);      // a NaN is dropped here and counted below
        const int c = ((lz + p.rd) * HH + ly + p.rh) * HWp + lx + p.rw;
        const float ca = sa[c], cb = sb[c];
        const float df = ca - cb;
        sq[j] = (double)df * (double)df;
        ss[j] = (double)s;
        na[j] = (ca != ca) ? 1.0 : 0.0;
        nb[j] = (cb != cb) ? 1.0 : 0.0;
        ax[j] = p.axis == 0 ? lz : p.axis == 1 ? ly : lx;
    }

    // one slot per covered index of the axis: partial[(index * S + s) * 4 ..], s = this block among the S blocks of an index
    const int cover = p.axis == 0 ? TD : p.axis == 1 ? TH : TW;
    const int i0 = p.axis == 0 ? z0 : p.axis == 1 ? y0 : x0;
    const int len = p.axis == 0 ? p.d : p.axis == 1 ? p.h : p.w;
    const long long tA = p.axis == 0 ? p.tiles_h : p.tiles_d, tB = p.axis == 2 ? p.tiles_h : p.tiles_w;
    const long long iA = p.axis == 0 ? th : td, iB = p.axis == 2 ? th : tw;
    const long long S = (long long)(gridDim.x / (p.tiles_d * p.tiles_h * p.tiles_w)) * tA * tB;
    const long long s = (vol * tA + iA) * tB + iB;
    for (int k = 0; k < cover && i0 + k < len; ++k) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < VM_VPT; ++j)
            if (ax[j] == k) v[0] += sq[j], v[1] += ss[j], v[2] += na[j], v[3] += nb[j];
        block_reduce<4, 0x0u>(v, red);
        if (threadIdx.x == 0) {
            double* out = p.partial + ((long long)(i0 + k) * S + s) * 4;
            out[0] = v[0], out[1] = v[1], out[2] = v[2], out[3] = v[3];
        }
        __syncthreads();                               // red is rewritten by the next index
    }
}

inline bool vm_dims_ok(int n, int c, int d, int h, int w) { return n > 0 && c > 0 && d > 0 && h > 0 && w > 0; }
inline bool vm_radii_ok(int rd, int rh, int rw) {
    return rd >= 0 && rh >= 0 && rw >= 0 && rd <= VM_RMAX && rh <= VM_RMAX && rw <= VM_RMAX;
}
inline long long vm_tiles(int len, int lt) { return ((long long)len + (1 << lt) - 1) >> lt; }

}  // namespace

// doubles of workspace that any axis of this shape and radius triple needs; 0 for an invalid shape or radius
extern "C" size_t ctsi_volume_metrics_workspace_doubles(int n, int c, int d, int h, int w, int rd, int rh, int rw) {
    if (!vm_dims_ok(n, c, d, h, w) || !vm_radii_ok(rd, rh, rw)) return 0;
    const VmTile t = vm_tile(rd, rh, rw);
    const long long td = vm_tiles(d, t.ltd), th = vm_tiles(h, t.lth), tw = vm_tiles(w, t.ltw);
    long long slots = (long long)d * th * tw;
    if ((long long)h * td * tw > slots) slots = (long long)h * td * tw;
    if ((long long)w * td * th > slots) slots = (long long)w * td * th;
    return (size_t)(slots * n * c * 4);
}

extern "C" int ctsi_volume_metrics(const float* a, const float* b, int n, int c, int d, int h, int w, int rd, int rh, int rw,
                                   const float* gd, const float* gh, const float* gw, int axis, float max_val,
                                   double* workspace, double* out, void* stream) {
    CTSI_CHECK_ARG(a && b && workspace && out, "ctsi_volume_metrics: null argument: a=%p b=%p workspace=%p out=%p",
                   (const void*)a, (const void*)b, (const void*)workspace, (const void*)out);
    CTSI_CHECK_ARG((gd && gh && gw) || (!gd && !gh && !gw),
                   "ctsi_volume_metrics: null argument: gd=%p gh=%p gw=%p must be all set (weights) or all null (box)",
                   (const void*)gd, (const void*)gh, (const void*)gw);
    CTSI_CHECK_ARG(vm_dims_ok(n, c, d, h, w), "ctsi_volume_metrics: bad sizes n=%d c=%d d=%d h=%d w=%d", n, c, d, h, w);
    CTSI_CHECK_ARG(vm_radii_ok(rd, rh, rw), "ctsi_volume_metrics: radii rd=%d rh=%d rw=%d must lie in [0, %d]", rd, rh, rw,
                   VM_RMAX);
    CTSI_CHECK_ARG(axis >= 0 && axis <= 2, "ctsi_volume_metrics: axis=%d must be 0 (d), 1 (h) or 2 (w)", axis);
    const VmTile t = vm_tile(rd, rh, rw);
    const long long td = vm_tiles(d, t.ltd), th = vm_tiles(h, t.lth), tw = vm_tiles(w, t.ltw);
    const double nblocks = (double)n * c * (double)td * (double)th * (double)tw;      // no wrap-around, whatever the sizes
    CTSI_CHECK_ARG(nblocks <= (double)INT_MAX, "ctsi_volume_metrics: n=%d c=%d d=%d h=%d w=%d give too many blocks (%.0f)", n,
                   c, d, h, w, nblocks);
    const long long blocks = (long long)n * c * td * th * tw;
    const size_t lds = (size_t)vm_lds_floats(t, rd, rh, rw) * sizeof(float);
    CTSI_CHECK_ARG(lds + 1024 <= (size_t)VM_LDS_MAX, "ctsi_volume_metrics: radii rd=%d rh=%d rw=%d need %zu bytes of LDS", rd,
                   rh, rw, lds);
    VmArgs p;
    p.a = a, p.b = b, p.gd = gd, p.gh = gh, p.gw = gw, p.partial = workspace;
    p.d = d, p.h = h, p.w = w, p.rd = rd, p.rh = rh, p.rw = rw;
    p.ltd = t.ltd, p.lth = t.lth, p.ltw = t.ltw;
    p.tiles_d = (int)td, p.tiles_h = (int)th, p.tiles_w = (int)tw;
    p.axis = axis;
    p.scale = gd ? 1.0f : 1.0f / (float)((2 * rd + 1) * (2 * rh + 1) * (2 * rw + 1));
    p.c1 = (0.01f * max_val) * (0.01f * max_val), p.c2 = (0.03f * max_val) * (0.03f * max_val);
    static CtsiPerDeviceOnce attr_once;
    if (attr_once.first())
        hipFuncSetAttribute((const void*)volume_metrics_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, VM_LDS_MAX - 1024);
    hipLaunchKernelGGL(volume_metrics_kernel, dim3((unsigned)blocks), dim3(FR_THREADS), lds, (hipStream_t)stream, p);
    CTSI_LAUNCH_CHECK();
    const int len = axis == 0 ? d : axis == 1 ? h : w;
    const long long slots = (long long)n * c * (axis == 0 ? th * tw : axis == 1 ? td * tw : td * th);
    hipLaunchKernelGGL((fold_slots_kernel<4, 0x0u>), dim3((unsigned)len), dim3(FR_THREADS), 0, (hipStream_t)stream, workspace,
                       out, slots, 4);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
