// Latent-space window fusion (MultiDiffusion, Bar-Tal et al. 2023): the two passes that move data between
// the full latent and the batch of overlapping windows inside the captured sampler step.
//   window_gather   the network input the update wrote for the full volume, cut into the z half of every window row: a pure
//                   copy, dst row (g nw + k) batch + b <- src row b at window k's start, for both guidance halves g.
//   window_blend    the network's fp32 output of all windows, blended into one full-size prediction.  Gather form: one thread
//                   per (voxel, 4 channels) loops over the windows that cover it, through three per-axis tables {count, window
//                   index, offset inside the window, weight}; the weights are normalised per axis on the host (the windows form
//                   a product grid, so the 3-D partition of unity factorises).  No accumulator, no atomics, fixed order kd, kh, kw.
// Both stream once over tens of MB: HBM-bound, 16-byte lanes, grid capped at 2048 blocks with a grid-stride loop, no LDS.
// The starts and the tables are trusted: window_fuse.axis_table, their one source, refuses windows outside the volume.
#include "ctsi_internal.h"

namespace {

constexpr int WF_MAX_BLOCKS = 2048;        // 256 CUs x 8 blocks of 256 threads

// V: the widest of uint4 / uint2 / uint32_t / uint16_t that divides the channel bytes and both voxel pitches
template <typename V>
__global__ void __launch_bounds__(256)
window_gather_kernel(const V* __restrict__ src, V* __restrict__ dst, const int* __restrict__ starts, int batch, int nw, int D,
                     int H, int W, int td, int lh, int lw, int cv, int src_pitch, int dst_pitch, long long total) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
        long long t = q / cv;                       // destination voxel, over all rows
        const int c = (int)(q - t * cv);
        const long long dvox = t;
        const int ow = (int)(t % lw);
        t /= lw;
        const int oh = (int)(t % lh);
        t /= lh;
        const int od = (int)(t % td);
        const long long row = t / td;               // (g nw + k) batch + b
        const int b = (int)(row % batch);
        const int k = (int)((row / batch) % nw);
        const int s0 = starts[3 * k], s1 = starts[3 * k + 1], s2 = starts[3 * k + 2];
        const long long svox = (((long long)b * D + (s0 + od)) * H + (s1 + oh)) * W + (s2 + ow);
        dst[dvox * dst_pitch + c] = src[svox * src_pitch + c];
    }
}

struct AxisTable {
    const int* cnt;      // [P]
    const int* idx;      // [P][K] window index along the axis
    const int* off;      // [P][K] position inside that window
    const float* wgt;    // [P][K] normalised weight
    int K, nwin, size;
};

__global__ void __launch_bounds__(256)
window_blend_kernel(const float* __restrict__ win, float* __restrict__ full, AxisTable ad, AxisTable ah, AxisTable aw, int batch,
                    int D, int H, int W, int C, long long total) {
    const int c4n = C / 4;
    const int nw = ad.nwin * ah.nwin * aw.nwin;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
        long long t = q / c4n;                      // full-volume voxel, over all rows
        const int c = (int)(q - t * c4n) * 4;
        const long long vox = t;
        const int x = (int)(t % W);
        t /= W;
        const int y = (int)(t % H);
        t /= H;
        const int z = (int)(t % D);
        const long long r = t / D;                  // g batch + b
        const long long g = r / batch, b = r % batch;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const int nd = ad.cnt[z], nh = ah.cnt[y], nx = aw.cnt[x];
        for (int jd = 0; jd < nd; ++jd) {
            const int kd = ad.idx[z * ad.K + jd], od = ad.off[z * ad.K + jd];
            const float wd = ad.wgt[z * ad.K + jd];
            for (int jh = 0; jh < nh; ++jh) {
                const int kh = ah.idx[y * ah.K + jh], oh = ah.off[y * ah.K + jh];
                const float wdh = wd * ah.wgt[y * ah.K + jh];
                for (int jw = 0; jw < nx; ++jw) {
                    const int kw = aw.idx[x * aw.K + jw], ow = aw.off[x * aw.K + jw];
                    const float wt = wdh * aw.wgt[x * aw.K + jw];
                    const long long k = ((long long)kd * ah.nwin + kh) * aw.nwin + kw;
                    const long long row = (g * nw + k) * batch + b;
                    const long long wv = ((row * ad.size + od) * ah.size + oh) * aw.size + ow;
                    const float4 v = *reinterpret_cast<const float4*>(win + wv * C + c);
                    acc.x = fmaf(wt, v.x, acc.x);
                    acc.y = fmaf(wt, v.y, acc.y);
                    acc.z = fmaf(wt, v.z, acc.z);
                    acc.w = fmaf(wt, v.w, acc.w);
                }
            }
        }
        *reinterpret_cast<float4*>(full + vox * C + c) = acc;
    }
}

unsigned wf_blocks(long long total) {
    long long blocks = (total + 255) / 256;
    return (unsigned)(blocks > WF_MAX_BLOCKS ? WF_MAX_BLOCKS : blocks);
}

template <typename V>
void gather_launch(const void* src, void* dst, const int* starts, int batch, int nw, int D, int H, int W, int td, int lh, int lw,
                   int c_bytes, int src_bytes, int dst_bytes, long long dvox, void* stream) {
    const int v = (int)sizeof(V);
    const long long total = dvox * (c_bytes / v);
    hipLaunchKernelGGL((window_gather_kernel<V>), dim3(wf_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const V*)src,
                       (V*)dst, starts, batch, nw, D, H, W, td, lh, lw, c_bytes / v, src_bytes / v, dst_bytes / v, total);
}

int gather(const char* name, const void* src, void* dst, const int* starts, int batch, int halves, int nw, int D, int H, int W,
           int td, int lh, int lw, int L, int src_c_total, int dst_c_total, int es, void* stream) {
    CTSI_CHECK_ARG(src && dst && starts, "%s: null argument", name);
    CTSI_CHECK_ARG(batch > 0 && (halves == 1 || halves == 2) && nw > 0 && L > 0 && td > 0 && lh > 0 && lw > 0 && td <= D &&
                       lh <= H && lw <= W && L <= src_c_total && L <= dst_c_total,
                   "%s: bad shape batch=%d halves=%d nw=%d full=(%d,%d,%d) window=(%d,%d,%d) L=%d c_total=%d/%d", name, batch,
                   halves, nw, D, H, W, td, lh, lw, L, src_c_total, dst_c_total);
    const long long dvox = (long long)halves * nw * batch * td * lh * lw;
    const int cb = L * es, sb = src_c_total * es, db = dst_c_total * es;
    auto fits = [&](int v) { return cb % v == 0 && sb % v == 0 && db % v == 0 && aligned_to(src, v) && aligned_to(dst, v); };
    if (fits(16))
        gather_launch<uint4>(src, dst, starts, batch, nw, D, H, W, td, lh, lw, cb, sb, db, dvox, stream);
    else if (fits(8))
        gather_launch<uint2>(src, dst, starts, batch, nw, D, H, W, td, lh, lw, cb, sb, db, dvox, stream);
    else if (fits(4))
        gather_launch<uint32_t>(src, dst, starts, batch, nw, D, H, W, td, lh, lw, cb, sb, db, dvox, stream);
    else
        gather_launch<uint16_t>(src, dst, starts, batch, nw, D, H, W, td, lh, lw, cb, sb, db, dvox, stream);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

}  // namespace

extern "C" int ctsi_window_gather(const void* src_bf16, void* dst_bf16, const int* starts, int batch, int halves, int nw, int D,
                                  int H, int W, int td, int lh, int lw, int L, int src_c_total, int dst_c_total, void* stream) {
    return gather("ctsi_window_gather", src_bf16, dst_bf16, starts, batch, halves, nw, D, H, W, td, lh, lw, L, src_c_total,
                  dst_c_total, 2, stream);
}

extern "C" int ctsi_window_gather_f32(const float* src, float* dst, const int* starts, int batch, int halves, int nw, int D, int H,
                                      int W, int td, int lh, int lw, int L, int src_c_total, int dst_c_total, void* stream) {
    return gather("ctsi_window_gather_f32", src, dst, starts, batch, halves, nw, D, H, W, td, lh, lw, L, src_c_total, dst_c_total,
                  4, stream);
}

extern "C" int ctsi_window_blend(const float* win, float* full, const int* tab_i, const float* tab_w, int batch, int halves,
                                 int nwd, int nwh, int nww, int D, int H, int W, int td, int lh, int lw, int C, int kd, int kh,
                                 int kw, void* stream) {
    CTSI_CHECK_ARG(win && full && tab_i && tab_w, "ctsi_window_blend: null argument");
    CTSI_CHECK_ARG(batch > 0 && (halves == 1 || halves == 2) && nwd > 0 && nwh > 0 && nww > 0 && td > 0 && lh > 0 && lw > 0 &&
                       td <= D && lh <= H && lw <= W && kd > 0 && kh > 0 && kw > 0 && kd <= nwd && kh <= nwh && kw <= nww,
                   "ctsi_window_blend: bad shape batch=%d halves=%d windows=(%d,%d,%d) full=(%d,%d,%d) window=(%d,%d,%d) "
                   "cover=(%d,%d,%d)", batch, halves, nwd, nwh, nww, D, H, W, td, lh, lw, kd, kh, kw);
    CTSI_CHECK_ARG(C > 0 && C % 4 == 0 && aligned_to(win, 16) && aligned_to(full, 16),
                   "ctsi_window_blend: the channel count must be a multiple of 4 and the tensors 16-byte aligned (C=%d)", C);
    // tab_i: per axis [P] counts, [P][K] window indices, [P][K] offsets; tab_w: per axis [P][K] weights (axes d, h, w in turn)
    AxisTable ad{tab_i, tab_i + D, tab_i + D + (long long)D * kd, tab_w, kd, nwd, td};
    const int* ih = tab_i + D + 2LL * D * kd;
    AxisTable ah{ih, ih + H, ih + H + (long long)H * kh, tab_w + (long long)D * kd, kh, nwh, lh};
    const int* iw = ih + H + 2LL * H * kh;
    AxisTable aw{iw, iw + W, iw + W + (long long)W * kw, tab_w + (long long)D * kd + (long long)H * kh, kw, nww, lw};
    const long long total = (long long)halves * batch * D * H * W * (C / 4);
    hipLaunchKernelGGL(window_blend_kernel, dim3(wf_blocks(total)), dim3(256), 0, (hipStream_t)stream, win, full, ad, ah, aw,
                       batch, D, H, W, C, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
