// The frame that the two convolutions on fp32 tensors share (conv_f32.hip: f32 MFMA; conv_bf16x3.hip: split-bf16 MFMA):
// the layer geometry and its rejections, the tap tables, the parameter block both kernels read, the argument checks of
// `_fwd`, and the device epilogue (bias, residual, tanh, NDHWC / strided store, column sums for ctsi_gn_finalize).
//
// GEMM view: rows = output voxels of one (parity class, sample), columns = output channels, K = taps x cpad (cpad = c1 + c2
// rounded up to the family's K slice; the padding channels are zero rows of the packed weight image and masked loads of the
// activations).  The transposed conv is evaluated as 4 parity classes (oh % 2, ow % 2) of 3 x 2 x 2 taps each -- every class
// a dense stride-1 gather -- instead of zero insertion; blockIdx.z = class * n + sample.
//
// The A loader (row decode, masked two-source gather) is NOT here: it sits inside each kernel's software-pipelined main loop
// and differs in chunk width (8 or 16 floats), and sharing it moved register allocation and occupancy of the two families in
// opposite directions.
#pragma once
#include "ctsi_internal.h"
#include <math.h>

#define CF_BM 128          // rows of a block
#define CF_MAXTAPS 48      // taps of the largest kernel (3,4,4)

struct ConvF32Geom {
    int ok;
    int ncls, ntaps, cpad, K, bn, cout_pad;
    int Do, Ho, Wo, Mh, Mw;
    long long mrows;
    int tps;
    double flops;
};

// what both kernels read besides their weight images
struct ConvF32Common {
    const float* x1;
    const float* x2;
    const float* bias;
    const float* res;      // optional residual, addressed like y
    float* y;
    float* colsum;         // optional [2][ncls * n * tps][cout_pad]
    int C1, C2, Cin, Di, Hi, Wi;
    int Do, Ho, Wo, Mh, Mw;
    long long mrows;       // rows per (class, sample) = Do * Mh * Mw
    int ntaps, cpad, K, Cout, CoutPad;
    int n, tps, vec4, transposed;
    int sh, sw, pd, ph, pw;
    int mode, cout_stride, c_off, act;
    long long sn, sc, sd, shs, sws;
    signed char off[4][CF_MAXTAPS][3];   // input offset of every (class, tap) relative to the row's base coordinate
    int rh[4], rw[4];                    // output parity of every class (transposed)
};

// kd, kh, kw of every (class, tap): what a pack kernel indexes the weight tensor with
struct CfTapTable {
    signed char k[4][CF_MAXTAPS][3];
};

// kd, kh, kw of tap t of class cls
static void cf_tap(const ctsi_conv_desc& d, int cls, int t, int* kd, int* kh, int* kw) {
    if (!d.transposed) {
        *kd = t / (d.kh * d.kw);
        *kh = (t / d.kw) % d.kh;
        *kw = t % d.kw;
    } else {
        const int rh = cls >> 1, rw = cls & 1;
        *kd = t / 4;
        *kh = ((rh + d.ph) & 1) + 2 * ((t >> 1) & 1);
        *kw = ((rw + d.pw) & 1) + 2 * (t & 1);
    }
}

// The geometry of a layer, or ok = 0 and the reason in ctsi_last_error.  bk: channels per K slice; api: the family's error
// prefix; mode: its name in the depth-sharding refusal.
static ConvF32Geom cf_geom(const ctsi_conv_desc* dp, int bk, const char* api, const char* mode) {
    ConvF32Geom g = {};
    g.ok = 0;
#define CF_REJECT(...)               \
    do {                             \
        ctsi_set_error(__VA_ARGS__); \
        return g;                    \
    } while (0)
    if (!dp) CF_REJECT("%s: null descriptor", api);
    const ctsi_conv_desc& d = *dp;
    if (!(d.n > 0 && d.c1 > 0 && d.c2 >= 0 && d.cout > 0 && d.di > 0 && d.hi > 0 && d.wi > 0))
        CF_REJECT("%s: sizes must be positive (n=%d c1=%d c2=%d cout=%d in=%dx%dx%d)", api, d.n, d.c1, d.c2, d.cout, d.di, d.hi,
                  d.wi);
    if (d.halo_d) CF_REJECT("%s: depth-sharded inputs (halo_d = 1) are not supported in the %s mode", api, mode);
    const bool k333 = !d.transposed && d.kd == 3 && d.kh == 3 && d.kw == 3 && d.sh == 1 && d.sw == 1 && d.pd == 1 &&
                      d.ph == 1 && d.pw == 1;
    const bool k111 = !d.transposed && d.kd == 1 && d.kh == 1 && d.kw == 1 && d.sh == 1 && d.sw == 1 && d.pd == 0 &&
                      d.ph == 0 && d.pw == 0;
    const bool k344 = d.kd == 3 && d.kh == 4 && d.kw == 4 && d.sh == 2 && d.sw == 2 && d.pd == 1 && d.ph == 1 && d.pw == 1;
    if (d.transposed != 0 && d.transposed != 1) CF_REJECT("%s: transposed=%d must be 0 or 1", api, d.transposed);
    if (!(k333 || k111 || k344))
        CF_REJECT("%s: unsupported geometry (%s k=%dx%dx%d s=%dx%d p=%dx%dx%d); supported: 3x3x3 p1, 1x1x1, "
                  "Conv3d / ConvTranspose3d (3,4,4) s(1,2,2) p1",
                  api, d.transposed ? "ConvTranspose3d" : "Conv3d", d.kd, d.kh, d.kw, d.sh, d.sw, d.pd, d.ph, d.pw);
    const long long cin = (long long)d.c1 + d.c2;
    if (cin > 8192 || d.cout > 8192) CF_REJECT("%s: channel counts above 8192 (cin=%lld cout=%d)", api, cin, d.cout);
    g.ncls = d.transposed ? 4 : 1;
    g.ntaps = d.transposed ? 12 : d.kd * d.kh * d.kw;
    g.cpad = (int)((cin + bk - 1) / bk * bk);
    g.K = g.ntaps * g.cpad;
    g.bn = d.cout <= 32 ? 32 : (d.cout <= 64 ? 64 : 128);
    g.cout_pad = (d.cout + g.bn - 1) / g.bn * g.bn;
    if (d.transposed) {
        g.Do = d.di - 2 * d.pd + d.kd - 1;
        g.Ho = (d.hi - 1) * d.sh - 2 * d.ph + d.kh;
        g.Wo = (d.wi - 1) * d.sw - 2 * d.pw + d.kw;
        g.Mh = d.hi;
        g.Mw = d.wi;
    } else {
        g.Do = d.di + 2 * d.pd - d.kd + 1;
        g.Ho = (d.hi + 2 * d.ph - d.kh) / d.sh + 1;
        g.Wo = (d.wi + 2 * d.pw - d.kw) / d.sw + 1;
        g.Mh = g.Ho;
        g.Mw = g.Wo;
    }
    if (g.Do < 1 || g.Ho < 1 || g.Wo < 1) CF_REJECT("%s: input %dx%dx%d too small for the kernel", api, d.di, d.hi, d.wi);
    g.mrows = (long long)g.Do * g.Mh * g.Mw;
    const long long tps = (g.mrows + CF_BM - 1) / CF_BM;
    const long long in_elems = (long long)d.n * d.di * d.hi * d.wi * (cin > 0 ? cin : 1);
    const long long out_elems = (long long)d.n * g.Do * g.Ho * g.Wo * d.cout;
    if (tps >= (1ll << 31) || (long long)g.ncls * d.n > 65535 || in_elems >= (1ll << 40) || out_elems >= (1ll << 40))
        CF_REJECT("%s: tensor too large (rows per sample %lld, n=%d)", api, g.mrows, d.n);
    g.tps = (int)tps;
    // the useful 2 M N K (for bf16x3: not the three products)
    g.flops = 2.0 * d.n * (double)(d.transposed ? (long long)d.di * d.hi * d.wi : (long long)g.Do * g.Ho * g.Wo) * cin *
              d.cout * d.kd * d.kh * d.kw;
    g.ok = 1;
    return g;
#undef CF_REJECT
}

// ctsi_conv_*_geometry on a computed geometry
static int cf_geometry_out(const ConvF32Geom& g, int* d_out, int* h_out, int* w_out, int* tiles_per_sample, int* nclass,
                           int* cout_pad) {
    if (!g.ok) return CTSI_ERR_INVALID;
    if (d_out) *d_out = g.Do;
    if (h_out) *h_out = g.Ho;
    if (w_out) *w_out = g.Wo;
    if (tiles_per_sample) *tiles_per_sample = g.tps;
    if (nclass) *nclass = g.ncls;
    if (cout_pad) *cout_pad = g.cout_pad;
    return CTSI_OK;
}

// the pack table (tt, may be null) and the kernel's input offsets and parities (p, may be null)
static void cf_taps(const ctsi_conv_desc& d, const ConvF32Geom& g, CfTapTable* tt, ConvF32Common* p) {
    for (int cls = 0; cls < 4; ++cls) {
        const int rh = cls >> 1, rw = cls & 1;
        if (p) {
            p->rh[cls] = rh;
            p->rw[cls] = rw;
        }
        for (int t = 0; t < CF_MAXTAPS; ++t) {
            int a = 0, b = 0, c = 0;
            if (cls < g.ncls && t < g.ntaps) cf_tap(d, cls, t, &a, &b, &c);
            if (tt) {
                tt->k[cls][t][0] = (signed char)a; tt->k[cls][t][1] = (signed char)b; tt->k[cls][t][2] = (signed char)c;
            }
            if (!p) continue;
            if (!d.transposed) {
                p->off[cls][t][0] = (signed char)a; p->off[cls][t][1] = (signed char)b; p->off[cls][t][2] = (signed char)c;
            } else {   // od = id - pd + kd, oh = 2 ih - ph + kh with oh = 2 mh + rh
                p->off[cls][t][0] = (signed char)(d.pd - a);
                p->off[cls][t][1] = (signed char)((rh + d.ph - b) / 2);
                p->off[cls][t][2] = (signed char)((rw + d.pw - c) / 2);
            }
        }
    }
}

// The argument checks of ctsi_conv_*_fwd behind the null check and the geometry, then the common block.  Returns the status
// (CTSI_CHECK_ARG returns from its caller); api is the entry point's name.
static int cf_fill(const char* api, const ctsi_conv_desc& d, const ConvF32Geom& g, const float* x1, const float* x2,
                   const float* bias, const float* residual, const ctsi_conv_out* out, ConvF32Common* pp) {
    CTSI_CHECK_ARG(d.c2 == 0 || x2, "%s: c2=%d but x2 is null", api, d.c2);
    CTSI_CHECK_ARG(out->mode == 0 || out->mode == 1, "%s: out mode %d (0: fp32 NDHWC, 1: fp32 strided)", api, out->mode);
    CTSI_CHECK_ARG(out->mode != 0 || (out->c_off >= 0 && out->cout_stride >= out->c_off + d.cout),
                   "%s: channel slice [%d, %d) outside stride %d", api, out->c_off, out->c_off + d.cout, out->cout_stride);
    CTSI_CHECK_ARG(out->act == 0 || out->act == 1, "%s: act %d (0: none, 1: tanh)", api, out->act);
    CTSI_CHECK_ARG(out->gn_x == nullptr, "%s: the fused GroupNorm tail is a bf16-path epilogue", api);
    ConvF32Common& p = *pp;
    p.x1 = x1; p.x2 = x2; p.bias = bias; p.res = residual;
    p.y = (float*)out->y; p.colsum = out->colsum;
    p.C1 = d.c1; p.C2 = d.c2; p.Cin = d.c1 + d.c2; p.Di = d.di; p.Hi = d.hi; p.Wi = d.wi;
    p.Do = g.Do; p.Ho = g.Ho; p.Wo = g.Wo; p.Mh = g.Mh; p.Mw = g.Mw; p.mrows = g.mrows;
    p.ntaps = g.ntaps; p.cpad = g.cpad; p.K = g.K; p.Cout = d.cout; p.CoutPad = g.cout_pad;
    p.n = d.n; p.tps = g.tps;
    p.vec4 = (d.c1 % 4 == 0 && d.c2 % 4 == 0 && ((uintptr_t)x1 & 15) == 0 && ((uintptr_t)x2 & 15) == 0) ? 1 : 0;
    p.transposed = d.transposed;
    p.sh = d.sh; p.sw = d.sw; p.pd = d.pd; p.ph = d.ph; p.pw = d.pw;
    p.mode = out->mode; p.cout_stride = out->cout_stride; p.c_off = out->c_off; p.act = out->act;
    p.sn = out->sn; p.sc = out->sc; p.sd = out->sd; p.shs = out->sh; p.sws = out->sw;
    cf_taps(d, g, nullptr, pp);
    return CTSI_OK;
}

static dim3 cf_grid(const ctsi_conv_desc& d, const ConvF32Geom& g) {
    return dim3((unsigned)g.tps, (unsigned)(g.cout_pad / g.bn), (unsigned)(g.ncls * d.n));
}

// ---- the epilogue: bias, residual, activation, store, column sums --------------------------------------------------------
// acc: the wave's TM x TN accumulator tiles in the 32x32 MFMA's C/D lane map (lane = 32 kl + cl holds column cl, rows
// (r & 3) + 8 (r >> 2) + 4 kl).  red: LDS for [WGM][BN][2] floats that no wave reads any more (every wave is past the main
// loop's last barrier).
template <int WGM, int WGN, int TM, int TN>
__device__ __forceinline__ void cf_epilogue(const ConvF32Common& p, const f32x16 (&acc)[TM][TN], float* red, int tile, int nt,
                                            int cls, int b, int wm, int wn, int kl, int cl, int tid) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    const int plane = p.Mh * p.Mw;
    const int rh = p.rh[cls], rw = p.rw[cls];
    float cs1[TN], cs2[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) cs1[j] = cs2[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = nt * BN + (wn * TN + j) * 32 + cl;
        const bool cok = col < p.Cout;
        const float bias = (cok && p.bias) ? p.bias[col] : 0.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
                const long long m = (long long)tile * BM + row;
                if (m >= p.mrows || !cok) continue;
                const int od = (int)(m / plane);
                const int rem = (int)(m - (long long)od * plane);
                int oh = rem / p.Mw, ow = rem - (rem / p.Mw) * p.Mw;
                if (p.transposed) {
                    oh = 2 * oh + rh;
                    ow = 2 * ow + rw;
                }
                long long idx;
                if (p.mode == 0)
                    idx = ((((long long)b * p.Do + od) * p.Ho + oh) * p.Wo + ow) * p.cout_stride + p.c_off + col;
                else
                    idx = (long long)b * p.sn + (long long)col * p.sc + (long long)od * p.sd + (long long)oh * p.shs +
                          (long long)ow * p.sws;
                float v = acc[i][j][r] + bias;
                if (p.res) v += p.res[idx];
                if (p.act == 1) v = tanhf(v);
                p.y[idx] = v;
                cs1[j] += v;
                {
                    // v * v rounded, then added: left to the compiler, the 128x128 tiles contract this into an fma and the
                    // narrower ones do not, and the slab's bits would depend on the tile and on where this text stands
#pragma clang fp contract(off)
                    cs2[j] += v * v;
                }
            }
    }
    if (p.colsum) {
        // lanes l and l + 32 hold the same column; then the WGM waves of one column range, in wave order, through LDS
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const float o1 = __shfl_xor(cs1[j], 32), o2 = __shfl_xor(cs2[j], 32);
            if (kl == 0) {
                const int cb = (wn * TN + j) * 32 + cl;
                red[(wm * BN + cb) * 2 + 0] = cs1[j] + o1;
                red[(wm * BN + cb) * 2 + 1] = cs2[j] + o2;
            }
        }
        __syncthreads();
        if (tid < BN) {
            float t1 = 0.0f, t2 = 0.0f;
#pragma unroll
            for (int q = 0; q < WGM; ++q) {
                t1 += red[(q * BN + tid) * 2 + 0];
                t2 += red[(q * BN + tid) * 2 + 1];
            }
            const long long tg = (long long)blockIdx.z * p.tps + tile;
            const long long slab = (long long)gridDim.z * p.tps * p.CoutPad;
            const int col = nt * BN + tid;
            p.colsum[tg * p.CoutPad + col] = t1;
            p.colsum[slab + tg * p.CoutPad + col] = t2;
        }
    }
}
