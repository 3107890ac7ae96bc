// fp32 inference mode: ONE implicit-GEMM convolution kernel on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32) for the
// four layer geometries of the U-Net and the VAE (include/ctsi.h, "fp32 inference mode"):
//   Conv3d 3x3x3 p=1, Conv3d 1x1x1, Conv3d (3,4,4) s=(1,2,2) p=1 (Downsample), ConvTranspose3d (3,4,4) s=(1,2,2) p=1 (Upsample).
// Activations are fp32 NDHWC; the input may be the channel concatenation of two tensors (c1 + c2, never materialised).
//
// GEMM view: rows = output voxels of one (parity class, sample), columns = output channels, K = taps x cpad (cpad = c1 + c2
// rounded up to 16; the padding channels are zero rows of the packed weight image and masked loads of the activations).
// The transposed conv is evaluated as 4 parity classes (oh % 2, ow % 2) of 3 x 2 x 2 taps each -- every class a dense
// stride-1 gather -- instead of zero insertion; blockIdx.z = class * n + sample.
//
// Block: 256 threads = 4 waves, 128 rows x BN columns (BN = 128, 64 or 32 by cout), K staged through LDS in 16-channel
// slices, double-buffered (global loads of slice s + 1 are in flight while slice s is multiplied; one barrier per slice).
// Each wave owns TM x TN accumulator tiles of 32 x 32.  A k-ordered fmaf chain of 8 slices (128 products) is added into a
// second register set, so no output's summation runs longer than 128 terms in one chain.  The summation order depends on
// the layer only: a relaunch is bit-identical (no atomics, no split-K).
#include "ctsi_internal.h"
#include <math.h>

#define CF_BM 128
#define CF_BK 16
#define CF_PAD 32          // LDS row padding (floats); untuned
#define CF_FLUSH 8         // slices per partial accumulation chain
#define CF_MAXTAPS 48      // taps of the largest kernel (3,4,4)

struct ConvF32Params {
    const float* x1;
    const float* x2;
    const float* w;        // [class][K][cout_pad]
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
    int rh[4], rw[4];            // output parity of every class (transposed)
};

struct ConvF32Geom {
    int ok;
    int ncls, ntaps, cpad, K, bn, cout_pad;
    int Do, Ho, Wo, Mh, Mw;
    long long mrows;
    int tps;
    double flops;
};

static int cf_bn(int cout) { return cout <= 32 ? 32 : (cout <= 64 ? 64 : 128); }

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

static ConvF32Geom cf_geom(const ctsi_conv_desc* dp, bool set_error) {
    ConvF32Geom g = {};
    g.ok = 0;
#define CF_REJECT(...)                                      \
    do {                                                    \
        if (set_error) ctsi_set_error(__VA_ARGS__);        \
        return g;                                           \
    } while (0)
    if (!dp) CF_REJECT("ctsi_conv_f32: null descriptor");
    const ctsi_conv_desc& d = *dp;
    if (!(d.n > 0 && d.c1 > 0 && d.c2 >= 0 && d.cout > 0 && d.di > 0 && d.hi > 0 && d.wi > 0))
        CF_REJECT("ctsi_conv_f32: sizes must be positive (n=%d c1=%d c2=%d cout=%d in=%dx%dx%d)", d.n, d.c1, d.c2, d.cout, d.di,
                  d.hi, d.wi);
    if (d.halo_d) CF_REJECT("ctsi_conv_f32: depth-sharded inputs (halo_d = 1) are not supported in the fp32 mode");
    const bool k333 = !d.transposed && d.kd == 3 && d.kh == 3 && d.kw == 3 && d.sh == 1 && d.sw == 1 && d.pd == 1 &&
                      d.ph == 1 && d.pw == 1;
    const bool k111 = !d.transposed && d.kd == 1 && d.kh == 1 && d.kw == 1 && d.sh == 1 && d.sw == 1 && d.pd == 0 &&
                      d.ph == 0 && d.pw == 0;
    const bool k344 = d.kd == 3 && d.kh == 4 && d.kw == 4 && d.sh == 2 && d.sw == 2 && d.pd == 1 && d.ph == 1 && d.pw == 1;
    if (d.transposed != 0 && d.transposed != 1) CF_REJECT("ctsi_conv_f32: transposed=%d must be 0 or 1", d.transposed);
    if (!(k333 || k111 || k344))
        CF_REJECT("ctsi_conv_f32: unsupported geometry (%s k=%dx%dx%d s=%dx%d p=%dx%dx%d); supported: 3x3x3 p1, 1x1x1, "
                  "Conv3d / ConvTranspose3d (3,4,4) s(1,2,2) p1",
                  d.transposed ? "ConvTranspose3d" : "Conv3d", d.kd, d.kh, d.kw, d.sh, d.sw, d.pd, d.ph, d.pw);
    const long long cin = (long long)d.c1 + d.c2;
    if (cin > 8192 || d.cout > 8192) CF_REJECT("ctsi_conv_f32: channel counts above 8192 (cin=%lld cout=%d)", cin, d.cout);
    g.ncls = d.transposed ? 4 : 1;
    g.ntaps = d.transposed ? 12 : d.kd * d.kh * d.kw;
    g.cpad = (int)((cin + 15) / 16 * 16);
    g.K = g.ntaps * g.cpad;
    g.bn = cf_bn(d.cout);
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
    if (g.Do < 1 || g.Ho < 1 || g.Wo < 1) CF_REJECT("ctsi_conv_f32: input %dx%dx%d too small for the kernel", d.di, d.hi, d.wi);
    g.mrows = (long long)g.Do * g.Mh * g.Mw;
    const long long tps = (g.mrows + CF_BM - 1) / CF_BM;
    const long long in_elems = (long long)d.n * d.di * d.hi * d.wi * (cin > 0 ? cin : 1);
    const long long out_elems = (long long)d.n * g.Do * g.Ho * g.Wo * d.cout;
    if (tps >= (1ll << 31) || (long long)g.ncls * d.n > 65535 || in_elems >= (1ll << 40) || out_elems >= (1ll << 40))
        CF_REJECT("ctsi_conv_f32: tensor too large (rows per sample %lld, n=%d)", g.mrows, d.n);
    g.tps = (int)tps;
    g.flops = 2.0 * d.n * (double)(d.transposed ? (long long)d.di * d.hi * d.wi : (long long)g.Do * g.Ho * g.Wo) * cin *
              d.cout * d.kd * d.kh * d.kw;
    g.ok = 1;
    return g;
#undef CF_REJECT
}

// ---- weight image ------------------------------------------------------------------------------------------------------
// packed[cls][k = tap * cpad + ci][co] = w(co, ci, tap of cls) (Conv3d (cout, cin, kd, kh, kw); ConvTranspose3d (cin, cout,
// kd, kh, kw)); zero for ci >= cin or co >= cout.
struct CfTapTable {
    signed char k[4][CF_MAXTAPS][3];
};

__global__ void __launch_bounds__(256)
conv_f32_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int cin, int cout, int cpad, int K, int cout_pad,
                     int kd, int kh, int kw, int transposed, long long total, CfTapTable tt) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int co = (int)(e % cout_pad);
        const long long r = e / cout_pad;
        const int k = (int)(r % K);
        const int cls = (int)(r / K);
        const int tap = k / cpad, ci = k - tap * cpad;
        float v = 0.0f;
        if (ci < cin && co < cout) {
            const int a = tt.k[cls][tap][0], b = tt.k[cls][tap][1], c = tt.k[cls][tap][2];
            const long long sp = ((long long)a * kh + b) * kw + c;
            const long long taps = (long long)kd * kh * kw;
            v = transposed ? w[((long long)ci * cout + co) * taps + sp] : w[((long long)co * cin + ci) * taps + sp];
        }
        packed[e] = v;
    }
}

// ---- the convolution -----------------------------------------------------------------------------------------------------
template <int WGM, int WGN, int TM, int TN>
__global__ void __launch_bounds__(256)
conv_f32_kernel(const ConvF32Params p) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    static_assert(BM == CF_BM && WGM * WGN == 4, "4 waves over 128 rows");
    constexpr int AS = BM + CF_PAD, BS = BN + CF_PAD;
    constexpr int BPT = BN / 16;                       // B floats per thread per slice
    __shared__ __attribute__((aligned(16))) float As[2][CF_BK][AS];
    __shared__ __attribute__((aligned(16))) float Bs[2][CF_BK][BS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int tile = blockIdx.x, nt = blockIdx.y;
    const int cls = blockIdx.z / p.n, b = blockIdx.z - cls * p.n;
    const float* wimg = p.w + (long long)cls * p.K * p.CoutPad + (long long)nt * BN;

    // A loader: row ar of the tile, channels [8 akh, 8 akh + 8) of the slice
    const int ar = tid & (BM - 1), akh = tid >> 7;
    const long long am = (long long)tile * BM + ar;
    const bool arow = am < p.mrows;
    int bd = 0, bh = 0, bw = 0;
    {
        const long long mm = arow ? am : 0;
        const int plane = p.Mh * p.Mw;
        const int od = (int)(mm / plane);
        const int rem = (int)(mm - (long long)od * plane);
        const int mh = rem / p.Mw, mw = rem - (rem / p.Mw) * p.Mw;
        if (p.transposed) {
            bd = od; bh = mh; bw = mw;
        } else {
            bd = od - p.pd; bh = mh * p.sh - p.ph; bw = mw * p.sw - p.pw;
        }
    }
    const long long vox_in = (long long)p.Di * p.Hi * p.Wi;
    const float* xb1 = p.x1 + (long long)b * vox_in * p.C1;
    const float* xb2 = p.C2 ? p.x2 + (long long)b * vox_in * p.C2 : nullptr;
    const int cchunks = p.cpad >> 4;
    const int nslices = p.ntaps * cchunks;
    // B loader: k row bk of the slice, columns [BPT bc, BPT bc + BPT)
    const int bk = tid >> 4, bc = (tid & 15) * BPT;

    float ra[8], rb[BPT];
    auto load = [&](int s) {
        const int tap = s / cchunks;
        const int c0 = (s - tap * cchunks) * 16 + akh * 8;
        const int id = bd + p.off[cls][tap][0], ih = bh + p.off[cls][tap][1], iw = bw + p.off[cls][tap][2];
        const bool ok = arow && (unsigned)id < (unsigned)p.Di && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
        const long long v = ((long long)id * p.Hi + ih) * p.Wi + iw;
        if (p.vec4) {
#pragma unroll
            for (int j = 0; j < 8; j += 4) {
                const int ci = c0 + j;
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) {
                    if (ci < p.C1)
                        q = *reinterpret_cast<const float4*>(xb1 + v * p.C1 + ci);
                    else if (ci < p.Cin)
                        q = *reinterpret_cast<const float4*>(xb2 + v * p.C2 + (ci - p.C1));
                }
                ra[j] = q.x; ra[j + 1] = q.y; ra[j + 2] = q.z; ra[j + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ci = c0 + j;
                float q = 0.0f;
                if (ok) {
                    if (ci < p.C1)
                        q = xb1[v * p.C1 + ci];
                    else if (ci < p.Cin)
                        q = xb2[v * p.C2 + (ci - p.C1)];
                }
                ra[j] = q;
            }
        }
        const float* wr = wimg + ((long long)s * CF_BK + bk) * p.CoutPad + bc;
        if constexpr (BPT % 4 == 0) {
#pragma unroll
            for (int j = 0; j < BPT; j += 4) {
                const float4 q = *reinterpret_cast<const float4*>(wr + j);
                rb[j] = q.x; rb[j + 1] = q.y; rb[j + 2] = q.z; rb[j + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < BPT; j += 2) {
                const float2 q = *reinterpret_cast<const float2*>(wr + j);
                rb[j] = q.x; rb[j + 1] = q.y;
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 8; ++j) As[buf][akh * 8 + j][ar] = ra[j];
        // B: each lane stores its BPT consecutive floats as 16- (8-) byte vectors: consecutive lanes fill consecutive
        // addresses (BPT single-float stores, BPT floats apart across lanes, were bank-conflicted)
        if constexpr (BPT % 4 == 0) {
#pragma unroll
            for (int j = 0; j < BPT; j += 4)
                *reinterpret_cast<float4*>(&Bs[buf][bk][bc + j]) = make_float4(rb[j], rb[j + 1], rb[j + 2], rb[j + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < BPT; j += 2) *reinterpret_cast<float2*>(&Bs[buf][bk][bc + j]) = make_float2(rb[j], rb[j + 1]);
        }
    };

    f32x16 acc[TM][TN], tot[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = tot[i][j][r] = 0.0f;

    const int kl = lane >> 5, cl = lane & 31;
    load(0);
    store(0);
    __syncthreads();
    for (int s = 0; s < nslices; ++s) {
        const int buf = s & 1;
        if (s + 1 < nslices) load(s + 1);
#pragma unroll
        for (int kk = 0; kk < CF_BK / 2; ++kk) {
            const int k = 2 * kk + kl;
            float a[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[buf][k][(wm * TM + i) * 32 + cl];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = Bs[buf][k][(wn * TN + j) * 32 + cl];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if ((s + 1) % CF_FLUSH == 0 || s + 1 == nslices) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    tot[i][j] += acc[i][j];
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
                }
        }
        if (s + 1 < nslices) store(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: bias, residual, activation, store, column sums ----
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
                float v = tot[i][j][r] + bias;
                if (p.res) v += p.res[idx];
                if (p.act == 1) v = tanhf(v);
                p.y[idx] = v;
                cs1[j] += v;
                cs2[j] += v * v;
            }
    }
    if (p.colsum) {
        // lanes l and l + 32 hold the same column; then the WGM waves of one column range, in wave order, through LDS
        float* red = &As[0][0][0];      // [WGM][BN][2]; every wave is past the main loop's last barrier
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

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int ctsi_conv_f32_supported(const ctsi_conv_desc* desc) {
    return cf_geom(desc, true).ok;
}

extern "C" size_t ctsi_conv_f32_weight_bytes(const ctsi_conv_desc* desc) {
    const ConvF32Geom g = cf_geom(desc, true);
    if (!g.ok) return 0;
    return (size_t)g.ncls * g.K * g.cout_pad * sizeof(float);
}

extern "C" double ctsi_conv_f32_flops(const ctsi_conv_desc* desc) {
    const ConvF32Geom g = cf_geom(desc, true);
    return g.ok ? g.flops : 0.0;
}

extern "C" int ctsi_conv_f32_geometry(const ctsi_conv_desc* desc, int* d_out, int* h_out, int* w_out, int* tiles_per_sample,
                                      int* nclass, int* cout_pad) {
    const ConvF32Geom g = cf_geom(desc, true);
    if (!g.ok) return CTSI_ERR_INVALID;
    if (d_out) *d_out = g.Do;
    if (h_out) *h_out = g.Ho;
    if (w_out) *w_out = g.Wo;
    if (tiles_per_sample) *tiles_per_sample = g.tps;
    if (nclass) *nclass = g.ncls;
    if (cout_pad) *cout_pad = g.cout_pad;
    return CTSI_OK;
}

static void cf_taps(const ctsi_conv_desc& d, const ConvF32Geom& g, signed char (*k)[CF_MAXTAPS][3], signed char (*off)[CF_MAXTAPS][3],
                    int* rh, int* rw) {
    for (int cls = 0; cls < 4; ++cls) {
        rh[cls] = cls >> 1;
        rw[cls] = cls & 1;
        for (int t = 0; t < CF_MAXTAPS; ++t) {
            int a = 0, b = 0, c = 0;
            if (cls < g.ncls && t < g.ntaps) cf_tap(d, cls, t, &a, &b, &c);
            k[cls][t][0] = (signed char)a; k[cls][t][1] = (signed char)b; k[cls][t][2] = (signed char)c;
            if (!d.transposed) {
                off[cls][t][0] = (signed char)a; off[cls][t][1] = (signed char)b; off[cls][t][2] = (signed char)c;
            } else {   // od = id - pd + kd, oh = 2 ih - ph + kh with oh = 2 mh + rh
                off[cls][t][0] = (signed char)(d.pd - a);
                off[cls][t][1] = (signed char)((rh[cls] + d.ph - b) / 2);
                off[cls][t][2] = (signed char)((rw[cls] + d.pw - c) / 2);
            }
        }
    }
}

extern "C" int ctsi_conv_f32_pack_weights(const ctsi_conv_desc* desc, const float* w, void* packed, void* stream) {
    CTSI_CHECK_ARG(w && packed, "ctsi_conv_f32_pack_weights: null argument");
    const ConvF32Geom g = cf_geom(desc, true);
    if (!g.ok) return CTSI_ERR_INVALID;
    CfTapTable tt;
    signed char off[4][CF_MAXTAPS][3];
    int rh[4], rw[4];
    cf_taps(*desc, g, tt.k, off, rh, rw);
    const long long total = (long long)g.ncls * g.K * g.cout_pad;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(conv_f32_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, (float*)packed,
                       desc->c1 + desc->c2, desc->cout, g.cpad, g.K, g.cout_pad, desc->kd, desc->kh, desc->kw, desc->transposed,
                       total, tt);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_conv_f32_fwd(const ctsi_conv_desc* desc, const float* x1, const float* x2, const void* packed_w,
                                 const float* bias, const float* residual, const ctsi_conv_out* out, void* stream) {
    CTSI_CHECK_ARG(desc && x1 && packed_w && out && out->y, "ctsi_conv_f32_fwd: null argument");
    const ConvF32Geom g = cf_geom(desc, true);
    if (!g.ok) return CTSI_ERR_INVALID;
    const ctsi_conv_desc& d = *desc;
    CTSI_CHECK_ARG(d.c2 == 0 || x2, "ctsi_conv_f32_fwd: c2=%d but x2 is null", d.c2);
    CTSI_CHECK_ARG(out->mode == 0 || out->mode == 1, "ctsi_conv_f32_fwd: out mode %d (0: fp32 NDHWC, 1: fp32 strided)",
                   out->mode);
    CTSI_CHECK_ARG(out->mode != 0 || (out->c_off >= 0 && out->cout_stride >= out->c_off + d.cout),
                   "ctsi_conv_f32_fwd: channel slice [%d, %d) outside stride %d", out->c_off, out->c_off + d.cout,
                   out->cout_stride);
    CTSI_CHECK_ARG(out->act == 0 || out->act == 1, "ctsi_conv_f32_fwd: act %d (0: none, 1: tanh)", out->act);
    CTSI_CHECK_ARG(out->gn_x == nullptr, "ctsi_conv_f32_fwd: the fused GroupNorm tail is a bf16-path epilogue");
    ConvF32Params p = {};
    p.x1 = x1; p.x2 = x2; p.w = (const float*)packed_w; p.bias = bias; p.res = residual;
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
    signed char kt[4][CF_MAXTAPS][3];
    cf_taps(d, g, kt, p.off, p.rh, p.rw);
    const dim3 grid((unsigned)g.tps, (unsigned)(g.cout_pad / g.bn), (unsigned)(g.ncls * d.n));
    hipStream_t st = (hipStream_t)stream;
    if (g.bn == 128)
        hipLaunchKernelGGL((conv_f32_kernel<2, 2, 2, 2>), grid, dim3(256), 0, st, p);
    else if (g.bn == 64)
        hipLaunchKernelGGL((conv_f32_kernel<2, 2, 2, 1>), grid, dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL((conv_f32_kernel<4, 1, 1, 1>), grid, dim3(256), 0, st, p);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
