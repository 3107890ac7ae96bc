// fp32 inference mode: ONE implicit-GEMM convolution kernel on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32) for the
// four layer geometries of the U-Net and the VAE (include/ctsi.h, "fp32 inference mode"):
//   Conv3d 3x3x3 p=1, Conv3d 1x1x1, Conv3d (3,4,4) s=(1,2,2) p=1 (Downsample), ConvTranspose3d (3,4,4) s=(1,2,2) p=1 (Upsample).
// Activations are fp32 NDHWC; the input may be the channel concatenation of two tensors (c1 + c2, never materialised).
//
// The GEMM view (rows = output voxels of one parity class and sample, columns = output channels, K = taps x cpad), the
// geometry, the parameter block and the epilogue are conv_f32_frame.h's, shared with conv_bf16x3.hip; cpad = c1 + c2 rounded
// up to 16.
//
// Block: 256 threads = 4 waves, 128 rows x BN columns (BN = 128, 64 or 32 by cout), K staged through LDS in 16-channel
// slices, double-buffered (global loads of slice s + 1 are in flight while slice s is multiplied; one barrier per slice).
// Each wave owns TM x TN accumulator tiles of 32 x 32.  A k-ordered fmaf chain of 8 slices (128 products) is added into a
// second register set, so no output's summation runs longer than 128 terms in one chain.  The summation order depends on
// the layer only: a relaunch is bit-identical (no atomics, no split-K).
#include "conv_f32_frame.h"

#define CF_BK 16           // channels per K slice
#define CF_PAD 32          // LDS row padding (floats); untuned
#define CF_FLUSH 8         // slices per partial accumulation chain

struct ConvF32Params : ConvF32Common {
    const float* w;        // [class][K][cout_pad]
};

static ConvF32Geom cf32_geom(const ctsi_conv_desc* desc) { return cf_geom(desc, CF_BK, "ctsi_conv_f32", "fp32"); }

// ---- weight image ------------------------------------------------------------------------------------------------------
// packed[cls][k = tap * cpad + ci][co] = w(co, ci, tap of cls) (Conv3d (cout, cin, kd, kh, kw); ConvTranspose3d (cin, cout,
// kd, kh, kw)); zero for ci >= cin or co >= cout.
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

    cf_epilogue<WGM, WGN, TM, TN>(p, tot, &As[0][0][0], tile, nt, cls, b, wm, wn, kl, cl, tid);
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int ctsi_conv_f32_supported(const ctsi_conv_desc* desc) {
    return cf32_geom(desc).ok;
}

extern "C" size_t ctsi_conv_f32_weight_bytes(const ctsi_conv_desc* desc) {
    const ConvF32Geom g = cf32_geom(desc);
    return g.ok ? (size_t)g.ncls * g.K * g.cout_pad * sizeof(float) : 0;
}

extern "C" double ctsi_conv_f32_flops(const ctsi_conv_desc* desc) {
    const ConvF32Geom g = cf32_geom(desc);
    return g.ok ? g.flops : 0.0;
}

extern "C" int ctsi_conv_f32_geometry(const ctsi_conv_desc* desc, int* d_out, int* h_out, int* w_out, int* tiles_per_sample,
                                      int* nclass, int* cout_pad) {
    return cf_geometry_out(cf32_geom(desc), d_out, h_out, w_out, tiles_per_sample, nclass, cout_pad);
}

extern "C" int ctsi_conv_f32_pack_weights(const ctsi_conv_desc* desc, const float* w, void* packed, void* stream) {
    CTSI_CHECK_ARG(w && packed, "ctsi_conv_f32_pack_weights: null argument");
    const ConvF32Geom g = cf32_geom(desc);
    if (!g.ok) return CTSI_ERR_INVALID;
    CfTapTable tt;
    cf_taps(*desc, g, &tt, nullptr);
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
    const ConvF32Geom g = cf32_geom(desc);
    if (!g.ok) return CTSI_ERR_INVALID;
    ConvF32Params p = {};
    const int rc = cf_fill("ctsi_conv_f32_fwd", *desc, g, x1, x2, bias, residual, out, &p);
    if (rc != CTSI_OK) return rc;
    p.w = (const float*)packed_w;
    const dim3 grid = cf_grid(*desc, g);
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
