// bf16x3 inference mode: the implicit-GEMM convolution on fp32 tensors with the inner product on the bf16 MFMA
// (v_mfma_f32_32x32x16_bf16) through a two-term split of both fp32 operands (include/ctsi.h, "bf16x3 inference mode"):
//   xh = bf16(x) (round to nearest even), xl = bf16(x - float(xh)); the same for w;
//   y = act(sum_k (xh wh + xh wl + xl wh) + bias [+ residual]),  every product exact in fp32, every sum in fp32.
// Geometry, parameter block and epilogue are conv_f32_frame.h's, shared with conv_f32.hip.  This file's own:
//   K slice     32 channels (cpad = c1 + c2 rounded up to 32) = two k-steps of 16; double-buffered, one barrier per slice.
//   LDS images  k-contiguous: [row or column][32 bf16] with an 80-byte row stride, a `hi` and a `lo` image per operand.  Lane l
//               of the MFMA holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col l & 31], j = 0..7: one
//               16-byte read per fragment.  80 bytes = 5 sixteen-byte slots: 5 is odd, so the 16 rows of one ds_read_b128
//               lane group (16 distinct rows mod 16) fall on 16 distinct slots of the 256-byte bank row, and the 8 consecutive
//               rows of one ds_write_b128 lane group on 8 distinct slots of its 128-byte bank row.
//   activations split on the way into LDS: the loader thread of (row, 16 channels) converts its 16 floats to 16 hi + 16 lo.
//   weights     split once, at pack time: image [hi | lo][class][slice = tap * cpad / 32 + chunk][cout_pad][32 bf16]; the B
//               loader moves 16-byte vectors from global memory to LDS unchanged.
//   accumulation  two register sets per tile: `acc` takes xh wh, `crs` the two cross terms (about 2^-8 of the main term: summed
//               among themselves they lose nothing to the main sum's rounding); crs is added to acc once, after the last slice.
//               The order depends on the layer only: no atomics, no split-K, a relaunch is bit-identical.
#include "conv_f32_frame.h"

#define CX_BK 32           // channels per K slice
#define CX_RS 80           // LDS row stride in bytes (64 data + 16 padding)

struct ConvX3Params : ConvF32Common {
    const bf16_t* wh;      // [class][slice][cout_pad][32]
    const bf16_t* wl;
};

static ConvF32Geom cx_geom(const ctsi_conv_desc* desc) { return cf_geom(desc, CX_BK, "ctsi_conv_bf16x3", "bf16x3"); }

// ---- weight images -----------------------------------------------------------------------------------------------------
// hi / lo[cls][slice s = tap * (cpad / 32) + ci / 32][co][ci % 32] = the split of w(co, ci, tap of cls); zero for ci >= cin or
// co >= cout (both halves: bf16(0) and bf16(0 - 0)).
__global__ void __launch_bounds__(256)
conv_bf16x3_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, int cin, int cout,
                        int cpad, int nslices, int cout_pad, int kd, int kh, int kw, int transposed, long long total,
                        CfTapTable tt) {
    const int cchunks = cpad / CX_BK;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int kk = (int)(e % CX_BK);
        long long r = e / CX_BK;
        const int co = (int)(r % cout_pad);
        r /= cout_pad;
        const int s = (int)(r % nslices);
        const int cls = (int)(r / nslices);
        const int tap = s / cchunks, ci = (s - tap * cchunks) * CX_BK + kk;
        float v = 0.0f;
        if (ci < cin && co < cout) {
            const int a = tt.k[cls][tap][0], b = tt.k[cls][tap][1], c = tt.k[cls][tap][2];
            const long long sp = ((long long)a * kh + b) * kw + c;
            const long long taps = (long long)kd * kh * kw;
            v = transposed ? w[((long long)ci * cout + co) * taps + sp] : w[((long long)co * cin + ci) * taps + sp];
        }
        const bf16_t h = f32_to_bf16(v);
        hi[e] = h;
        lo[e] = f32_to_bf16(v - bf16_to_f32(h));
    }
}

// ---- the convolution -----------------------------------------------------------------------------------------------------
typedef unsigned int cx_u4 __attribute__((ext_vector_type(4)));

// 8 fp32 -> 8 hi + 8 lo bf16 (k-contiguous: element j in bits [16 (j & 1), 16 (j & 1) + 16) of dword j / 2)
__device__ __forceinline__ void cx_split8(const float* f, cx_u4* h, cx_u4* l) {
    unsigned int hh[4], ll[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x2_t v;
        v.x = f[2 * q];
        v.y = f[2 * q + 1];
        const unsigned int hp = pack_bf16x2_v(v);
        f32x2_t d;
        d.x = v.x - __uint_as_float(hp << 16);            // exact in fp32: |x - hi| <= ulp_bf16(x) / 2
        d.y = v.y - __uint_as_float(hp & 0xffff0000u);
        hh[q] = hp;
        ll[q] = pack_bf16x2_v(d);
    }
    h->x = hh[0]; h->y = hh[1]; h->z = hh[2]; h->w = hh[3];
    l->x = ll[0]; l->y = ll[1]; l->z = ll[2]; l->w = ll[3];
}

template <int BN>
constexpr int cx_lds_bytes() { return 2 * 2 * (CF_BM + BN) * CX_RS; }

template <int WGM, int WGN, int TM, int TN>
__global__ void __launch_bounds__(256, 2)
conv_bf16x3_kernel(const ConvX3Params p) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    static_assert(BM == CF_BM && WGM * WGN == 4, "4 waves over 128 rows");
    constexpr int A_IMG = BM * CX_RS, B_IMG = BN * CX_RS;      // bytes of one (buffer, half) image
    constexpr int NVB = BN / 32;                               // 16-byte B vectors per thread per slice (hi and lo together)
    extern __shared__ __attribute__((aligned(16))) unsigned char cx_smem[];
    // [buf][half] images: A at (buf * 2 + half) * A_IMG, B behind the four A images
    unsigned char* const As = cx_smem;
    unsigned char* const Bs = cx_smem + 4 * A_IMG;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int tile = blockIdx.x, nt = blockIdx.y;
    const int cls = blockIdx.z / p.n, b = blockIdx.z - cls * p.n;

    // A loader: row ar of the tile, channels [16 akh, 16 akh + 16) of the slice
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
    const int cchunks = p.cpad / CX_BK;
    const int nslices = p.ntaps * cchunks;
    // B loader: vector v = tid + 256 i of the slice's [half][BN columns][4 k-quarters]; consecutive threads, consecutive bytes
    const long long wcls = ((long long)cls * nslices * p.CoutPad + (long long)nt * BN) * CX_BK;
    const bf16_t* bsrc[NVB];
    int bdst[NVB];
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
        const int v = tid + 256 * i;
        const int half = v / (BN * 4), r = v - half * (BN * 4);
        const int col = r >> 2, kq = r & 3;
        bsrc[i] = (half ? p.wl : p.wh) + wcls + (long long)col * CX_BK + kq * 8;
        bdst[i] = half * B_IMG + col * CX_RS + kq * 16;
    }

    float ra[16];
    cx_u4 rb[NVB];
    auto load = [&](int s) {
        const int tap = s / cchunks;
        const int c0 = (s - tap * cchunks) * CX_BK + akh * 16;
        const int id = bd + p.off[cls][tap][0], ih = bh + p.off[cls][tap][1], iw = bw + p.off[cls][tap][2];
        const bool ok = arow && (unsigned)id < (unsigned)p.Di && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
        const long long v = ((long long)id * p.Hi + ih) * p.Wi + iw;
        if (p.vec4) {
#pragma unroll
            for (int j = 0; j < 16; j += 4) {
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
            for (int j = 0; j < 16; ++j) {
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
        const long long so = (long long)s * p.CoutPad * CX_BK;
#pragma unroll
        for (int i = 0; i < NVB; ++i) rb[i] = *reinterpret_cast<const cx_u4*>(bsrc[i] + so);
    };
    auto store = [&](int buf) {
        unsigned char* ah = As + (buf * 2) * A_IMG + ar * CX_RS + akh * 32;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            cx_u4 h, l;
            cx_split8(ra + 8 * g, &h, &l);
            *reinterpret_cast<cx_u4*>(ah + g * 16) = h;
            *reinterpret_cast<cx_u4*>(ah + A_IMG + g * 16) = l;
        }
        unsigned char* bb = Bs + (buf * 2) * B_IMG;
#pragma unroll
        for (int i = 0; i < NVB; ++i) *reinterpret_cast<cx_u4*>(bb + bdst[i]) = rb[i];
    };

    f32x16 acc[TM][TN], crs[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = crs[i][j][r] = 0.0f;

    const int kl = lane >> 5, cl = lane & 31;
    const int afrag = (wm * TM * 32 + cl) * CX_RS + kl * 16;
    const int bfrag = (wn * TN * 32 + cl) * CX_RS + kl * 16;
    load(0);
    store(0);
    __syncthreads();
    for (int s = 0; s < nslices; ++s) {
        const int buf = s & 1;
        if (s + 1 < nslices) load(s + 1);
        const unsigned char* ab = As + (buf * 2) * A_IMG + afrag;
        const unsigned char* bb = Bs + (buf * 2) * B_IMG + bfrag;
#pragma unroll
        for (int kk = 0; kk < CX_BK / 16; ++kk) {
            bf16x8 ah[TM], al[TM], bhv[TN], blv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ah[i] = *reinterpret_cast<const bf16x8*>(ab + i * 32 * CX_RS + kk * 32);
                al[i] = *reinterpret_cast<const bf16x8*>(ab + A_IMG + i * 32 * CX_RS + kk * 32);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                bhv[j] = *reinterpret_cast<const bf16x8*>(bb + j * 32 * CX_RS + kk * 32);
                blv[j] = *reinterpret_cast<const bf16x8*>(bb + B_IMG + j * 32 * CX_RS + kk * 32);
            }
            // three passes over the tiles, so that MFMAs on one accumulator are TM * TN instructions apart
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) crs[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bhv[j], crs[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) crs[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], blv[j], crs[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bhv[j], acc[i][j], 0, 0, 0);
        }
        if (s + 1 < nslices) store(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] += crs[i][j];

    cf_epilogue<WGM, WGN, TM, TN>(p, acc, reinterpret_cast<float*>(cx_smem), tile, nt, cls, b, wm, wn, kl, cl, tid);
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int ctsi_conv_bf16x3_supported(const ctsi_conv_desc* desc) {
    return cx_geom(desc).ok;
}

extern "C" size_t ctsi_conv_bf16x3_weight_bytes(const ctsi_conv_desc* desc) {
    const ConvF32Geom g = cx_geom(desc);
    return g.ok ? (size_t)2 * g.ncls * g.K * g.cout_pad * sizeof(bf16_t) : 0;
}

extern "C" double ctsi_conv_bf16x3_flops(const ctsi_conv_desc* desc) {
    const ConvF32Geom g = cx_geom(desc);
    return g.ok ? g.flops : 0.0;
}

extern "C" int ctsi_conv_bf16x3_geometry(const ctsi_conv_desc* desc, int* d_out, int* h_out, int* w_out, int* tiles_per_sample,
                                         int* nclass, int* cout_pad) {
    return cf_geometry_out(cx_geom(desc), d_out, h_out, w_out, tiles_per_sample, nclass, cout_pad);
}

extern "C" int ctsi_conv_bf16x3_pack_weights(const ctsi_conv_desc* desc, const float* w, void* packed, void* stream) {
    CTSI_CHECK_ARG(w && packed, "ctsi_conv_bf16x3_pack_weights: null argument");
    const ConvF32Geom g = cx_geom(desc);
    if (!g.ok) return CTSI_ERR_INVALID;
    CfTapTable tt;
    cf_taps(*desc, g, &tt, nullptr);
    const long long total = (long long)g.ncls * g.K * g.cout_pad;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    bf16_t* hi = (bf16_t*)packed;
    hipLaunchKernelGGL(conv_bf16x3_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, hi, hi + total,
                       desc->c1 + desc->c2, desc->cout, g.cpad, g.K / CX_BK, g.cout_pad, desc->kd, desc->kh, desc->kw,
                       desc->transposed, total, tt);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

template <int WGM, int WGN, int TM, int TN>
static void cx_launch(const dim3& grid, hipStream_t st, const ConvX3Params& p) {
    constexpr int lds = cx_lds_bytes<WGN * TN * 32>();
    static CtsiPerDeviceOnce attr_once;
    if (attr_once.first())
        hipFuncSetAttribute((const void*)conv_bf16x3_kernel<WGM, WGN, TM, TN>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL((conv_bf16x3_kernel<WGM, WGN, TM, TN>), grid, dim3(256), lds, st, p);
}

extern "C" int ctsi_conv_bf16x3_fwd(const ctsi_conv_desc* desc, const float* x1, const float* x2, const void* packed_w,
                                    const float* bias, const float* residual, const ctsi_conv_out* out, void* stream) {
    CTSI_CHECK_ARG(desc && x1 && packed_w && out && out->y, "ctsi_conv_bf16x3_fwd: null argument");
    const ConvF32Geom g = cx_geom(desc);
    if (!g.ok) return CTSI_ERR_INVALID;
    ConvX3Params p = {};
    const int rc = cf_fill("ctsi_conv_bf16x3_fwd", *desc, g, x1, x2, bias, residual, out, &p);
    if (rc != CTSI_OK) return rc;
    CTSI_CHECK_ARG(((uintptr_t)packed_w & 15) == 0, "ctsi_conv_bf16x3_fwd: the packed image must be 16-byte aligned");
    p.wh = (const bf16_t*)packed_w;
    p.wl = p.wh + (long long)g.ncls * g.K * g.cout_pad;
    const dim3 grid = cf_grid(*desc, g);
    hipStream_t st = (hipStream_t)stream;
    if (g.bn == 128)
        cx_launch<2, 2, 2, 2>(grid, st, p);
    else if (g.bn == 64)
        cx_launch<2, 2, 2, 1>(grid, st, p);
    else
        cx_launch<4, 1, 1, 1>(grid, st, p);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
