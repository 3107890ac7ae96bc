// In-plane (spatial) attention: A = softmax(Q K^T / sqrt(hd)) V over the N = h * w positions of one (sample, depth slice, head),
// forward and backward, flash-attention style: nothing of size N x N is stored, and N has no LDS limit.
//
// qkv is the bf16 NDHWC output of the block's 1x1x1 conv C -> 3C: channels [q | k | v], heads split inside each third.  One
// item = one (sample, slice, head): Q, K, V are N x hd, rows 3C elements apart, channels contiguous.
//
// Forward.  One workgroup = four waves = one block of 64 queries of one item, 16 queries per wave, Q fragments in registers.
// K and V arrive in tiles of 64 keys, double-buffered in LDS: the global loads of tile t + 1 are issued before tile t's MFMAs
// and written to the other buffer after them (register staging), one barrier per tile.  The K image is [key][hd] with its
// 16-byte chunks XOR-swizzled by the key (ap_off<HD, true>) and is read back in MFMA operand layout -- lane (r16, kg) takes
// channels 8 kg .. 8 kg + 7 of key r16 per 32-channel step; the V image keeps plain rows padded by 32 bytes and is read with
// gfx950's transposing ds_read_b64_tr_b16.  The lane maps are those of attention_core.hip: the score tile is computed
// TRANSPOSED, S^T = K Q^T (lane = query r16, registers = keys 4 kg + i), so that P, rounded to bf16, is the B operand of
// O^T += V^T P^T without lane movement, and a query's max and sum live in the four lanes that hold it.  Softmax: fp32, scores
// scaled by log2(e) / sqrt(hd) and exponentiated with v_exp_f32; online max / sum across tiles; keys beyond N are -inf before
// the max; padded queries are computed on a clamped row and never stored; the row sum is taken from the unrounded
// probabilities.  lse (optional) = ln sum_j exp(s_ij) of the scaled scores.  hd 8 / 16 use the K = 16 MFMA (hd 8 zero-padded).
//
// Backward, two grids behind one entry point, no atomics and no hand-off between workgroups: every output element is the sum
// of one workgroup's accumulators in a fixed order, so the gradients are bit-identical run to run.
//   query-block pass (attn_plane_dq_kernel): the forward's frame; delta = rowsum(dA o A) from the saved bf16 A,
//     P = exp2(c s - lse log2 e) from the saved LSE (no max pass), dP^T = V dA^T, dS = P o (dP - delta),
//     dQ^T += K^T dS^T; K is the padded image here (row reads and transposed reads), V the swizzled one (row reads only).
//   key-block pass (attn_plane_dkv_kernel): one workgroup = 64 keys, 16 per wave, K and V fragments in registers; Q and dA tiles
//     of 64 queries double-buffered in LDS (padded images: row reads for S = Q K^T and dP = dA V^T with the KEY on the lane,
//     transposed reads for dV^T += dA^T P and dK^T += Q^T dS), with the tile's lse and delta beside them.
// S and dP are therefore computed twice (14 N^2 hd flops per item instead of 10): the price of bit-stable gradients without a
// protocol between workgroups.  Roundings: P -> bf16 (forward, dV), dS -> bf16 (dQ, dK), delta from the bf16 A; all else fp32.
#include "ctsi_internal.h"

typedef __attribute__((ext_vector_type(4))) short ap_s16x4;
typedef ap_s16x4 __attribute__((address_space(3))) * ap_lds_ptr;
__device__ __forceinline__ ap_s16x4 ap_tr_read(unsigned lds_addr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((ap_lds_ptr)(unsigned long long)lds_addr);
}

#define AP_NEG_INF (-__builtin_inff())
#define AP_LOG2E 1.4426950408889634f
#define AP_LN2 0.6931471805599453f
#define AP_TILE 64          // keys (or queries) per LDS tile; also the queries / keys a workgroup owns
#define AP_THREADS 256

// operand fragments of one 16-row tile over the hd channels (K dimension = channel)
template <int HD> struct ApFrag { bf16x8 v[HD / 32]; };
template <> struct ApFrag<16> { ap_s16x4 v[1]; };
template <> struct ApFrag<8> { ap_s16x4 v[1]; };      // channels 8 .. 15 of the K = 16 step are zero

template <int HD>
__device__ __forceinline__ void ap_load(ApFrag<HD>& f, const bf16_t* __restrict__ rowp, int kg) {
    if constexpr (HD == 8) {
        f.v[0] = ap_s16x4{0, 0, 0, 0};
        if (kg < 2) f.v[0] = *reinterpret_cast<const ap_s16x4*>(rowp + kg * 4);
    } else if constexpr (HD == 16) {
        f.v[0] = *reinterpret_cast<const ap_s16x4*>(rowp + kg * 4);
    } else {
#pragma unroll
        for (int s = 0; s < HD / 32; ++s) f.v[s] = *reinterpret_cast<const bf16x8*>(rowp + s * 32 + kg * 8);
    }
}

// byte offset of 16-byte chunk `ch` of row `row` of a 64-row tile image.  SWZ: dense rows, the chunk index XORed with the row
// (rows read together by the 16 lanes of one kg then fall on distinct chunks); otherwise plain rows padded by 32 bytes, which
// serve row reads and transposed reads alike.
template <int HD, bool SWZ>
__device__ __forceinline__ unsigned ap_off(int row, int ch) {
    constexpr int CPR = HD / 8;
    if constexpr (SWZ) return (unsigned)(row * (HD * 2) + ((ch ^ (row & (CPR - 1))) << 4));
    else return (unsigned)(row * (HD * 2 + 32) + (ch << 4));
}
template <int HD, bool SWZ> constexpr int ap_img_bytes() { return AP_TILE * (SWZ ? HD * 2 : HD * 2 + 32); }

// the same fragment from a tile image
template <int HD, bool SWZ>
__device__ __forceinline__ void ap_load_lds(ApFrag<HD>& f, const char* img, int row, int kg) {
    if constexpr (HD == 8) {
        f.v[0] = ap_s16x4{0, 0, 0, 0};
        if (kg < 2) f.v[0] = *reinterpret_cast<const ap_s16x4*>(img + ap_off<HD, SWZ>(row, 0) + kg * 8);
    } else if constexpr (HD == 16) {
        f.v[0] = *reinterpret_cast<const ap_s16x4*>(img + ap_off<HD, SWZ>(row, kg >> 1) + (kg & 1) * 8);
    } else {
#pragma unroll
        for (int s = 0; s < HD / 32; ++s) f.v[s] = *reinterpret_cast<const bf16x8*>(img + ap_off<HD, SWZ>(row, s * 4 + kg));
    }
}

// C[row of a][row of b] = sum_ch a[.][ch] b[.][ch]
template <int HD>
__device__ __forceinline__ f32x4 ap_dot(const ApFrag<HD>& a, const ApFrag<HD>& b) {
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (HD <= 16) {
        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a.v[0], b.v[0], acc, 0, 0, 0);
    } else {
#pragma unroll
        for (int s = 0; s < HD / 32; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v[s], b.v[s], acc, 0, 0, 0);
    }
    return acc;
}

// sum over this lane's channels of a o b (both bf16, products and sum in fp32)
template <int HD>
__device__ __forceinline__ float ap_elem_dot(const ApFrag<HD>& a, const ApFrag<HD>& b) {
    float s = 0.0f;
    constexpr int NV = HD <= 16 ? 1 : HD / 32, NE = HD <= 16 ? 4 : 8;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int e = 0; e < NE; ++e) s += bf16_to_f32((bf16_t)a.v[v][e]) * bf16_to_f32((bf16_t)b.v[v][e]);
    return s;
}

__device__ __forceinline__ ap_s16x4 ap_pack4(float a, float b, float c, float d) {
    union { ap_s16x4 v; uint32_t u[2]; } r;
    r.u[0] = pack_bf16x2(a, b);
    r.u[1] = pack_bf16x2(c, d);
    return r.v;
}

__device__ __forceinline__ float ap_max_kg(float v) {   // over the four lanes r16, r16 + 16, r16 + 32, r16 + 48
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float ap_sum_kg(float v) {
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

// One 64-row x hd tile on its way from global memory to LDS: every thread holds NCH 16-byte chunks.  Rows beyond `nrows` are
// loaded from the clamped last row (no out-of-bounds address) and written as zeros.
template <int HD> struct ApStage {
    static constexpr int CPR = HD / 8, TOTAL = AP_TILE * CPR, NCH = TOTAL >= AP_THREADS ? TOTAL / AP_THREADS : 1;
    uint4 v[NCH];
};

template <int HD>
__device__ __forceinline__ void ap_gload(ApStage<HD>& st, const bf16_t* __restrict__ src, long long stride, int row0, int nrows,
                                         int tid) {
    constexpr int CPR = ApStage<HD>::CPR, TOTAL = ApStage<HD>::TOTAL;
#pragma unroll
    for (int u = 0; u < ApStage<HD>::NCH; ++u) {
        const int idx = (tid + u * AP_THREADS) & (TOTAL - 1), r = idx / CPR, ch = idx - r * CPR;
        const int rr = row0 + r < nrows ? row0 + r : nrows - 1;
        st.v[u] = *reinterpret_cast<const uint4*>(src + rr * stride + ch * 8);
    }
}

template <int HD, bool SWZ>
__device__ __forceinline__ void ap_lstore(const ApStage<HD>& st, char* img, int row0, int nrows, int tid) {
    constexpr int CPR = ApStage<HD>::CPR, TOTAL = ApStage<HD>::TOTAL;
#pragma unroll
    for (int u = 0; u < ApStage<HD>::NCH; ++u) {
        const int idx = tid + u * AP_THREADS, r = idx / CPR, ch = idx - r * CPR;
        if (idx < TOTAL)
            *reinterpret_cast<uint4*>(img + ap_off<HD, SWZ>(r, ch)) = row0 + r < nrows ? st.v[u] : make_uint4(0u, 0u, 0u, 0u);
    }
}

struct ApItem {
    const bf16_t *q, *k, *v;     // row 0 of the item's Q, K, V (rows 3c apart)
    long long o;                 // element offset of row 0 in a c-channel tensor (rows c apart)
    long long l;                 // element offset of row 0 in lse
};
__device__ __forceinline__ ApItem ap_item(const bf16_t* qkv, long long item, int c, int nq, int heads, int hd) {
    const long long head = item % heads, slice = item / heads;
    ApItem it;
    it.q = qkv + slice * nq * 3 * c + head * hd;
    it.k = it.q + c;
    it.v = it.q + 2 * c;
    it.o = slice * nq * c + head * hd;
    it.l = item * nq;
    return it;
}

// grid: query blocks x items (the blocks of one item adjacent: they stream the same K and V); block: 256.  No wave leaves early
// and no lane is masked around the transposing reads (they need EXEC all ones).
template <int HD>
__global__ void __launch_bounds__(AP_THREADS)
attn_plane_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, float* __restrict__ lse, int c, int nq, int heads,
                      int qblocks) {
    extern __shared__ __attribute__((aligned(16))) char ap_smem[];
    constexpr int RS = HD * 2 + 32, CT = (HD + 15) / 16;   // hd == 8: the upper half of the one channel tile is padding
    constexpr int KB = ap_img_bytes<HD, true>(), BUF = KB + ap_img_bytes<HD, false>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, kg = lane >> 4;
    const long long item = blockIdx.x / qblocks;
    const int qb = (int)(blockIdx.x - item * qblocks);
    const ApItem it = ap_item(qkv, item, c, nq, heads, HD);
    const long long row = 3ll * c;
    const int qi = qb * AP_TILE + wave * 16 + r16;
    ApFrag<HD> qf;
    ap_load<HD>(qf, it.q + (qi < nq ? qi : nq - 1) * row, kg);
    const int nt = (nq + AP_TILE - 1) / AP_TILE;
    ApStage<HD> ks, vs;
    ap_gload<HD>(ks, it.k, row, 0, nq, tid);
    ap_gload<HD>(vs, it.v, row, 0, nq, tid);
    ap_lstore<HD, true>(ks, ap_smem, 0, nq, tid);
    ap_lstore<HD, false>(vs, ap_smem + KB, 0, nq, tid);
    __syncthreads();
    const unsigned toff = (unsigned)((4 * kg + (r16 >> 2)) * RS + (r16 & 3) * 8);
    const float sc = AP_LOG2E * rsqrtf((float)HD);
    float m = AP_NEG_INF, l = 0.0f;
    f32x4 o[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) o[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = 0; t < nt; ++t) {
        const char* kimg = ap_smem + (t & 1) * BUF;
        const unsigned vaddr = (unsigned)(unsigned long long)(kimg + KB) + toff;
        const bool more = t + 1 < nt;                              // block-uniform
        if (more) {                                                // tile t + 1 travels under tile t's arithmetic
            ap_gload<HD>(ks, it.k, row, (t + 1) * AP_TILE, nq, tid);
            ap_gload<HD>(vs, it.v, row, (t + 1) * AP_TILE, nq, tid);
        }
        f32x4 s[4];
        float bm = AP_NEG_INF;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int key0 = t * AP_TILE + tt * 16;
            s[tt] = f32x4{AP_NEG_INF, AP_NEG_INF, AP_NEG_INF, AP_NEG_INF};
            if (key0 < nq) {                                       // wave-uniform
                ApFrag<HD> kf;
                ap_load_lds<HD, true>(kf, kimg, tt * 16 + r16, kg);
                const f32x4 acc = ap_dot<HD>(kf, qf);              // [key 4 kg + i][query r16]
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    s[tt][i] = (key0 + 4 * kg + i < nq) ? acc[i] * sc : AP_NEG_INF;
                    bm = fmaxf(bm, s[tt][i]);
                }
            }
        }
        const float mn = fmaxf(m, ap_max_kg(bm));                  // finite: every tile holds a real key
        const float alpha = __builtin_amdgcn_exp2f(m - mn);        // first tile: exp2(-inf) = 0 on zeros
        l *= alpha;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) o[ct] *= alpha;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int key0 = t * AP_TILE + tt * 16;
            if (key0 < nq) {
                float p[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    p[i] = __builtin_amdgcn_exp2f(s[tt][i] - mn);
                    l += p[i];
                }
                const ap_s16x4 pb = ap_pack4(p[0], p[1], p[2], p[3]);   // P^T[key 4 kg + j][query r16]
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const ap_s16x4 vt = ap_tr_read(vaddr + (unsigned)(tt * 16 * RS + ct * 32));   // V^T[ch 16 ct + r16][key 4 kg + j]
                    o[ct] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vt, pb, o[ct], 0, 0, 0);
                }
            }
        }
        m = mn;
        if (more) {
            char* nimg = ap_smem + ((t + 1) & 1) * BUF;
            ap_lstore<HD, true>(ks, nimg, (t + 1) * AP_TILE, nq, tid);
            ap_lstore<HD, false>(vs, nimg + KB, (t + 1) * AP_TILE, nq, tid);
        }
        __syncthreads();
    }
    const float lsum = ap_sum_kg(l), linv = 1.0f / lsum;
    if (lse != nullptr && kg == 0 && qi < nq) lse[it.l + qi] = (m + __log2f(lsum)) * AP_LN2;
    if (qi < nq && 4 * kg < HD) {
        // o[ct][i] = O[query r16][channel 16 ct + 4 kg + i]
        bf16_t* op = out + it.o + (long long)qi * c + 4 * kg;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            uint2 v;
            v.x = pack_bf16x2(o[ct][0] * linv, o[ct][1] * linv);
            v.y = pack_bf16x2(o[ct][2] * linv, o[ct][3] * linv);
            *reinterpret_cast<uint2*>(op + ct * 16) = v;
        }
    }
}

// Backward, query-block pass: the forward's frame (one workgroup = 64 queries, K / V tiles streamed); writes the q third of dqkv.
template <int HD>
__global__ void __launch_bounds__(AP_THREADS)
attn_plane_dq_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out, const bf16_t* __restrict__ da,
                     const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int c, int nq, int heads, int qblocks) {
    extern __shared__ __attribute__((aligned(16))) char ap_smem[];
    constexpr int RS = HD * 2 + 32, CT = (HD + 15) / 16;
    constexpr int KB = ap_img_bytes<HD, false>(), BUF = KB + ap_img_bytes<HD, true>();   // K padded (two kinds of read), V swizzled
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, kg = lane >> 4;
    const long long item = blockIdx.x / qblocks;
    const int qb = (int)(blockIdx.x - item * qblocks);
    const ApItem it = ap_item(qkv, item, c, nq, heads, HD);
    const long long row = 3ll * c;
    const int qi = qb * AP_TILE + wave * 16 + r16, qr = qi < nq ? qi : nq - 1;
    ApFrag<HD> qf, df, af;
    ap_load<HD>(qf, it.q + qr * row, kg);
    ap_load<HD>(df, da + it.o + (long long)qr * c, kg);
    ap_load<HD>(af, out + it.o + (long long)qr * c, kg);
    const float lse2 = lse[it.l + qr] * AP_LOG2E;
    const int nt = (nq + AP_TILE - 1) / AP_TILE;
    ApStage<HD> ks, vs;
    ap_gload<HD>(ks, it.k, row, 0, nq, tid);
    ap_gload<HD>(vs, it.v, row, 0, nq, tid);
    ap_lstore<HD, false>(ks, ap_smem, 0, nq, tid);
    ap_lstore<HD, true>(vs, ap_smem + KB, 0, nq, tid);
    __syncthreads();
    const float dl = ap_sum_kg(ap_elem_dot<HD>(df, af));          // delta = rowsum(dA o A), A as stored
    const unsigned toff = (unsigned)((4 * kg + (r16 >> 2)) * RS + (r16 & 3) * 8);
    const float rs = rsqrtf((float)HD), sc = AP_LOG2E * rs;
    f32x4 dq[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) dq[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = 0; t < nt; ++t) {
        const char* kimg = ap_smem + (t & 1) * BUF;
        const char* vimg = kimg + KB;
        const unsigned kaddr = (unsigned)(unsigned long long)kimg + toff;
        const bool more = t + 1 < nt;
        if (more) {
            ap_gload<HD>(ks, it.k, row, (t + 1) * AP_TILE, nq, tid);
            ap_gload<HD>(vs, it.v, row, (t + 1) * AP_TILE, nq, tid);
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int key0 = t * AP_TILE + tt * 16;
            if (key0 < nq) {                                       // wave-uniform
                ApFrag<HD> kf, vf;
                ap_load_lds<HD, false>(kf, kimg, tt * 16 + r16, kg);
                ap_load_lds<HD, true>(vf, vimg, tt * 16 + r16, kg);
                const f32x4 acc = ap_dot<HD>(kf, qf);              // S^T[key 4 kg + i][query r16]
                const f32x4 dpt = ap_dot<HD>(vf, df);              // dP^T
                float ds[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = (key0 + 4 * kg + i < nq) ? __builtin_amdgcn_exp2f(acc[i] * sc - lse2) : 0.0f;
                    ds[i] = p * (dpt[i] - dl);
                }
                const ap_s16x4 dsb = ap_pack4(ds[0], ds[1], ds[2], ds[3]);   // dS^T[key 4 kg + j][query r16]
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const ap_s16x4 kt = ap_tr_read(kaddr + (unsigned)(tt * 16 * RS + ct * 32));   // K^T[ch][key]
                    dq[ct] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kt, dsb, dq[ct], 0, 0, 0);
                }
            }
        }
        if (more) {
            char* nimg = ap_smem + ((t + 1) & 1) * BUF;
            ap_lstore<HD, false>(ks, nimg, (t + 1) * AP_TILE, nq, tid);
            ap_lstore<HD, true>(vs, nimg + KB, (t + 1) * AP_TILE, nq, tid);
        }
        __syncthreads();
    }
    if (qi < nq && 4 * kg < HD) {
        bf16_t* op = dqkv + (it.q - qkv) + qi * row + 4 * kg;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            uint2 v;
            v.x = pack_bf16x2(dq[ct][0] * rs, dq[ct][1] * rs);
            v.y = pack_bf16x2(dq[ct][2] * rs, dq[ct][3] * rs);
            *reinterpret_cast<uint2*>(op + ct * 16) = v;
        }
    }
}

// the HD / 4 channels of one query row's dA and A that one of its four threads sums for delta
template <int HD> struct ApDelta { uint32_t a[HD / 8], o[HD / 8]; };

template <int HD>
__device__ __forceinline__ void ap_delta_load(ApDelta<HD>& dd, const bf16_t* __restrict__ da_row, const bf16_t* __restrict__ o_row,
                                              int part) {
    constexpr int NDW = HD / 8;
    const uint32_t* pa = reinterpret_cast<const uint32_t*>(da_row + part * (HD / 4));
    const uint32_t* po = reinterpret_cast<const uint32_t*>(o_row + part * (HD / 4));
    if constexpr (NDW >= 4) {
#pragma unroll
        for (int j = 0; j < NDW / 4; ++j) {
            const uint4 x = reinterpret_cast<const uint4*>(pa)[j], y = reinterpret_cast<const uint4*>(po)[j];
            dd.a[4 * j] = x.x, dd.a[4 * j + 1] = x.y, dd.a[4 * j + 2] = x.z, dd.a[4 * j + 3] = x.w;
            dd.o[4 * j] = y.x, dd.o[4 * j + 1] = y.y, dd.o[4 * j + 2] = y.z, dd.o[4 * j + 3] = y.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < NDW; ++j) dd.a[j] = pa[j], dd.o[j] = po[j];
    }
}

template <int HD>
__device__ __forceinline__ float ap_delta_sum(const ApDelta<HD>& dd) {   // over the row's four threads (adjacent lanes)
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < HD / 8; ++j) {
        s += __uint_as_float(dd.a[j] << 16) * __uint_as_float(dd.o[j] << 16);
        s += __uint_as_float(dd.a[j] & 0xffff0000u) * __uint_as_float(dd.o[j] & 0xffff0000u);
    }
    s += __shfl_xor(s, 1);
    return s + __shfl_xor(s, 2);
}

// Backward, key-block pass: one workgroup = 64 keys (16 per wave, fragments in registers), Q / dA tiles of 64 queries streamed;
// plain layout S = Q K^T (lane = key r16, registers = queries 4 kg + i), whose accumulator is the B operand of the products
// that sum over the QUERY.  Writes the k and v thirds of dqkv.  LDS buffer: Q image, dA image, lse log2 e [64], delta [64].
template <int HD>
__global__ void __launch_bounds__(AP_THREADS)
attn_plane_dkv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out, const bf16_t* __restrict__ da,
                      const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int c, int nq, int heads, int kblocks) {
    extern __shared__ __attribute__((aligned(16))) char ap_smem[];
    constexpr int RS = HD * 2 + 32, CT = (HD + 15) / 16;
    constexpr int IB = ap_img_bytes<HD, false>(), BUF = 2 * IB + 2 * AP_TILE * 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, kg = lane >> 4;
    const long long item = blockIdx.x / kblocks;
    const int kb = (int)(blockIdx.x - item * kblocks);
    const ApItem it = ap_item(qkv, item, c, nq, heads, HD);
    const long long row = 3ll * c;
    const bf16_t* dab = da + it.o;
    const bf16_t* ob = out + it.o;
    const int ki = kb * AP_TILE + wave * 16 + r16, kr = ki < nq ? ki : nq - 1;
    ApFrag<HD> kc, vc;
    ap_load<HD>(kc, it.k + kr * row, kg);
    ap_load<HD>(vc, it.v + kr * row, kg);
    const int nt = (nq + AP_TILE - 1) / AP_TILE;
    const int srow = tid >> 2, spart = tid & 3;                   // delta: four threads per query row of the tile
    ApStage<HD> qs, as;
    ApDelta<HD> dd;
    float lreg = 0.0f;
    auto gload = [&](int t) {
        const int r0 = t * AP_TILE;
        ap_gload<HD>(qs, it.q, row, r0, nq, tid);
        ap_gload<HD>(as, dab, (long long)c, r0, nq, tid);
        const int sr = r0 + srow < nq ? r0 + srow : nq - 1;
        ap_delta_load<HD>(dd, dab + (long long)sr * c, ob + (long long)sr * c, spart);
        if (tid < AP_TILE) lreg = lse[it.l + (r0 + tid < nq ? r0 + tid : nq - 1)];
    };
    auto lstore = [&](int t) {
        char* img = ap_smem + (t & 1) * BUF;
        ap_lstore<HD, false>(qs, img, t * AP_TILE, nq, tid);
        ap_lstore<HD, false>(as, img + IB, t * AP_TILE, nq, tid);
        float* st = reinterpret_cast<float*>(img + 2 * IB);
        const float dl = ap_delta_sum<HD>(dd);                     // every lane takes part in the shuffles
        if (spart == 0) st[AP_TILE + srow] = dl;
        if (tid < AP_TILE) st[tid] = lreg * AP_LOG2E;
    };
    gload(0);
    lstore(0);
    __syncthreads();
    const unsigned toff = (unsigned)((4 * kg + (r16 >> 2)) * RS + (r16 & 3) * 8);
    const float rs = rsqrtf((float)HD), sc = AP_LOG2E * rs;
    f32x4 dv[CT], dk[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) dv[ct] = dk[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = 0; t < nt; ++t) {
        const char* qimg = ap_smem + (t & 1) * BUF;
        const char* aimg = qimg + IB;
        const float* st = reinterpret_cast<const float*>(qimg + 2 * IB);
        const unsigned qaddr = (unsigned)(unsigned long long)qimg + toff, aaddr = qaddr + IB;
        const bool more = t + 1 < nt;
        if (more) gload(t + 1);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int q0 = t * AP_TILE + tt * 16;
            if (q0 < nq) {                                         // wave-uniform
                ApFrag<HD> qf, df;
                ap_load_lds<HD, false>(qf, qimg, tt * 16 + r16, kg);
                ap_load_lds<HD, false>(df, aimg, tt * 16 + r16, kg);
                const f32x4 sacc = ap_dot<HD>(qf, kc);             // S[query 4 kg + i][key r16]
                const f32x4 dpa = ap_dot<HD>(df, vc);              // dP[query 4 kg + i][key r16]
                const float4 lq = *reinterpret_cast<const float4*>(st + tt * 16 + 4 * kg);
                const float4 dq_ = *reinterpret_cast<const float4*>(st + AP_TILE + tt * 16 + 4 * kg);
                const float lv[4] = {lq.x, lq.y, lq.z, lq.w}, dlv[4] = {dq_.x, dq_.y, dq_.z, dq_.w};
                float p[4], ds[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool ok = (q0 + 4 * kg + i < nq) && (ki < nq);
                    p[i] = ok ? __builtin_amdgcn_exp2f(sacc[i] * sc - lv[i]) : 0.0f;
                    ds[i] = ok ? p[i] * (dpa[i] - dlv[i]) : 0.0f;
                }
                const ap_s16x4 pb = ap_pack4(p[0], p[1], p[2], p[3]);       // P[query 4 kg + j][key r16]
                const ap_s16x4 dsb = ap_pack4(ds[0], ds[1], ds[2], ds[3]);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const ap_s16x4 at = ap_tr_read(aaddr + (unsigned)(tt * 16 * RS + ct * 32));   // dA^T[ch][query]
                    const ap_s16x4 qt = ap_tr_read(qaddr + (unsigned)(tt * 16 * RS + ct * 32));   // Q^T[ch][query]
                    dv[ct] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(at, pb, dv[ct], 0, 0, 0);
                    dk[ct] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(qt, dsb, dk[ct], 0, 0, 0);
                }
            }
        }
        if (more) lstore(t + 1);
        __syncthreads();
    }
    if (ki < nq && 4 * kg < HD) {
        bf16_t* kp = dqkv + (it.k - qkv) + ki * row + 4 * kg;
        bf16_t* vp = kp + c;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            uint2 v;
            v.x = pack_bf16x2(dk[ct][0] * rs, dk[ct][1] * rs);
            v.y = pack_bf16x2(dk[ct][2] * rs, dk[ct][3] * rs);
            *reinterpret_cast<uint2*>(kp + ct * 16) = v;
            v.x = pack_bf16x2(dv[ct][0], dv[ct][1]);
            v.y = pack_bf16x2(dv[ct][2], dv[ct][3]);
            *reinterpret_cast<uint2*>(vp + ct * 16) = v;
        }
    }
}

static int ap_check(const char* who, int n, int c, int d, int h, int w, int heads, long long* items, int* blocks) {
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "%s: bad shape n=%d c=%d d=%d h=%d w=%d", who, n, c, d, h, w);
    CTSI_CHECK_ARG(heads > 0 && c % heads == 0, "%s: c=%d is not divisible by heads=%d", who, c, heads);
    const int hd = c / heads;
    CTSI_CHECK_ARG(hd == 8 || hd == 16 || hd == 32 || hd == 64 || hd == 128,
                   "%s: head dimension %d (c=%d / heads=%d) is not supported (8, 16, 32, 64 or 128)", who, hd, c, heads);
    const long long nq = (long long)h * w, it = (long long)n * d * heads, nb = (nq + AP_TILE - 1) / AP_TILE;
    CTSI_CHECK_ARG(nq < (1ll << 24), "%s: plane %d x %d has too many positions", who, h, w);
    CTSI_CHECK_ARG(it * nb < (1ll << 31), "%s: too many blocks (%lld items x %lld blocks)", who, it, nb);
    *items = it;
    *blocks = (int)nb;
    return CTSI_OK;
}

template <int HD>
static void ap_launch_fwd(const bf16_t* qkv, bf16_t* out, float* lse, int c, int nq, int heads, long long items, int nb,
                          hipStream_t st) {
    constexpr int LDS = 2 * (ap_img_bytes<HD, true>() + ap_img_bytes<HD, false>());
    auto k = attn_plane_fwd_kernel<HD>;
    static CtsiPerDeviceOnce attr_once;
    if (LDS > 65536 && attr_once.first()) hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    hipLaunchKernelGGL(k, dim3((unsigned)(items * nb)), dim3(AP_THREADS), LDS, st, qkv, out, lse, c, nq, heads, nb);
}

template <int HD>
static void ap_launch_bwd(const bf16_t* qkv, const bf16_t* out, const bf16_t* da, const float* lse, bf16_t* dqkv, int c, int nq,
                          int heads, long long items, int nb, hipStream_t st) {
    constexpr int LDS_Q = 2 * (ap_img_bytes<HD, true>() + ap_img_bytes<HD, false>());
    constexpr int LDS_K = 2 * (2 * ap_img_bytes<HD, false>() + 2 * AP_TILE * 4);
    auto kq = attn_plane_dq_kernel<HD>;
    auto kk = attn_plane_dkv_kernel<HD>;
    static CtsiPerDeviceOnce attr_once;
    if ((LDS_Q > 65536 || LDS_K > 65536) && attr_once.first()) {
        hipFuncSetAttribute((const void*)kq, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_Q);
        hipFuncSetAttribute((const void*)kk, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_K);
    }
    hipLaunchKernelGGL(kq, dim3((unsigned)(items * nb)), dim3(AP_THREADS), LDS_Q, st, qkv, out, da, lse, dqkv, c, nq, heads, nb);
    hipLaunchKernelGGL(kk, dim3((unsigned)(items * nb)), dim3(AP_THREADS), LDS_K, st, qkv, out, da, lse, dqkv, c, nq, heads, nb);
}

extern "C" int ctsi_attn_plane(const void* qkv, void* out, float* lse, int n, int c, int d, int h, int w, int heads,
                               void* stream) {
    CTSI_CHECK_ARG(qkv && out, "ctsi_attn_plane: null argument");
    long long items = 0;
    int nb = 0;
    const int rc = ap_check("ctsi_attn_plane", n, c, d, h, w, heads, &items, &nb);
    if (rc != CTSI_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
#define AP_FWD(HD_) ap_launch_fwd<HD_>((const bf16_t*)qkv, (bf16_t*)out, lse, c, h * w, heads, items, nb, st)
    switch (c / heads) {
        case 8: AP_FWD(8); break;
        case 16: AP_FWD(16); break;
        case 32: AP_FWD(32); break;
        case 64: AP_FWD(64); break;
        default: AP_FWD(128); break;
    }
#undef AP_FWD
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_attn_plane_bwd(const void* qkv, const void* out, const void* da, const float* lse, void* dqkv, int n, int c,
                                   int d, int h, int w, int heads, void* stream) {
    CTSI_CHECK_ARG(qkv && out && da && lse && dqkv, "ctsi_attn_plane_bwd: null argument");
    long long items = 0;
    int nb = 0;
    const int rc = ap_check("ctsi_attn_plane_bwd", n, c, d, h, w, heads, &items, &nb);
    if (rc != CTSI_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
#define AP_BWD(HD_)                                                                                                         \
    ap_launch_bwd<HD_>((const bf16_t*)qkv, (const bf16_t*)out, (const bf16_t*)da, lse, (bf16_t*)dqkv, c, h * w, heads, items, \
                       nb, st)
    switch (c / heads) {
        case 8: AP_BWD(8); break;
        case 16: AP_BWD(16); break;
        case 32: AP_BWD(32); break;
        case 64: AP_BWD(64); break;
        default: AP_BWD(128); break;
    }
#undef AP_BWD
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
