// True depth attention: A = softmax(Q K^T / sqrt(hd)) V over the D depth positions of one (sample, position, head), forward
// and backward (attention_mode='softmax'; attention.hip has the reference's degenerate einsum the other two modes reproduce).
//
// qkv is the bf16 NDHWC output of the block's 1x1x1 conv C -> 3C: channels [q | k | v], heads split inside each third.  One
// work item = one (sample, position, head): Q, K, V are D x hd, rows H*W*3C elements apart, channels contiguous.  One wave owns
// one item; a block is up to four waves (the heads of one position when heads == 4: adjacent channels of the same rows).
//
// Operand path.  Every product whose K dimension is the channel (Q K^T, dA V^T) reads both operands straight from global
// memory in MFMA operand layout: lane (r16, kg) takes 8 consecutive channels 8 kg .. 8 kg + 7 of row r16 of a 16-row tile
// (v_mfma_f32_16x16x32_bf16; hd <= 16: 4 channels, v_mfma_f32_16x16x16_bf16, zero-padded at hd == 8).  The score tile is computed TRANSPOSED,
// S^T = K Q^T, so that its accumulator layout -- lane = query r16, registers = keys 4 kg .. 4 kg + 3 -- is, rounded to bf16, the
// B operand of a 16x16x16 MFMA whose K dimension is the key: O^T = V^T P^T needs no lane movement for P.  The other operand
// of such a product (V^T here; K^T, dA^T, Q^T in the backward) must have its 4 keys in one lane: the tensor is staged once per
// item in LDS as it lies in memory ([row][hd] bf16, rows padded by 32 bytes: the 8 rows a 32-lane half reads fall on distinct
// banks) and read with gfx950's transposing ds_read_b64_tr_b16 -- a 16-lane group fetches 4 rows x 16 channels and each lane
// receives its channel's 4 rows.  The result tile O^T has 4 consecutive channels of one query per lane: 8-byte stores, and the
// softmax statistics of a query live in the lanes that hold it (reduced over kg with two DPP-free shuffles).
//
// Softmax: fp32, scores scaled by log2(e) / sqrt(hd) and exponentiated with v_exp_f32 (exp2); keys beyond D are -inf before the
// max, padded queries are computed on a clamped row and never stored.  Keys are walked in blocks of 64 (4 score tiles in
// registers) with an online max / sum; D <= 64 is one block, i.e. a single pass per query tile.
//
// Backward (dqkv from qkv and dA; S and P are recomputed): phase A works per query tile in the transposed layout -- row max and
// sum, delta = sum_k P dP (== rowsum(dA o A)), dS = P o (dP - delta), dQ^T = K^T dS^T / sqrt(hd) -- and leaves (max, 1 / sum,
// delta) per query in LDS; phase B works per key tile in the plain layout S = Q K^T (lane = key, registers = queries), whose
// accumulator is the B operand of products that sum over the QUERY: dV^T = dA^T P, dK^T = Q^T dS / sqrt(hd).
#include "ctsi_internal.h"

typedef __attribute__((ext_vector_type(4))) short ac_s16x4;
typedef ac_s16x4 __attribute__((address_space(3))) * ac_lds_ptr;
__device__ __forceinline__ ac_s16x4 ac_tr_read(unsigned lds_addr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((ac_lds_ptr)(unsigned long long)lds_addr);
}

#define AC_NEG_INF (-__builtin_inff())

// operand fragments of one 16-row tile over the hd channels (K dimension = channel)
template <int HD> struct AcFrag { bf16x8 v[HD / 32]; };
template <> struct AcFrag<16> { ac_s16x4 v[1]; };
template <> struct AcFrag<8> { ac_s16x4 v[1]; };      // channels 8 .. 15 of the K = 16 step are zero

template <int HD>
__device__ __forceinline__ void ac_load(AcFrag<HD>& f, const bf16_t* __restrict__ rowp, int kg) {
    if constexpr (HD == 8) {
        f.v[0] = ac_s16x4{0, 0, 0, 0};
        if (kg < 2) f.v[0] = *reinterpret_cast<const ac_s16x4*>(rowp + kg * 4);
    } else if constexpr (HD == 16) {
        f.v[0] = *reinterpret_cast<const ac_s16x4*>(rowp + kg * 4);
    } else {
#pragma unroll
        for (int s = 0; s < HD / 32; ++s) f.v[s] = *reinterpret_cast<const bf16x8*>(rowp + s * 32 + kg * 8);
    }
}

// C[row of a][row of b] = sum_ch a[.][ch] b[.][ch]
template <int HD>
__device__ __forceinline__ f32x4 ac_dot(const AcFrag<HD>& a, const AcFrag<HD>& b) {
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (HD <= 16) {
        acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a.v[0], b.v[0], acc, 0, 0, 0);
    } else {
#pragma unroll
        for (int s = 0; s < HD / 32; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v[s], b.v[s], acc, 0, 0, 0);
    }
    return acc;
}

__device__ __forceinline__ ac_s16x4 ac_pack4(float a, float b, float c, float d) {
    union { ac_s16x4 v; uint32_t u[2]; } r;
    r.u[0] = pack_bf16x2(a, b);
    r.u[1] = pack_bf16x2(c, d);
    return r.v;
}

__device__ __forceinline__ float ac_max_kg(float v) {   // over the four lanes r16, r16 + 16, r16 + 32, r16 + 48
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float ac_sum_kg(float v) {
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

// LDS image of a D x hd tensor: row stride hd * 2 + 32 bytes, rows d .. dp - 1 zero.  Eight 16-byte loads per lane are issued
// before the first LDS store (unconditional loads from clamped rows): one memory latency per 8 KB, not one per KB.
template <int HD>
__device__ __forceinline__ void ac_stage(char* img, const bf16_t* __restrict__ src, long long row, int d, int dp, int lane) {
    constexpr int CPR = HD / 8, RS = HD * 2 + 32;
    const int total = dp * CPR;
    for (int base = lane; base < total; base += 512) {
        uint4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = base + u * 64, r = idx / CPR, ch = idx - r * CPR;
            v[u] = *reinterpret_cast<const uint4*>(src + (r < d ? r : d - 1) * row + ch * 8);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = base + u * 64, r = idx / CPR, ch = idx - r * CPR;
            if (idx < total) *reinterpret_cast<uint4*>(img + r * RS + ch * 16) = r < d ? v[u] : make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

// the fragments of the four 16-row tiles of one 64-row block of `src`, rows beyond d clamped (their products are masked):
// unconditional loads, so that all of them are in flight before the first MFMA waits
template <int HD>
__device__ __forceinline__ void ac_load_block(AcFrag<HD> (&f)[4], const bf16_t* __restrict__ src, long long row, int r0, int d,
                                              int r16, int kg) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = r0 + t * 16 + r16;
        ac_load<HD>(f[t], src + (r < d ? r : d - 1) * row, kg);
    }
}

// grid: ceil(items / waves per block); block: 64 * waves per block.  No wave leaves early and no lane is masked around the
// transposing reads (they need EXEC all ones): a wave beyond the last item redoes the last one and stores nothing.
// Loads: the K fragments of a 64-key block (d <= 64: of the item, once), the first query tile and the V image are all issued
// before anything waits; the next query tile's fragments are loaded while the current one is computed.
template <int HD>
__global__ void __launch_bounds__(256)
attn_core_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int c, int d, long long hw, int heads,
                     long long items, unsigned lds_per_wave) {
    extern __shared__ __attribute__((aligned(16))) char ac_smem[];
    constexpr int RS = HD * 2 + 32, CT = (HD + 15) / 16;   // hd == 8: the upper half of the one channel tile is padding
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    long long item = (long long)blockIdx.x * wpb + wave;
    const bool live = item < items;
    if (!live) item = items - 1;
    const int head = (int)(item % heads);
    const long long np = item / heads, pos = np % hw, nb = np / hw;
    const long long row = hw * 3 * c, orow = hw * c;
    const bf16_t* qb = qkv + ((nb * d) * hw + pos) * 3 * c + head * HD;
    const bf16_t* kb_ = qb + c;
    const bf16_t* vb = qb + 2 * c;
    bf16_t* ob = out + ((nb * d) * hw + pos) * c + head * HD;
    char* vimg = ac_smem + (size_t)wave * lds_per_wave;
    const int dp = (d + 15) & ~15;
    const int nkb = (d + 63) >> 6;
    const bool single = nkb == 1;
    AcFrag<HD> kf[4], qf, qn;
    if (single) ac_load_block<HD>(kf, kb_, row, 0, d, r16, kg);
    ac_load<HD>(qf, qb + (r16 < d ? r16 : d - 1) * row, kg);
    ac_stage<HD>(vimg, vb, row, d, dp, lane);
    __syncthreads();
    const unsigned vaddr = (unsigned)(unsigned long long)vimg + (unsigned)((4 * kg + (r16 >> 2)) * RS + (r16 & 3) * 8);
    const float sc = 1.4426950408889634f * rsqrtf((float)HD);
    for (int q0 = 0; q0 < dp; q0 += 16) {
        const int qi = q0 + r16, qnext = qi + 16;
        qn = qf;
        if (q0 + 16 < dp) ac_load<HD>(qn, qb + (qnext < d ? qnext : d - 1) * row, kg);     // wave-uniform
        float m = AC_NEG_INF, l = 0.0f;
        f32x4 o[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) o[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int kb = 0; kb < nkb; ++kb) {
            if (!single) ac_load_block<HD>(kf, kb_, row, kb * 64, d, r16, kg);
            f32x4 s[4];
            float bm = AC_NEG_INF;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int key0 = kb * 64 + t * 16;
                s[t] = f32x4{AC_NEG_INF, AC_NEG_INF, AC_NEG_INF, AC_NEG_INF};
                if (key0 < d) {                                        // wave-uniform
                    const f32x4 acc = ac_dot<HD>(kf[t], qf);            // [key 4 kg + i][query r16]
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        s[t][i] = (key0 + 4 * kg + i < d) ? acc[i] * sc : AC_NEG_INF;
                        bm = fmaxf(bm, s[t][i]);
                    }
                }
            }
            const float mn = fmaxf(m, ac_max_kg(bm));                  // finite: every block holds a real key
            const float alpha = __builtin_amdgcn_exp2f(m - mn);        // first block: exp2(-inf) = 0 on zeros
            l *= alpha;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) o[ct] *= alpha;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int key0 = kb * 64 + t * 16;
                if (key0 < d) {
                    float p[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        p[i] = __builtin_amdgcn_exp2f(s[t][i] - mn);
                        l += p[i];
                    }
                    const ac_s16x4 pb = ac_pack4(p[0], p[1], p[2], p[3]);   // P^T[key 4 kg + j][query r16]
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        const ac_s16x4 vt = ac_tr_read(vaddr + (unsigned)(key0 * RS + ct * 32));   // V^T[ch 16 ct + r16][key 4 kg + j]
                        o[ct] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(vt, pb, o[ct], 0, 0, 0);
                    }
                }
            }
            m = mn;
        }
        const float linv = 1.0f / ac_sum_kg(l);
        if (live && qi < d && 4 * kg < HD) {
            // o[ct][i] = O[query r16][channel 16 ct + 4 kg + i]
            bf16_t* op = ob + qi * orow + 4 * kg;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                uint2 v;
                v.x = pack_bf16x2(o[ct][0] * linv, o[ct][1] * linv);
                v.y = pack_bf16x2(o[ct][2] * linv, o[ct][3] * linv);
                *reinterpret_cast<uint2*>(op + ct * 16) = v;
            }
        }
        qf = qn;
    }
}

// LDS per wave: image 0 (K, then dA), image 1 (Q), then [max | 1 / sum | delta] x dp floats.
template <int HD>
__global__ void __launch_bounds__(256)
attn_core_bwd_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ da, bf16_t* __restrict__ dqkv, int c, int d,
                     long long hw, int heads, long long items, unsigned lds_per_wave) {
    extern __shared__ __attribute__((aligned(16))) char ac_smem[];
    constexpr int RS = HD * 2 + 32, CT = (HD + 15) / 16;   // hd == 8: the upper half of the one channel tile is padding
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    long long item = (long long)blockIdx.x * wpb + wave;
    const bool live = item < items;
    if (!live) item = items - 1;
    const int head = (int)(item % heads);
    const long long np = item / heads, pos = np % hw, nb = np / hw;
    const long long row = hw * 3 * c, arow = hw * c;
    const long long off3 = ((nb * d) * hw + pos) * 3 * c + head * HD;
    const bf16_t* qb = qkv + off3;
    const bf16_t* kb_ = qb + c;
    const bf16_t* vb = qb + 2 * c;
    const bf16_t* ab = da + ((nb * d) * hw + pos) * c + head * HD;
    bf16_t* dqb = dqkv + off3;
    const int dp = (d + 15) & ~15;
    char* img0 = ac_smem + (size_t)wave * lds_per_wave;
    char* img1 = img0 + dp * RS;
    float* st_m = reinterpret_cast<float*>(img1 + dp * RS);
    float* st_li = st_m + dp;
    float* st_dl = st_li + dp;
    const int nkb = (d + 63) >> 6;
    const bool single = nkb == 1;            // d <= 64: K / V fragments, scores and dP stay in registers over the three passes
    AcFrag<HD> kf[4], vf[4], qf, df, qn, dn;
    if (single) {
        ac_load_block<HD>(kf, kb_, row, 0, d, r16, kg);
        ac_load_block<HD>(vf, vb, row, 0, d, r16, kg);
    }
    ac_load<HD>(qf, qb + (r16 < d ? r16 : d - 1) * row, kg);
    ac_load<HD>(df, ab + (r16 < d ? r16 : d - 1) * arow, kg);
    ac_stage<HD>(img0, kb_, row, d, dp, lane);
    ac_stage<HD>(img1, qb, row, d, dp, lane);
    __syncthreads();
    const unsigned toff = (unsigned)((4 * kg + (r16 >> 2)) * RS + (r16 & 3) * 8);
    const unsigned a0 = (unsigned)(unsigned long long)img0 + toff, a1 = (unsigned)(unsigned long long)img1 + toff;
    const float rs = rsqrtf((float)HD), sc = 1.4426950408889634f * rs;

    // ---- phase A: per query tile, transposed layout (lane = query r16, registers = keys 4 kg + i) -------------------------
    for (int q0 = 0; q0 < dp; q0 += 16) {
        const int qi = q0 + r16, qx = qi + 16 < d ? qi + 16 : d - 1;
        qn = qf;
        dn = df;
        if (q0 + 16 < dp) {                  // wave-uniform: the next tile's fragments travel under this tile's arithmetic
            ac_load<HD>(qn, qb + qx * row, kg);
            ac_load<HD>(dn, ab + qx * arow, kg);
        }
        f32x4 s[4], dpt[4];
        auto calc = [&](int kb, bool with_dp) {      // scaled scores (-inf beyond d) and dP^T[key][query] of key block kb
            if (!single) {
                ac_load_block<HD>(kf, kb_, row, kb * 64, d, r16, kg);
                if (with_dp) ac_load_block<HD>(vf, vb, row, kb * 64, d, r16, kg);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int key0 = kb * 64 + t * 16;
                s[t] = f32x4{AC_NEG_INF, AC_NEG_INF, AC_NEG_INF, AC_NEG_INF};
                dpt[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (key0 < d) {
                    const f32x4 acc = ac_dot<HD>(kf[t], qf);
#pragma unroll
                    for (int i = 0; i < 4; ++i) s[t][i] = (key0 + 4 * kg + i < d) ? acc[i] * sc : AC_NEG_INF;
                    if (with_dp) dpt[t] = ac_dot<HD>(vf[t], df);
                }
            }
        };
        if (single) calc(0, true);
        float m = AC_NEG_INF, l = 0.0f;
        for (int kb = 0; kb < nkb; ++kb) {
            if (!single) calc(kb, false);
            float bm = AC_NEG_INF;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) bm = fmaxf(bm, s[t][i]);
            const float mn = fmaxf(m, ac_max_kg(bm));
            l *= __builtin_amdgcn_exp2f(m - mn);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) l += __builtin_amdgcn_exp2f(s[t][i] - mn);
            m = mn;
        }
        const float linv = 1.0f / ac_sum_kg(l);
        float dl = 0.0f;
        for (int kb = 0; kb < nkb; ++kb) {
            if (!single) calc(kb, true);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) dl += __builtin_amdgcn_exp2f(s[t][i] - m) * linv * dpt[t][i];
        }
        dl = ac_sum_kg(dl);
        f32x4 dq[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) dq[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int kb = 0; kb < nkb; ++kb) {
            if (!single) calc(kb, true);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int key0 = kb * 64 + t * 16;
                if (key0 < d) {
                    float ds[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        ds[i] = __builtin_amdgcn_exp2f(s[t][i] - m) * linv * (dpt[t][i] - dl);
                    const ac_s16x4 dsb = ac_pack4(ds[0], ds[1], ds[2], ds[3]);   // dS^T[key 4 kg + j][query r16]
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) {
                        const ac_s16x4 kt = ac_tr_read(a0 + (unsigned)(key0 * RS + ct * 32));   // K^T[ch][key]
                        dq[ct] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kt, dsb, dq[ct], 0, 0, 0);
                    }
                }
            }
        }
        if (kg == 0) {
            st_m[qi] = m;
            st_li[qi] = linv;
            st_dl[qi] = dl;
        }
        if (live && qi < d && 4 * kg < HD) {
            bf16_t* op = dqb + qi * row + 4 * kg;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                uint2 v;
                v.x = pack_bf16x2(dq[ct][0] * rs, dq[ct][1] * rs);
                v.y = pack_bf16x2(dq[ct][2] * rs, dq[ct][3] * rs);
                *reinterpret_cast<uint2*>(op + ct * 16) = v;
            }
        }
        qf = qn;
        df = dn;
    }
    __syncthreads();                         // image 0 (K) is done with; the statistics are written
    ac_stage<HD>(img0, ab, arow, d, dp, lane);
    // first (key tile, query tile) of phase B: its fragments travel with the staging loads
    AcFrag<HD> kc, vc;
    ac_load<HD>(kc, kb_ + (r16 < d ? r16 : d - 1) * row, kg);
    ac_load<HD>(vc, vb + (r16 < d ? r16 : d - 1) * row, kg);
    ac_load<HD>(qf, qb + (r16 < d ? r16 : d - 1) * row, kg);
    ac_load<HD>(df, ab + (r16 < d ? r16 : d - 1) * arow, kg);
    __syncthreads();

    // ---- phase B: per key tile, plain layout (lane = key r16, registers = queries 4 kg + i) -------------------------------
    for (int k0 = 0; k0 < dp; k0 += 16) {
        const int ki = k0 + r16;
        f32x4 dv[CT], dk[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) dv[ct] = dk[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int q0 = 0; q0 < dp; q0 += 16) {
            // the next (key tile, query tile)'s query-side fragments are loaded while this one is computed
            const bool more = q0 + 16 < dp || k0 + 16 < dp;
            const int qnx = (q0 + 16 < dp ? q0 + 16 : 0) + r16, qx = qnx < d ? qnx : d - 1;
            qn = qf;
            dn = df;
            if (more) {
                ac_load<HD>(qn, qb + qx * row, kg);
                ac_load<HD>(dn, ab + qx * arow, kg);
            }
            const f32x4 sacc = ac_dot<HD>(qf, kc);     // S[query 4 kg + i][key r16]
            const f32x4 dpa = ac_dot<HD>(df, vc);      // dP[query 4 kg + i][key r16]
            const float4 mq = *reinterpret_cast<const float4*>(st_m + q0 + 4 * kg);
            const float4 lq = *reinterpret_cast<const float4*>(st_li + q0 + 4 * kg);
            const float4 dq_ = *reinterpret_cast<const float4*>(st_dl + q0 + 4 * kg);
            const float mv[4] = {mq.x, mq.y, mq.z, mq.w}, lv[4] = {lq.x, lq.y, lq.z, lq.w};
            const float dlv[4] = {dq_.x, dq_.y, dq_.z, dq_.w};
            float p[4], ds[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool ok = (q0 + 4 * kg + i < d) && (ki < d);
                p[i] = ok ? __builtin_amdgcn_exp2f(sacc[i] * sc - mv[i]) * lv[i] : 0.0f;
                ds[i] = ok ? p[i] * (dpa[i] - dlv[i]) : 0.0f;
            }
            const ac_s16x4 pb = ac_pack4(p[0], p[1], p[2], p[3]);       // P[query 4 kg + j][key r16]
            const ac_s16x4 dsb = ac_pack4(ds[0], ds[1], ds[2], ds[3]);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const ac_s16x4 at = ac_tr_read(a0 + (unsigned)(q0 * RS + ct * 32));   // dA^T[ch][query]
                const ac_s16x4 qt = ac_tr_read(a1 + (unsigned)(q0 * RS + ct * 32));   // Q^T[ch][query]
                dv[ct] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(at, pb, dv[ct], 0, 0, 0);
                dk[ct] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(qt, dsb, dk[ct], 0, 0, 0);
            }
            qf = qn;
            df = dn;
        }
        // the next key tile's own fragments, under this tile's stores
        AcFrag<HD> kn = kc, vn = vc;
        if (k0 + 16 < dp) {
            const int kx = ki + 16 < d ? ki + 16 : d - 1;
            ac_load<HD>(kn, kb_ + kx * row, kg);
            ac_load<HD>(vn, vb + kx * row, kg);
        }
        if (live && ki < d && 4 * kg < HD) {
            bf16_t* kp = dqb + ki * row + c + 4 * kg;
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
        kc = kn;
        vc = vn;
    }
}

#define AC_LDS_LIMIT 65536

static int ac_check(const char* who, int n, int c, int d, int h, int w, int heads, int images, int stat_floats,
                    unsigned* per_wave, int* wpb) {
    CTSI_CHECK_ARG(n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "%s: bad shape n=%d c=%d d=%d h=%d w=%d", who, n, c, d, h, w);
    CTSI_CHECK_ARG(heads > 0 && c % heads == 0, "%s: c=%d is not divisible by heads=%d", who, c, heads);
    const int hd = c / heads;
    CTSI_CHECK_ARG(hd == 8 || hd == 16 || hd == 32 || hd == 64 || hd == 128,
                   "%s: head dimension %d (c=%d / heads=%d) is not supported (8, 16, 32, 64 or 128)", who, hd, c, heads);
    const int dp = (d + 15) & ~15;
    const long long pw = (long long)dp * (images * (hd * 2 + 32) + stat_floats * 4);
    CTSI_CHECK_ARG(pw <= AC_LDS_LIMIT, "%s: depth %d at head dimension %d needs %lld bytes of LDS per item (limit %d)", who, d,
                   hd, pw, AC_LDS_LIMIT);
    CTSI_CHECK_ARG((long long)n * h * w * heads < (1ll << 31), "%s: too many items", who);
    int wv = 4;
    while (wv > 1 && wv * pw > AC_LDS_LIMIT) wv >>= 1;
    *per_wave = (unsigned)pw;
    *wpb = wv;
    return CTSI_OK;
}

extern "C" int ctsi_attn_core(const void* qkv, void* out, int n, int c, int d, int h, int w, int heads, void* stream) {
    CTSI_CHECK_ARG(qkv && out, "ctsi_attn_core: null argument");
    unsigned pw = 0;
    int wpb = 0;
    const int rc = ac_check("ctsi_attn_core", n, c, d, h, w, heads, 1, 0, &pw, &wpb);
    if (rc != CTSI_OK) return rc;
    const long long items = (long long)n * h * w * heads, hw = (long long)h * w;
    const dim3 grid((unsigned)((items + wpb - 1) / wpb)), block(64 * wpb);
    const size_t lds = (size_t)pw * wpb;
    hipStream_t st = (hipStream_t)stream;
#define AC_FWD(HD_) \
    hipLaunchKernelGGL(attn_core_fwd_kernel<HD_>, grid, block, lds, st, (const bf16_t*)qkv, (bf16_t*)out, c, d, hw, heads, items, pw)
    switch (c / heads) {
        case 8: AC_FWD(8); break;
        case 16: AC_FWD(16); break;
        case 32: AC_FWD(32); break;
        case 64: AC_FWD(64); break;
        default: AC_FWD(128); break;
    }
#undef AC_FWD
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_attn_core_bwd(const void* qkv, const void* da, void* dqkv, int n, int c, int d, int h, int w, int heads,
                                  void* stream) {
    CTSI_CHECK_ARG(qkv && da && dqkv, "ctsi_attn_core_bwd: null argument");
    unsigned pw = 0;
    int wpb = 0;
    const int rc = ac_check("ctsi_attn_core_bwd", n, c, d, h, w, heads, 2, 3, &pw, &wpb);
    if (rc != CTSI_OK) return rc;
    const long long items = (long long)n * h * w * heads, hw = (long long)h * w;
    const dim3 grid((unsigned)((items + wpb - 1) / wpb)), block(64 * wpb);
    const size_t lds = (size_t)pw * wpb;
    hipStream_t st = (hipStream_t)stream;
#define AC_BWD(HD_)                                                                                                        \
    hipLaunchKernelGGL(attn_core_bwd_kernel<HD_>, grid, block, lds, st, (const bf16_t*)qkv, (const bf16_t*)da, (bf16_t*)dqkv, \
                       c, d, hw, heads, items, pw)
    switch (c / heads) {
        case 8: AC_BWD(8); break;
        case 16: AC_BWD(16); break;
        case 32: AC_BWD(32); break;
        case 64: AC_BWD(64); break;
        default: AC_BWD(128); break;
    }
#undef AC_BWD
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
