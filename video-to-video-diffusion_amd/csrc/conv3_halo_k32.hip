// 3x3x3 stride-1 convolution, 512-voxel LDS halo tile x 128 couts on v_mfma_f32_16x16x32_bf16: the K = 32 of one MFMA is
// TWO TAPS x 16 channels.
//
// Why this form: the round-1 512-voxel kernel (conv3_halo32m_kernel, 32x32x16 MFMAs; now experiments/conv3_halo_m512.hip) is
// not cycle- but CLOCK-bound on real data -- the same
// launch on all-zero operands runs 26-33 % faster (1236 -> 1579 TFLOP/s for 384->128 @48x128^2; profiles/r02_notes.md), i.e. the
// chip lowers its clock under the MFMA load (MI355X_MICROARCH.md, DVFS give-back) and cycles saved in the issue stream come back
// only in part.  What raises the clock for the same FLOPs: the 16x16x32 MFMA shape (give-back item 7: ~1.12-1.15 x the FLOP/s
// of the 32x32x16 loop at equal cycles) and fewer VALU instructions per MFMA (rule 28).  This kernel keeps conv3_halo32m's
// data movement (16-channel chunks, 32-byte halo rows, double-buffered halo, weight ring fed by LDS-DMA, one barrier per
// step, 128 KB output tile through LDS) and changes the arithmetic:
//   * the (chunk, tap) pairs of a block form ONE linear stream q = chunk * 27 + tap; a *unit* is two consecutive entries
//     (2 x 16 channels = K 32), a *step* two units (4 taps, 16 KB of weights, one barrier).  Lanes 0-31 of an operand read
//     the unit's first tap, lanes 32-63 the second: the tap shift is a per-lane LDS address, so pairs may straddle (kd, kh)
//     rows and chunks (27 taps per chunk is odd); the stream is zero-padded to whole steps in the packed image;
//   * per wave 64 voxels x 128 couts = 4 x 8 tiles of 16x16: 32 MFMAs and 12 ds_read_b128 per unit -- the same LDS bytes per
//     FLOP as the 32x32x16 form -- with every fragment address = one per-lane base + a per-unit tap offset + an immediate
//     (4 VALU per 32 MFMAs instead of ~5 per fragment);
//   * no LDS swizzle: a 16-lane group of a ds_read_b128 covers 16 consecutive 32-byte rows, rows r and r + 8 (same banks)
//     always with DIFFERENT 16-byte halves (group lanes {0-3, 12-15} read half h, {4-11} read half 1 - h), conflict-free as laid
//     out by the DMA.
#include "conv3_halo_common.h"
#include <stdlib.h>
#include <type_traits>

// <TD, TH, TW, BN, UPS>: tile TD x TH x TW = 512 or 384 voxels, BN couts per block, UPS units per step (one barrier per step):
//   <4,4,32,128,2> / <4,8,16,128,2>: per wave 64 voxels x 128 couts (32 MFMAs, 12 ds_read_b128 per unit), steps of 4 entries;
//   <3,4,32,128,2> / <3,8,16,128,2>: 384 voxels, 48 per wave (24 MFMAs, 11 reads per unit) for levels the 512-voxel grid fills
//     badly (48 x 32 x 32 x 512 couts: 384 blocks of 512 x 128 = 1.5 rounds of the 256 CUs, 512 of 384 x 128 = 2 rounds);
//   <4,4,32, 64,4> / <4,8,16, 64,4>: per wave 64 x 64 (16 MFMAs, 8 reads per unit), steps of 8 entries -- the same 16 KB of
//     weights and 64 MFMAs per wave and barrier -- for levels where 128-cout blocks leave CUs idle (48 x 32 x 32 x 512 couts:
//     96 tiles x 4 = 384 blocks = 1.5 rounds of the 256 CUs; x 8 = 768 = 3 whole rounds).  Parity-tested, then measured
//     1.5-3 % SLOWER there than conv3_halo32_kernel's 768 blocks of 256 x 128 (1126-1159 vs 1148-1176 TFLOP/s; 0.5 LDS reads per
//     MFMA instead of 0.375 and twice the halo DMA per FLOP eat the MFMA-shape gain): NOT instantiated or dispatched
//     (profiles/r02_notes.md).
// Epilogue form (round 4), template parameter DIRECT.  DIRECT: packed row 16 j + r of an n-tile holds cout NJ r + j, so that lane
// r16 ends up with the NJ = 8 CONSECUTIVE couts NJ r16 .. NJ r16 + 7 of each of its 16 voxel rows and stores them as 16-byte pieces
// straight from the accumulators (a store instruction of a wave = 4 voxel rows x 256 contiguous bytes): no 128 KB tile through
// LDS, no 2-byte LDS writes, no row re-reads.  Staged (round 2): the bf16 tile goes through LDS, packed row = cout.  The two forms
// use different packed weight images (ctsi_conv3_halo_k32_pack's `direct`).  Same-box alternation of whole bench runs
// (profiles/r04_epilogue_ab.log): 512-voxel tiles -1.8 % (plain), -2.1 % (ConvTranspose), -0.7 % (split-K), the 384-voxel split-K
// form -4.3 %; the 24- / 12-wide 384-voxel tiles -2 % (25 stitching windows: 46.7 -> 45.8 ms over their 20 launches); the PLAIN
// 3x4x32 / 3x8x16 tiles +3 % / +1.5-2 % (slower) and their Downsample forms +-0: ctsi_conv3_halo_k32_direct() picks per form.
// cout (within the block's n-tile) of accumulator column r16 of cout tile j
template <int NJ, bool DIRECT>
__device__ __forceinline__ int hk_col(int j, int r16) { return DIRECT ? r16 * NJ + j : j * 16 + r16; }

template <int TD_, int TH_, int TW_ = 32, int BN_ = 128, int UPS_ = 2, bool PL_ = false>
struct HkCfg {
    static constexpr int TD = TD_, TH = TH_, TW = TW_, UPS = UPS_;
    static constexpr int HD = PL_ ? TD : TD + 2, HH = TH + 2, HW = TW + 2;   // (planar form: no depth halo)
    static constexpr int HV = HD * HH * HW;                 // <4,4,32>: 1224 halo voxels
    static constexpr int HALO_INSTR = (HV + 31) / 32;       // wave-DMAs of 32 voxels x 32 B
    static constexpr int HALO_BYTES = HALO_INSTR * 1024;
    static constexpr int BM = TD * TH * TW;                 // 512
    static constexpr int BN = BN_;
    static constexpr int NJ = BN / 16;                      // 16-cout B tiles per wave
    static constexpr int TAP_BYTES = BN * 32;               // [BN couts][16 channels] bf16
    static constexpr int STEP_TAPS = 2 * UPS;
    static constexpr int WSLOT_BYTES = STEP_TAPS * TAP_BYTES;   // 16384
    static constexpr int NWS = 4;                           // three steps in flight + the one being read
    static constexpr int NWAVE = 8;
    static constexpr int MA = BM / 128;                     // 16-voxel A tiles per wave: 4 (512-voxel tile) or 3 (384)
    static constexpr int NTH = 64 * NWAVE;
    static constexpr int NPIECE = (HALO_INSTR + NWAVE - 1) / NWAVE;   // halo DMAs per wave and chunk
    static constexpr int OFF_W = 2 * HALO_BYTES;
    static constexpr int LOOP_END = OFF_W + NWS * WSLOT_BYTES;
    // output tile rows padded by 16 B: rows 4 apart (the k-groups of one ds_write_b16) fall 16 banks apart instead of on the
    // same banks (SQ_LDS_BANK_CONFLICT of the kernel 3.0 -> 0.8 %; the staging itself stayed at ~3.7 k cycles per tile: a
    // 2-way conflict fits under a 2-byte write's issue cost)
    static constexpr int BNP = BN + 8;
    static constexpr int OFF_ROW = LOOP_END > BM * BNP * 2 ? LOOP_END : BM * BNP * 2;
    static constexpr int OFF_CS = OFF_ROW + BM * 8;
    static constexpr int LDS_BYTES = OFF_CS + NWAVE * BN * 8;
    static constexpr int LPW = 64 / TW;                     // W-lines per wave
    // TW = 24 / 12 (round 4: the 24- and 12-wide planes of 192^2 patches, which 16- / 32-wide tiles cover at 75 %): a 16-row A tile
    // then STRADDLES W-lines, so every lane carries its own row offset per A tile instead of one wave-uniform offset (MA more
    // v_add per unit); nothing else in the kernel assumes that an A tile lies in one line
    static constexpr bool STRADDLE = TW % 16 != 0;
    static_assert(BM % 128 == 0 && (MA == 3 || (MA == 4 && TH % LPW == 0 && !STRADDLE)) && NPIECE <= 5 && LDS_BYTES <= 160 * 1024 &&
                      WSLOT_BYTES == 16384 && (UPS == 2 || UPS == 4), "unsupported tile");
    // A tile i (rows [16 i, 16 i + 16) of the wave's 64): halo-voxel offset from the wave's first voxel
    static constexpr int a_imm(int i) { return (((16 * i) / TW) * HW + (16 * i) % TW) * 32; }
};

__device__ __forceinline__ void hk_wait_vm(int allowed) {   // wave-uniform `allowed`
    switch (allowed) {
        case 0: asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)" ::: "memory"); break;
    }
}

// TR = true: ConvTranspose3d k = (3,4,4), s = (1,2,2), p = 1 (models/unet3d.py:218-221 Upsample, models/vae.py decoder): output
// voxel (d, 2 h + py, 2 w + px) of parity class (py, px) is a 3 x 2 x 2-tap convolution on the INPUT grid (k_h in {1, 3} at
// input rows {h, h - 1} for py = 0, {2, 0} at {h, h + 1} for py = 1; same along w; i_d = o_d + 1 - k_d), i.e. the same halo
// tile as the 3x3x3 conv with 12 entries per chunk instead of 27.  One block = one (input tile, class, n-tile); the four
// classes of a tile are neighbours in the grid (they share the halo in L2).
//
// SK = true: 2-way split-K.  Levels with few voxels and many channels (48 x 16 x 16 x 512 -> 512: 32 tiles of 384 voxels x 4
// n-tiles = 128 blocks for 256 CUs) run every (tile, n-tile) as TWO blocks that each walk half of the input-channel chunks.
// The block that finishes first parks its fp32 accumulators in a workspace ([tile][register][512 threads]: coalesced, the
// partner has the same register <-> output mapping) and leaves; the second adds them to its own and runs the epilogue.  a + b
// = b + a in fp32, so the result does not depend on which block comes first: bit-stable without a second pass.  Hand-off per
// MI355X_MICROARCH.md (per-XCD L2s are not coherent), in its form WITHOUT cache maintenance: every store and load of the parked
// bytes and of the flag is an agent-scope (sc1) access; the producer drains them (vmcnt(0), workgroup barrier) before one lane
// raises the flag, the consumer polls with one lane, then a workgroup barrier (see the epilogue).  The consumer waits only for
// a block that has already taken its ticket, i.e. one that is in its epilogue: no deadlock; the spin is bounded anyway.
// DS = true: strided Conv3d k = (3,4,4), s = (1,2,2), p = 1 (models/unet3d.py:204-207 Downsample, models/vae.py encoder) -- the
// mirror of the TR form.  Split the INPUT into its four (h, w) parity sub-grids in_c[d, m, n] = in[d, 2 m + py, 2 n + px]:
// out[d, y, x] = sum over the 4 classes of a 3 x 2 x 2-tap stride-1 convolution on that sub-grid (k_h = 1 - py + 2 b reads
// sub-grid row y + b - py, b in {0, 1}; same along w), i.e. 48 taps = 4 "virtual chunks" of 12 entries per 16 input
// channels, every one on the 3x3x3 conv's halo tile of the OUTPUT grid.  The sub-grid is only an address pattern: the halo DMA
// of virtual chunk vc = 4 * chunk + class fetches voxel (2 m + py, 2 n + px) -- a wave-uniform add to the class-(0, 0)
// offsets (H_in, W_in are even, so the validity of a halo voxel does not depend on the class).  All classes accumulate into
// the same output tile: one block = one (output tile, n-tile), K = 48 * Cin like the gather kernel, which re-staged the slab
// per tap (505-850 TFLOP/s on the three Downsample layers of the U-Net; 27-48 % LDS bank conflicts in its 48-tap form).
//
// Sticky device-side error word ([0] = count, [1] = last tile): set when a split-K consumer's bounded wait expires (see the
// hand-off below); read and cleared by ctsi_device_error_status().
__device__ unsigned int g_hk_device_error[2] = {0u, 0u};
// timing-only instrumentation (CTSI_DEBUG_FLAGS & 4096): per block, wave 0 records s_memtime at 7 points + its HW_ID
#define HK_NSTAMP 4096
__device__ unsigned long long g_hk_stamps[HK_NSTAMP][8];
#define HK_STAMP(K)                                                                                              \
    if ((CTSI_DBG(p.dbg, 4096)) && tid == 0 && blockIdx.x < HK_NSTAMP) g_hk_stamps[blockIdx.x][K] = __builtin_amdgcn_s_memtime();

// PL = true: the planar form, k = (1,3,3), s = 1, p = (0,1,1) -- a 3 x 3 convolution of every depth slice on its own (the VGG-19
// stack of the perceptual loss, whose depth axis counts IMAGES: vgg_loss_engine.py).  9 entries per 16-channel chunk in the same
// linear (chunk, tap) stream (9 is odd, as 27 is), a halo tile of TD x (TH + 2) x (TW + 2) voxels without depth halo, so a tile
// may span images and every step reads every halo slice.  A chunk lasts 2.25 steps: all its halo pieces go out in ONE issue
// group, the first in which its buffer is free (see issue_group).  RELU = true: max(., 0) on each value as the direct epilogue
// packs it (ctsi_conv_out.act = 2; planar instantiations only, which write no column sums).
template <int TD_, int TH_, int TW_ = 32, int BN_ = 128, int UPS_ = 2, bool TR = false, bool SK = false, bool DS = false, bool DIRECT = false>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, 512)))
conv3_halo_k32_kernel(const Conv3HaloParams p) {
    constexpr bool PL = false, RELU = false;
#include "conv3_halo_k32_body.inc"
}

// the planar (1,3,3) form: 128 couts, steps of 4 entries, the direct-store epilogue, optionally with ReLU
template <int TD_, int TH_, int TW_, bool RELU>
__global__ void __attribute__((amdgpu_flat_work_group_size(1, 512)))
conv3_planar_k32_kernel(const Conv3HaloParams p) {
    constexpr int BN_ = 128, UPS_ = 2;
    constexpr bool TR = false, SK = false, DS = false, DIRECT = true, PL = true;
#include "conv3_halo_k32_body.inc"
}

// ---- weight packing: fp32 (cout, cin, 3,3,3) -> bf16 [entry q = chunk16 * 27 + tap][cout_pad][16], zero entries up to whole steps;
//      ConvTranspose3d (cin, cout, 3,4,4) -> [class][entry q = chunk16 * 12 + t][cout_pad][16], t = (a * 2 + b) * 2 + c with
//      kernel taps k_d = 2 - a (halo slices ascending), k_h = (py ? {2, 0} : {1, 3})[b], k_w likewise (the tap order conv3_halo_k32_kernel<TR> walks)
__global__ void conv3_halo_k32_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int Cout, int CoutPad,
                                           int CinW, int nchunks, long long per_class, int form, int bn, int direct) {
    // form 0: 3x3x3; 1: ConvTranspose3d (3,4,4)/(1,2,2) (4 class images); 2: Conv3d (3,4,4)/(1,2,2) (nchunks = 4 virtual chunks
    // per 16 input channels: vc = 4 * chunk + class, entry t = (a * 2 + b) * 2 + c <-> k_d = a, k_h = 2 b + 1 - py, k_w = 2 c + 1 - px);
    // 3: planar Conv3d (1,3,3): entry q = chunk16 * 9 + tap
    const bool transposed = form == 1;
    const int taps = form == 3 ? 9 : form ? 12 : 27;
    const int Q = nchunks * taps;
    const long long total = per_class * (transposed ? 4 : 1);
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int cls = (int)(idx / per_class);
        const long long in_class = idx - cls * per_class;
        const int e = (int)(in_class & 15);
        const long long row = in_class >> 4;           // q * CoutPad + cout
        const int co_p = (int)(row % CoutPad);           // packed row
        // direct epilogue form: packed row 16 j + r of a bn-cout n-tile holds cout (bn / 16) r + j (see hk_col)
        const int co = direct ? (co_p / bn) * bn + (co_p % 16) * (bn / 16) + (co_p % bn) / 16 : co_p;
        const long long q = row / CoutPad;
        float v = 0.0f;
        if (q < Q) {
            const int t = (int)(q % taps), cc = (int)(q / taps);
            const int ci = (form == 2 ? (cc >> 2) : cc) * 16 + e;
            if (co < Cout && ci < CinW) {
                if (form == 2) {
                    const int py = (cc >> 1) & 1, px = cc & 1;
                    const int a = t >> 2, b = (t >> 1) & 1, c = t & 1;
                    v = w[((long long)co * CinW + ci) * 48 + (a * 4 + 2 * b + 1 - py) * 4 + 2 * c + 1 - px];
                } else if (transposed) {
                    const int py = cls >> 1, px = cls & 1;
                    const int a = 2 - (t >> 2), b = (t >> 1) & 1, c = t & 1;   // i_d = o_d + 1 - k_d: k_d descending = halo slices ascending
                    const int ky = py ? (b ? 0 : 2) : (b ? 3 : 1), kx = px ? (c ? 0 : 2) : (c ? 3 : 1);
                    v = w[((long long)ci * Cout + co) * 48 + (a * 4 + ky) * 4 + kx];
                } else {
                    v = w[((long long)co * CinW + ci) * taps + t];
                }
            }
        }
        out[idx] = f32_to_bf16(v);
    }
}

// form: 0 = 3x3x3, 1 = ConvTranspose3d (3,4,4)/(1,2,2), 2 = strided Conv3d (3,4,4)/(1,2,2), 3 = planar Conv3d (1,3,3)
extern "C" size_t ctsi_conv3_halo_k32_weight_bytes(int cin, int cout_pad, int bn, int form) {
    const long long q = (long long)(cin / 16) * (form == 3 ? 9 : form == 2 ? 48 : form == 1 ? 12 : 27), step = bn == 64 ? 8 : 4;   // entries per step: 2 x UPS
    return (size_t)(((q + step - 1) / step) * step * cout_pad * 32) * (form == 1 ? 4 : 1);
}

extern "C" int ctsi_conv3_halo_k32_pack(const float* w, void* packed, int cout, int cout_pad, int cin, int cin_w, int bn,
                                        int form, int direct, void* stream) {
    CTSI_CHECK_ARG(w && packed && cin % 16 == 0 && (bn == 64 || bn == 128) && cout_pad % bn == 0 && (form != 1 || cin_w == cin) &&
                       form >= 0 && form <= 3,
                   "ctsi_conv3_halo_k32_pack: bad arguments");
    const int nchunks = (cin / 16) * (form == 2 ? 4 : 1);
    const int transposed = form;
    const long long total = (long long)ctsi_conv3_halo_k32_weight_bytes(cin, cout_pad, bn, form) / 2;
    const long long per_class = form == 1 ? total / 4 : total;
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(conv3_halo_k32_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)packed,
                       cout, cout_pad, cin_w, nchunks, per_class, transposed, bn, direct);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// Which forms store straight from the accumulators (measured per form, see hk_col): the 512-voxel tiles and the 24- / 12-wide
// 384-voxel tiles in every form, and the 384-voxel split-K form of the plain conv; the other 384-voxel forms keep the staged epilogue.
// (-DHK_STAGED_EPILOGUE, `make staged`: the staged epilogue everywhere, for A/B timing through CTSI_LIB.)
extern "C" int ctsi_conv3_halo_k32_direct(int tile, int ksplit, int ds) {
#ifdef HK_STAGED_EPILOGUE
    return 0;
#else
    const bool t512 = tile == 0 || tile == 2, narrow = tile == 6 || tile == 7, planar = tile >= 16;
    return (t512 || narrow || planar || (tile == 5 && ksplit == 2 && !ds)) ? 1 : 0;
#endif
}

template <int TD, int TH, int TW, int BN, int UPS, bool TR, bool SK = false, bool DS = false>
static void hk_launch(const Conv3HaloParams* hp, hipStream_t stream) {
    using Cfg = HkCfg<TD, TH, TW, BN, UPS>;
#ifdef HK_STAGED_EPILOGUE
    constexpr bool DIRECT = false;
#else
    constexpr bool DIRECT = TD * TH * TW == 512 || TW == 24 || TW == 12 || (SK && !DS);
#endif
    auto k = conv3_halo_k32_kernel<TD, TH, TW, BN, UPS, TR, SK, DS, DIRECT>;
    static CtsiPerDeviceOnce attr_once;
    if (attr_once.first()) hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(k, dim3((TR ? 4 : 1) * (SK ? 2 : 1) * hp->mtiles * hp->ntiles_n), dim3(Cfg::NTH), Cfg::LDS_BYTES, stream,
                       *hp);
}

extern "C" size_t ctsi_conv3_halo_k32_splitk_bytes(int tiles) {   // [2 ints per tile: ticket, flag | pad to 256 B][partials]
    const size_t sync = ((size_t)tiles * 8 + 255) / 256 * 256;
    return sync + (size_t)tiles * (4 * 8 * 4) * 512 * sizeof(float);   // sized for the 512-voxel tile (128 accumulators per lane)
}

extern "C" int ctsi_conv3_halo_k32_launch(const Conv3HaloParams* hp, int tile /* 0: 4x4x32, 2: 4x8x16, 3: 3x4x32, 5: 3x8x16, 6: 4x4x24, 7: 8x4x12 */,
                                          int bn, void* stream) {
    CTSI_CHECK_ARG(bn == 128 && (tile == 0 || tile == 2 || tile == 3 || tile == 5 || tile == 6 || tile == 7),
                   "ctsi_conv3_halo_k32_launch: bad BN %d / tile %d", bn, tile);
    if (tile == 6 || tile == 7) {   // 384-voxel tiles for 24- / 12-wide planes (2-way split-K for the plain conv only)
        CTSI_CHECK_ARG(!(hp->ds && hp->tr) && !(hp->ksplit == 2 && (hp->ds || hp->tr)),
                       "ctsi_conv3_halo_k32_launch: tile %d has no split-K form for strided / transposed layers", tile);
        if (hp->ksplit == 2) {
            CTSI_CHECK_ARG(hp->sk_ws && hp->sk_sync && hp->nchunks % 8 == 0, "ctsi_conv3_halo_k32_launch: split-K needs its workspace");
            if (tile == 6)
                hk_launch<4, 4, 24, 128, 2, false, true>(hp, (hipStream_t)stream);
            else
                hk_launch<8, 4, 12, 128, 2, false, true>(hp, (hipStream_t)stream);
        } else if (hp->ds) {
            CTSI_CHECK_ARG(hp->Hi == 2 * hp->Ho && hp->Wi == 2 * hp->Wo && hp->C2 == 0 && hp->nchunks % 4 == 0,
                           "ctsi_conv3_halo_k32_launch: the Downsample form needs even input planes and one source");
            if (tile == 6)
                hk_launch<4, 4, 24, 128, 2, false, false, true>(hp, (hipStream_t)stream);
            else
                hk_launch<8, 4, 12, 128, 2, false, false, true>(hp, (hipStream_t)stream);
        } else if (hp->tr) {
            if (tile == 6)
                hk_launch<4, 4, 24, 128, 2, true>(hp, (hipStream_t)stream);
            else
                hk_launch<8, 4, 12, 128, 2, true>(hp, (hipStream_t)stream);
        } else if (tile == 6) {
            hk_launch<4, 4, 24, 128, 2, false>(hp, (hipStream_t)stream);
        } else {
            hk_launch<8, 4, 12, 128, 2, false>(hp, (hipStream_t)stream);
        }
        CTSI_LAUNCH_CHECK();
        return CTSI_OK;
    }
    if (hp->ds) {   // strided Conv3d (3,4,4)/(1,2,2): nchunks counts virtual chunks (4 per 16 input channels)
        CTSI_CHECK_ARG(!hp->tr && hp->Hi == 2 * hp->Ho && hp->Wi == 2 * hp->Wo && hp->C2 == 0 && hp->nchunks % 4 == 0,
                       "ctsi_conv3_halo_k32_launch: the Downsample form needs even input planes and one source");
        if (hp->ksplit == 2) {
            CTSI_CHECK_ARG(tile == 5 && hp->sk_ws && hp->sk_sync && hp->nchunks % 8 == 0, "ctsi_conv3_halo_k32_launch: split-K needs its workspace");
            hk_launch<3, 8, 16, 128, 2, false, true, true>(hp, (hipStream_t)stream);
        } else if (tile == 5) {
            hk_launch<3, 8, 16, 128, 2, false, false, true>(hp, (hipStream_t)stream);
        } else if (tile == 3) {
            hk_launch<3, 4, 32, 128, 2, false, false, true>(hp, (hipStream_t)stream);
        } else if (tile == 2) {
            hk_launch<4, 8, 16, 128, 2, false, false, true>(hp, (hipStream_t)stream);
        } else {
            hk_launch<4, 4, 32, 128, 2, false, false, true>(hp, (hipStream_t)stream);
        }
    } else if (hp->tr && tile == 5) {
        hk_launch<3, 8, 16, 128, 2, true>(hp, (hipStream_t)stream);
    } else if (hp->tr && tile == 3) {
        hk_launch<3, 4, 32, 128, 2, true>(hp, (hipStream_t)stream);
    } else if (tile == 5) {          // 3x8x16 = 384 voxels for 16-wide levels, plain or 2-way split-K
        if (hp->ksplit == 2) {
            CTSI_CHECK_ARG(hp->sk_ws && hp->sk_sync && hp->nchunks % 8 == 0, "ctsi_conv3_halo_k32_launch: split-K needs its workspace");
            hk_launch<3, 8, 16, 128, 2, false, true>(hp, (hipStream_t)stream);
        } else {
            hk_launch<3, 8, 16, 128, 2, false, false>(hp, (hipStream_t)stream);
        }
    } else if (tile == 3) {
        hk_launch<3, 4, 32, 128, 2, false>(hp, (hipStream_t)stream);
    } else if (tile == 0 && hp->ksplit == 2) {   // 4x4x32 with 2-way split-K
        CTSI_CHECK_ARG(hp->sk_ws && hp->sk_sync && hp->nchunks % 8 == 0, "ctsi_conv3_halo_k32_launch: split-K needs its workspace");
        hk_launch<4, 4, 32, 128, 2, false, true>(hp, (hipStream_t)stream);
    } else if (hp->tr) {
        if (tile == 2)
            hk_launch<4, 8, 16, 128, 2, true>(hp, (hipStream_t)stream);
        else
            hk_launch<4, 4, 32, 128, 2, true>(hp, (hipStream_t)stream);
    } else if (tile == 2) {
        hk_launch<4, 8, 16, 128, 2, false>(hp, (hipStream_t)stream);
    } else {
        hk_launch<4, 4, 32, 128, 2, false>(hp, (hipStream_t)stream);
    }
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// The planar (1,3,3) form.  tile: 16 = 1x16x32, 17 = 2x16x16, 18 = 4x8x16 (512 voxels, A tiles inside one W-line), 19 = 4x4x24,
// 20 = 8x4x12 (384 voxels, A tiles that straddle W-lines, for 24- / 12-wide planes); TD counts depth slices (images).  One
// source or two, whole 16-channel chunks each; no split-K, no column sums.  relu != 0: the ReLU epilogue.
template <int TD, int TH, int TW>
static void hk_launch_planar(const Conv3HaloParams* hp, int relu, hipStream_t stream) {
    using Cfg = HkCfg<TD, TH, TW, 128, 2, true>;
    static CtsiPerDeviceOnce attr_once;
    if (attr_once.first()) {
        hipFuncSetAttribute((const void*)conv3_planar_k32_kernel<TD, TH, TW, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipFuncSetAttribute((const void*)conv3_planar_k32_kernel<TD, TH, TW, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    const dim3 grid(hp->mtiles * hp->ntiles_n), block(Cfg::NTH);
    if (relu)
        hipLaunchKernelGGL((conv3_planar_k32_kernel<TD, TH, TW, true>), grid, block, Cfg::LDS_BYTES, stream, *hp);
    else
        hipLaunchKernelGGL((conv3_planar_k32_kernel<TD, TH, TW, false>), grid, block, Cfg::LDS_BYTES, stream, *hp);
}

extern "C" int ctsi_conv3_planar_k32_launch(const Conv3HaloParams* hp, int tile, int relu, void* stream) {
    CTSI_CHECK_ARG(tile >= 16 && tile <= 20, "ctsi_conv3_planar_k32_launch: bad tile %d", tile);
    CTSI_CHECK_ARG(!hp->tr && !hp->ds && hp->ksplit != 2 && hp->dshift == 0 && hp->colsum == nullptr && hp->Di == hp->Do &&
                       hp->Hi == hp->Ho && hp->Wi == hp->Wo && hp->C1 % 16 == 0 && hp->C2 % 16 == 0,
                   "ctsi_conv3_planar_k32_launch: the planar form is a plain stride-1 (1,3,3) conv without column sums");
    hipStream_t st = (hipStream_t)stream;
    switch (tile) {
    case 16: hk_launch_planar<1, 16, 32>(hp, relu, st); break;
    case 17: hk_launch_planar<2, 16, 16>(hp, relu, st); break;
    case 18: hk_launch_planar<4, 8, 16>(hp, relu, st); break;
    case 19: hk_launch_planar<4, 4, 24>(hp, relu, st); break;
    default: hk_launch_planar<8, 4, 12>(hp, relu, st); break;
    }
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// Number of device-side errors recorded since the last call with reset != 0 (0 on a healthy run), and the split-K tile of the
// last one.  SYNCHRONOUS (a 8-byte device-to-host copy): call it where the host reads results anyway.
extern "C" int ctsi_debug_k32_stamps(unsigned long long* out, int nblocks) {   // timing-only (CTSI_DEBUG_FLAGS & 4096)
    if (nblocks > HK_NSTAMP) nblocks = HK_NSTAMP;
    CTSI_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hk_stamps), (size_t)nblocks * 8 * sizeof(unsigned long long)));
    return CTSI_OK;
}

extern "C" int ctsi_device_error_status(unsigned int* count, unsigned int* detail, int reset) {
    CTSI_CHECK_ARG(count, "ctsi_device_error_status: null argument");
    unsigned int h[2] = {0u, 0u};
    CTSI_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_hk_device_error), sizeof(h)));
    *count = h[0];
    if (detail) *detail = h[1];
    if (reset && h[0]) {
        const unsigned int z[2] = {0u, 0u};
        CTSI_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_hk_device_error), z, sizeof(z)));
    }
    return CTSI_OK;
}
