// The conv plan: what conv_plan.hip (host-only: which kernel and which tile a layer runs on) decides and conv_mfma.hip
// (weight packing, launches) consumes.
#pragma once
#include "ctsi_internal.h"

#define CTSI_MAX_TAPS 48
#define CTSI_BK 64

// Kernel families.  CONV_GATHER (conv_gather_mfma_kernel, conv_mfma.hip) has no tile table: its tiles are power-of-two boxes or
// linear runs of BM rows.  The 16x16x32 form of the 4x4x16 tile, persistent and half-size blocks and the 32x32x16 form of the
// 512-voxel tile were measured slower and live under csrc/experiments/, outside libctsi.so.
enum ConvFamily {
    CONV_GATHER,
    CONV_HALO32,   // conv3_halo32_kernel (conv3_halo.hip): 3x3x3 LDS halo tiles on 32x32x16 MFMAs
    CONV_K32,      // conv3_halo_k32_kernel (conv3_halo_k32.hip): 512- / 384-voxel tiles on 16x16x32 MFMAs; ConvTranspose, Downsample
    CONV_HEAD,     // few-cout heads (conv3_head.hip, conv3_head2.hip)
};

// One row per tile form of the halo-tile kernels: THE place a new form is added (conv_plan.hip holds the table).
struct ConvForm {
    ConvFamily family;
    int mode;          // what ctsi_conv_plan_config reports (engine.py derives its kernel labels from it)
    int td, th, tw;    // output tile; BM = td * th * tw voxels
    int bn;            // couts per block
    int code;          // what the launcher takes: `wide` of ctsi_conv3_halo_launch, `tile` of ctsi_conv3_halo_k32_launch
    double eff;        // relative efficiency on full grids as a 3x3x3 conv, with which a chosen form defends its place
    const char* name;
};

struct ctsi_conv_plan {
    ctsi_conv_desc d;
    int Cin, CinW;
    int Do, Ho, Wo;
    int Dr, Hr, Wr, sH, sW, uH, uW;
    int nclass, T;
    int small, lcpt, kc_per_tap, ksteps, Ktot;
    int BM, BN, CoutPad, ntiles_n;
    int lTH, lTW, TD, TH, TW, tilesD, tilesH, tilesW, tps, mtiles;
    int linear;   // gather kernel: tiles are runs of BM consecutive row-grid voxels
    int tapk[CTSI_MAX_TAPS];
    int tapdelta[CTSI_MAX_TAPS];
    int8_t od[CTSI_MAX_TAPS], oh[CTSI_MAX_TAPS], ow[CTSI_MAX_TAPS];
    int NA, NB, NC;
    int ad[4][4], bh[4][4], cw[4][4];
    int8_t pH[4], pW[4];
    int tap_margin[4], ad_min[4];
    int fast, dshift;
    const ConvForm* form;   // the row of the tile table this plan runs on; NULL: gather kernel (or stem / stream1 below)
    int gsplit;     // gather kernel: S-way split-K for launches of a few dozen blocks with a deep K loop (needs a workspace)
    int ds;         // k32 kernel: the strided (3,4,4)/(1,2,2) Downsample form (conv3_halo_k32.hip, DS)
    int head2;      // head: conv3_head2_kernel (taps as the GEMM's N dimension) serves the launches that ask for no column sums
    int planar;     // k32 kernel: the planar (1,3,3) form (conv3_halo_k32.hip, PL): depth slices are independent images
    int ksplit;     // k32 kernel: 2 = two blocks per (tile, n-tile), each half of the input-channel chunks (needs a workspace)
    int stem;       // 1: conv3_stem_kernel (conv3_stem.hip: 3x3x3 conv of a one-channel volume stored with 8 channels); chosen by
                    // ctsi_conv_plan_set_weight_cin(plan, 1)
    int stream1;    // > 0: conv1_stream_kernel (conv1_stream.hip: 1x1x1 conv + fused GroupNorm tail as a streaming pass), value = 16-cout
                    // tiles per n-tile; chosen by ctsi_conv_plan_set_stream_tail, never by ctsi_conv_plan_create
    double flops;
};

static inline ConvFamily conv_family(const ctsi_conv_plan* p) { return p->form ? p->form->family : CONV_GATHER; }
// k32 plans: the packed image's form (0 Conv3d 3x3x3, 1 ConvTranspose3d, 2 strided Conv3d, 3 planar Conv3d (1,3,3)) and whether
// it is cout-permuted
static inline int conv_k32_image(const ctsi_conv_plan* p) { return p->planar ? 3 : p->ds ? 2 : p->d.transposed; }
static inline int conv_k32_direct(const ctsi_conv_plan* p) { return ctsi_conv3_halo_k32_direct(p->form->code, p->ksplit, p->ds); }
// few-cout heads: the packed buffer holds conv3_head_kernel's image, padded to 256 B, then conv3_head2_kernel's
static inline size_t head1_bytes(const ctsi_conv_plan* p) {
    return ((size_t)p->Cin * 27 * (p->d.cout <= 8 ? 8 : 16) * 2 + 1024 + 255) / 256 * 256;
}
