// Conv plans (host-only): which kernel and which tile a convolution runs on -- inference, training data-gradient, VAE and
// the sharded views.  The kernels, weight packing and launches are in conv_mfma.hip and the files it drives.
//
// A new tile form is one row of FORMS below plus the launcher code it mirrors; the choosers compare candidates through score().
#include "conv_plan.h"
#include <string.h>
#include <stdlib.h>

// ---- the tile table -----------------------------------------------------------------------------------------------------
// Relative efficiencies on full grids, measured (profiles/r01_notes.md, r02_notes.md): 4x2x32 / 32x32x16 MFMAs 1.0, the 3x4x16
// tile's 3x1 MFMA tiles per wave 0.95 of the 2x2 form, k32 512-voxel 1.15, k32 384-voxel 1.1, the straddling narrow tiles 1.07.
static const double EFF_HALO32 = 1.0, EFF_HALO32_192 = 0.95, EFF_K32_512 = 1.15, EFF_K32_384 = 1.1, EFF_K32_NARROW = 1.07;
// ... and as first picked, before a form defends its place: 16-wide 0.85, 512 voxels 1.1, its 4x8x16 form 1.0
static const double EFF_PICK_W16 = 0.85, EFF_PICK_512 = 1.1, EFF_PICK_512_W16 = 1.0;
// strided / transposed forms of the k32 kernel: 512-voxel tiles 1.0, 384-voxel tiles 0.96
static const double EFF_ST_512 = 1.0, EFF_ST_384 = 0.96;
// the gather kernel where halo tiles wasted > 30 % of their rows
static const double EFF_GATHER_STANDIN = 0.6;

enum FormId { H32_4x2x32, H32_4x4x16, H32_3x4x16, K32_4x4x32, K32_4x8x16, K32_3x4x32, K32_3x8x16, K32_4x4x24, K32_8x4x12, HEAD_4x2x16,
              PL_1x16x32, PL_2x16x16, PL_4x8x16, PL_4x4x24, PL_8x4x12, N_FORMS };
// codes: `wide` 1 / 3 / 4 of ctsi_conv3_halo_launch (conv3_halo.hip), `tile` 0 / 2 / 3 / 5 / 6 / 7 of ctsi_conv3_halo_k32_launch
// (conv3_halo_k32.hip); the 4x4x24 / 8x4x12 tiles are A tiles that straddle W-lines, for 24- / 12-wide planes
static const ConvForm FORMS[N_FORMS] = {
    {CONV_HALO32, 4, 4, 2, 32, 128, 1, EFF_HALO32, "halo32 4x2x32"},
    {CONV_HALO32, 4, 4, 4, 16, 128, 3, EFF_HALO32, "halo32 4x4x16"},        // an A tile of 32 rows = two W-lines of 16
    {CONV_HALO32, 4, 3, 4, 16, 128, 4, EFF_HALO32_192, "halo32 3x4x16"},
    {CONV_K32, 9, 4, 4, 32, 128, 0, EFF_K32_512, "k32 4x4x32"},
    {CONV_K32, 9, 4, 8, 16, 128, 2, EFF_K32_512, "k32 4x8x16"},
    {CONV_K32, 9, 3, 4, 32, 128, 3, EFF_K32_384, "k32 3x4x32"},
    {CONV_K32, 9, 3, 8, 16, 128, 5, EFF_K32_384, "k32 3x8x16"},
    {CONV_K32, 9, 4, 4, 24, 128, 6, EFF_K32_NARROW, "k32 4x4x24"},
    {CONV_K32, 9, 8, 4, 12, 128, 7, EFF_K32_NARROW, "k32 8x4x12"},
    {CONV_HEAD, 8, 4, 2, 16, 16, 0, 1.0, "head 4x2x16"},                    // x 16 couts, see conv3_head.hip
    // the planar (1,3,3) form of the k32 kernel (codes 16-20 of ctsi_conv3_planar_k32_launch): td counts depth slices, which
    // are independent images; no depth halo, so the flat tiles stage the fewest halo voxels per output voxel
    {CONV_K32, 9, 1, 16, 32, 128, 16, EFF_K32_512, "planar 1x16x32"},
    {CONV_K32, 9, 2, 16, 16, 128, 17, EFF_K32_512, "planar 2x16x16"},
    {CONV_K32, 9, 4, 8, 16, 128, 18, EFF_K32_512, "planar 4x8x16"},
    {CONV_K32, 9, 4, 4, 24, 128, 19, EFF_K32_NARROW, "planar 4x4x24"},
    {CONV_K32, 9, 8, 4, 12, 128, 20, EFF_K32_NARROW, "planar 8x4x12"},
};
static int form_voxels(const ConvForm& f) { return f.td * f.th * f.tw; }
// the 384-voxel / 512-voxel k32 tile of the same width
static const ConvForm* k32_sized(const ConvForm* f, bool v384) {
    return &FORMS[f->tw == 16 ? (v384 ? K32_3x8x16 : K32_4x8x16) : (v384 ? K32_3x4x32 : K32_4x4x32)];
}

// ---- overrides: tuning / test aids, read once per ctsi_conv_plan_create ------------------------------------
enum Tri { UNSET = -1, OFF = 0, ON = 1 };
enum SplitK { SK_UNSET, SK_OFF, SK_ON, SK_PLAIN, SK_512 };
struct PlanEnv {
    bool no_halo3, force_halo3, no_c16, no_head3, no_head2, no_fast;
    Tri m512, m512w16, k32_384, k32t, k32d, narrow, narrow_sk, linear;
    int planar;               // -1: unset, 0: the gather kernel, 1: the planar form wherever it applies, 16-20: that tile where it applies
    int halo_tile;            // 16 | 32, 0: unset
    int h32w16;               // 1 | 2, 0: unset
    SplitK splitk;
    int sk384_min, sk512_min; // least input channels of the 384-voxel split-K forms / of the 4x4x32 split-K form (A/B timing)
    bool has_gsplit; int gsplit;
    int tile_bm, tile_bn;     // gather tile, 0: unset
};
static Tri env_tri(const char* name) {
    const char* e = getenv(name);
    return e && !strcmp(e, "0") ? OFF : e && !strcmp(e, "1") ? ON : UNSET;
}
static int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}
static PlanEnv read_plan_env() {
    PlanEnv e;
    e.no_halo3 = getenv("CTSI_CONV_NO_HALO3") != nullptr;
    e.force_halo3 = getenv("CTSI_CONV_FORCE_HALO3") != nullptr;
    e.no_c16 = getenv("CTSI_CONV_NO_C16") != nullptr;
    e.no_head3 = getenv("CTSI_CONV_NO_HEAD3") != nullptr;
    e.no_head2 = getenv("CTSI_CONV_NO_HEAD2") != nullptr;
    e.no_fast = getenv("CTSI_CONV_NO_FAST") != nullptr;
    e.m512 = env_tri("CTSI_CONV_M512");
    e.m512w16 = env_tri("CTSI_CONV_M512W16");          // the 4x8x16 form of the 512-voxel kernel
    e.k32_384 = env_tri("CTSI_CONV_K32_384");
    e.k32t = env_tri("CTSI_CONV_K32T");                // 0: ConvTranspose3d stays on the gather kernel
    e.k32d = env_tri("CTSI_CONV_K32D");                // 0: the strided Conv3d stays on the gather kernel
    {   // CTSI_CONV_PLANAR: "0" the (1,3,3) convs stay on the gather kernel | "1" the planar form wherever it applies | a tile
        // ("1x16x32", "2x16x16", "4x8x16", "4x4x24", "8x4x12"): that tile wherever it applies (A/B timing, parity tests)
        const char* pl = getenv("CTSI_CONV_PLANAR");
        e.planar = -1;
        if (pl && (!strcmp(pl, "0") || !strcmp(pl, "1"))) e.planar = pl[0] - '0';
        for (int f = PL_1x16x32; pl && f <= PL_8x4x12; ++f)
            if (!strcmp(pl, FORMS[f].name + 7)) e.planar = FORMS[f].code;   // (the name behind "planar ")
    }
    e.narrow = env_tri("CTSI_CONV_K32_NARROW");        // 0 / 1: never / wherever the plane divides
    e.narrow_sk = env_tri("CTSI_CONV_K32_NARROW_SK");  // 0 / 1: never / wherever K allows
    e.linear = env_tri("CTSI_CONV_LINEAR");
    const char* hv = getenv("CTSI_CONV_HALO_TILE");    // "16" | "32"
    e.halo_tile = hv && !strcmp(hv, "16") ? 16 : hv && !strcmp(hv, "32") ? 32 : 0;
    const char* hw = getenv("CTSI_CONV_H32W16");       // "1" | "2": 4x4x16 / 3x4x16
    e.h32w16 = hw && !strcmp(hw, "1") ? 1 : hw && !strcmp(hw, "2") ? 2 : 0;
    const char* sk = getenv("CTSI_CONV_K32_SPLITK");   // "0" | "1" | "plain" | "512"
    e.splitk = !sk ? SK_UNSET : !strcmp(sk, "0") ? SK_OFF : !strcmp(sk, "1") ? SK_ON : !strcmp(sk, "plain") ? SK_PLAIN
               : !strcmp(sk, "512") ? SK_512 : SK_UNSET;
    e.sk384_min = env_int("CTSI_CONV_K32_SK384_MIN", 256);
    e.sk512_min = env_int("CTSI_CONV_K32_SK512_MIN", 512);
    const char* gs = getenv("CTSI_CONV_GSPLIT");       // 0 | 2..8
    e.has_gsplit = gs != nullptr;
    e.gsplit = gs ? atoi(gs) : 0;
    const char* tile = getenv("CTSI_CONV_TILE");       // "128x128" | "256x128" | "256x256" (tuning aid)
    e.tile_bm = tile && !strcmp(tile, "128x128") ? 128 : tile && (!strcmp(tile, "256x128") || !strcmp(tile, "256x256")) ? 256 : 0;
    e.tile_bn = tile && !strcmp(tile, "256x256") ? 256 : 128;
    return e;
}

// ---- the score ---------------------------------------------------------------------------------------------------------
// blocks rounded up to whole rounds of the 256 CUs
static double cu_rounds(long long b) { return (double)(((b + 255) / 256) * 256); }
static double cu_fill(long long b) { return (double)b / cu_rounds(b); }
static long long plan_rows(const ctsi_conv_plan* p) { return (long long)p->Dr * p->Hr * p->Wr; }
// rows of one sample when the row grid is covered with f's tiles
static long long padded_rows(const ctsi_conv_plan* p, const ConvForm& f) {
    return (long long)ceil_div(p->Dr, f.td) * ceil_div(p->Hr, f.th) * ceil_div(p->Wr, f.tw) * form_voxels(f);
}
// score = useful fraction of the tile rows x fill of the 256 CUs (blocks / whole rounds) x the kernel's relative efficiency.
// kmul: blocks per (tile, n-tile) (2-way split-K); classes: parity classes per input tile (ConvTranspose: 4)
struct TileFit { long long blocks; double useful, score; };
static TileFit fit(const ctsi_conv_plan* p, const ConvForm& f, int kmul, int classes, double eff) {
    const long long t = (long long)p->d.n * ceil_div(p->Dr, f.td) * ceil_div(p->Hr, f.th) * ceil_div(p->Wr, f.tw);
    TileFit r;
    r.blocks = t * classes * ceil_div(p->d.cout, 128) * kmul;
    r.useful = (double)plan_rows(p) * p->d.n / ((double)t * f.td * f.th * f.tw);
    r.score = r.useful * (double)r.blocks / cu_rounds(r.blocks) * eff;
    return r;
}
static double score(const ctsi_conv_plan* p, FormId f, int kmul, double eff) { return fit(p, FORMS[f], kmul, 1, eff).score; }
// the score with which the plan's current form defends its place
static double defended(const ctsi_conv_plan* p) { return fit(p, *p->form, p->ksplit == 2 ? 2 : 1, 1, p->form->eff).score; }

static int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// gather kernel: the power-of-two (TD,TH,TW) with TD*TH*TW == BM that covers the row grid with the fewest
// padded rows; ties go to the most cube-like tile (smallest halo for the L2).
static void choose_box_tile(ctsi_conv_plan* p) {
    long long best = -1;
    int bsurf = 0;
    const int lb = ilog2(p->BM);
    for (int lw = 0; lw <= lb; ++lw)
        for (int lh = 0; lh + lw <= lb; ++lh) {
            const int tw = 1 << lw, th = 1 << lh, td = p->BM >> (lw + lh);
            const long long tiles = (long long)ceil_div(p->Dr, td) * ceil_div(p->Hr, th) * ceil_div(p->Wr, tw);
            const int surf = (td + 2) * (th + 2) * (tw + 2);
            if (best < 0 || tiles < best || (tiles == best && surf < bsurf)) {
                best = tiles;
                bsurf = surf;
                p->TD = td; p->TH = th; p->TW = tw;
            }
        }
}

// ---- geometry and taps ---------------------------------------------------------------------------------------------------
static int plan_geometry(ctsi_conv_plan* p) {
    const ctsi_conv_desc& d = p->d;
    auto unsupported = [](auto... msg) {   // (ctsi_conv_plan_create frees the plan)
        ctsi_set_error(msg...);
        return (int)CTSI_ERR_UNSUPPORTED;
    };
    p->dshift = d.halo_d ? 1 : 0;
    const int di_own = d.di - 2 * p->dshift;   // depth of the slab the rows cover
    if (d.halo_d && (d.kd != 3 || d.pd != 1 || di_own < 1))
        return unsupported("ctsi_conv_plan_create: halo_d needs kd=3, pd=1 and di >= 3");
    p->Cin = d.c1 + d.c2;
    p->CinW = p->Cin;
    const int KK = d.kd * d.kh * d.kw;
    if (!d.transposed) {
        p->Do = di_own + 2 * d.pd - d.kd + 1;
        p->Ho = (d.hi + 2 * d.ph - d.kh) / d.sh + 1;
        p->Wo = (d.wi + 2 * d.pw - d.kw) / d.sw + 1;
        if (KK > CTSI_MAX_TAPS || p->Do <= 0 || p->Ho <= 0 || p->Wo <= 0 || d.kd > 3 || d.kh > 4 || d.kw > 4)
            return unsupported("ctsi_conv_plan_create: unsupported Conv3d geometry k=(%d,%d,%d)", d.kd, d.kh, d.kw);
        p->nclass = 1; p->T = KK;
        p->Dr = p->Do; p->Hr = p->Ho; p->Wr = p->Wo;
        p->sH = d.sh; p->sW = d.sw; p->uH = 1; p->uW = 1;
        p->pH[0] = 0; p->pW[0] = 0;
        p->NA = d.kd; p->NB = d.kh; p->NC = d.kw;
        for (int a = 0; a < d.kd; ++a) p->ad[0][a] = a - d.pd;
        for (int b = 0; b < d.kh; ++b) p->bh[0][b] = b - d.ph;
        for (int c = 0; c < d.kw; ++c) p->cw[0][c] = c - d.pw;
        int t = 0;
        for (int a = 0; a < d.kd; ++a)
            for (int b = 0; b < d.kh; ++b)
                for (int c = 0; c < d.kw; ++c, ++t) {
                    p->od[t] = (int8_t)(a - d.pd);
                    p->oh[t] = (int8_t)(b - d.ph);
                    p->ow[t] = (int8_t)(c - d.pw);
                    p->tapk[t] = (a * d.kh + b) * d.kw + c;
                }
        p->flops = 2.0 * d.n * (double)p->Do * p->Ho * p->Wo * p->Cin * d.cout * KK;
    } else {
        // ConvTranspose3d, depth stride 1: o_d = i_d - pd + k_d; o_h = i_h*sh - ph + k_h.
        // One parity class per (o_h % sh, o_w % sw); each class is a stride-1 gather conv on the
        // input grid with kd * (kh/sh) * (kw/sw) taps.
        if (!(d.sh == 2 && d.sw == 2 && d.kh == 4 && d.kw == 4 && d.ph == 1 && d.pw == 1 && d.kd == 3 && d.pd == 1))
            return unsupported("ctsi_conv_plan_create: ConvTranspose3d supports k=(3,4,4) s=(1,2,2) p=1 only");
        p->Do = di_own; p->Ho = d.hi * 2; p->Wo = d.wi * 2;
        p->nclass = 4; p->T = 12;
        p->Dr = di_own; p->Hr = d.hi; p->Wr = d.wi;
        p->sH = 1; p->sW = 1; p->uH = 2; p->uW = 2;
        for (int cls = 0; cls < 4; ++cls) {
            const int py = cls >> 1, px = cls & 1;
            p->pH[cls] = (int8_t)py; p->pW[cls] = (int8_t)px;
            // output o = 2m+py receives (k, i): py=0 -> (1,m),(3,m-1); py=1 -> (2,m),(0,m+1)
            const int ky[2] = {py == 0 ? 1 : 2, py == 0 ? 3 : 0};
            const int oy[2] = {0, py == 0 ? -1 : 1};
            const int kx[2] = {px == 0 ? 1 : 2, px == 0 ? 3 : 0};
            const int ox[2] = {0, px == 0 ? -1 : 1};
            p->NA = 3; p->NB = 2; p->NC = 2;
            for (int a = 0; a < 3; ++a) p->ad[cls][a] = 1 - a;
            for (int b = 0; b < 2; ++b) { p->bh[cls][b] = oy[b]; p->cw[cls][b] = ox[b]; }
            int t = cls * 12;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 2; ++b)
                    for (int c = 0; c < 2; ++c, ++t) {
                        p->od[t] = (int8_t)(1 - a);  // i_d = o_d + pd - k_d
                        p->oh[t] = (int8_t)oy[b];
                        p->ow[t] = (int8_t)ox[c];
                        p->tapk[t] = (a * 4 + ky[b]) * 4 + kx[c];
                    }
        }
        p->flops = 2.0 * d.n * (double)di_own * d.hi * d.wi * p->Cin * d.cout * KK;
    }
    for (int t = 0; t < p->nclass * p->T; ++t)
        p->tapdelta[t] = (p->od[t] * d.hi + p->oh[t]) * d.wi + p->ow[t];
    for (int c = 0; c < p->nclass; ++c) {
        int mn = 0, dmin = 0;
        for (int t = 0; t < p->T; ++t) {
            if (p->tapdelta[c * p->T + t] < mn) mn = p->tapdelta[c * p->T + t];
            if (p->od[c * p->T + t] < dmin) dmin = p->od[c * p->T + t];
        }
        p->tap_margin[c] = -mn;
        p->ad_min[c] = dmin;
    }
    return CTSI_OK;
}

static void plan_k_walk(ctsi_conv_plan* p) {
    if (p->Cin <= 32 && (p->Cin & (p->Cin - 1)) == 0) {
        p->small = 1;
        p->lcpt = ilog2(p->Cin / 8);
        p->ksteps = ceil_div(p->T << p->lcpt, 8);   // chunks of 8 channels, 8 per K-step
    } else {
        p->kc_per_tap = ceil_div(p->Cin, 64);
        p->ksteps = p->T * p->kc_per_tap;
    }
    p->Ktot = p->ksteps * CTSI_BK;
}

// gather tile: the bigger the tile the fewer L2->LDS bytes per flop (128x128: 64 flop/B, 256x128: 85, 256x256: 128), but the
// grid must still fill 256 CUs about twice over.
static void choose_gather_tile(ctsi_conv_plan* p, const PlanEnv& e) {
    const ctsi_conv_desc& d = p->d;
    const long long rows = d.n * plan_rows(p) * p->nclass;
    p->BM = 128; p->BN = d.cout <= 32 ? 32 : 128;
    if (d.cout <= 32) return;
    const long long wg_256x256 = (rows / 256) * ceil_div(d.cout, 256);
    const long long wg_256x128 = (rows / 256) * ceil_div(d.cout, 128);
    if (d.cout >= 256 && d.cout % 256 == 0 && wg_256x256 >= 640) {
        p->BM = 256; p->BN = 256;
    } else if (wg_256x128 >= 640) {
        p->BM = 256; p->BN = 128;
    }
    if (e.tile_bm && (e.tile_bn != 256 || d.cout % 256 == 0)) { p->BM = e.tile_bm; p->BN = e.tile_bn; }
}

// the tile halo (8 depth slices of the larger source) must fit 2^31 bytes
static bool halo_fits(const ctsi_conv_plan* p) {
    return 8.0 * p->d.hi * p->d.wi * (p->d.c1 > p->d.c2 ? p->d.c1 : p->d.c2) * 2.0 < 2.0e9;
}
static bool is_k3(const ctsi_conv_desc& d) {
    return !d.transposed && d.kd == 3 && d.kh == 3 && d.kw == 3 && d.sh == 1 && d.sw == 1 && d.pd == 1 && d.ph == 1 && d.pw == 1;
}
// whether the useful rows are at least 70 % of the rows f's tiles cover
static bool covers_70(const ctsi_conv_plan* p, FormId f) { return plan_rows(p) * 10 >= padded_rows(p, FORMS[f]) * 7; }
// the straddling tiles apply where the plane divides into them and not into 16-wide ones
static bool narrow_fits(const ctsi_conv_plan* p, const ConvForm& f) { return p->Wr % f.tw == 0 && p->Wr % 16 != 0; }
static bool splitk_channels(const ctsi_conv_plan* p) { return p->Cin % 128 == 0 && p->d.c1 % 16 == 0 && p->d.c2 % 16 == 0; }

// 3x3x3 / stride 1 / pad 1 with whole 32-channel chunks per source: LDS halo-tile kernels, provided the 4x4x16 tile does not
// waste more than ~30 % of the rows and the per-tile halo fits 2^31 bytes
static void choose_k3_form(ctsi_conv_plan* p, const PlanEnv& e) {
    const ctsi_conv_desc& d = p->d;
    // whole 32-channel chunks per source for the 4x4x16 / 4x2x32 kernels; the 512-voxel kernel walks 16-channel chunks,
    // so sources of 16 channels (the U-Net stem: [z | cond] = 2 x latent_dim = 16) can use it too
    const bool c32 = !p->small && d.c1 % 32 == 0 && d.c2 % 32 == 0;
    const bool c16 = d.c1 % 16 == 0 && d.c2 % 16 == 0 && !e.no_c16;
    if (!((c32 || c16) && d.cout >= 64 && d.cout % 8 == 0 && halo_fits(p) && !e.no_halo3)) return;
    if (covers_70(p, H32_4x4x16) || e.force_halo3) {
        // Which of the three halo-tile kernels: the score with the efficiencies of a first pick (16-wide 0.85, 4x2x32 1.0, 4x4x32 /
        // 512 voxels 1.1).  Reproduces every interleaved A/B measurement of profiles/r01_notes.md: 48x128^2 and 48x64^2 -> 512-voxel
        // tile, 48x32^2 x 512 couts -> 4x2x32 (384 big blocks would idle a quarter of the CUs), 48x16^2 and 48x48^2 ->
        // 16-wide, a lone 48x24^2 level (144 blocks either way) -> 512-voxel tile.
        const double s16 = score(p, H32_4x4x16, 1, EFF_PICK_W16), s32 = score(p, H32_4x2x32, 1, EFF_HALO32),
                     s512 = score(p, K32_4x4x32, 1, EFF_PICK_512);
        const double s512w = e.m512w16 == OFF ? 0.0 : score(p, K32_4x8x16, 1, EFF_PICK_512_W16);
        enum { W16, W32, M512 } pick = s16 >= s32 && s16 >= s512 ? W16 : (s32 >= s512 ? W32 : M512);
        bool use_w16 = (s512w > s16 && s512w > s32 && s512w > s512) || e.m512w16 == ON;
        if (e.halo_tile == 16) pick = W16;
        if (e.halo_tile == 32 && pick == W16) pick = s32 >= s512 ? W32 : M512;
        if (e.m512 == OFF && pick == M512) pick = W32;
        if (e.m512 == ON && pick != W16) pick = M512;
        if (!c32 && pick != M512) {   // 16-channel sources: only the 512-voxel kernel applies
            pick = M512;
            use_w16 = s512w > s512;
        }
        if (use_w16 && (!c32 || (e.halo_tile != 16 && e.m512 != OFF))) {
            p->form = &FORMS[K32_4x8x16];
        } else if (pick == M512) {
            // the 512-voxel tile runs on v_mfma_f32_16x16x32_bf16 over tap pairs (conv3_halo_k32.hip: +10-12 % on real data
            // over the 32x32x16 form conv3_halo32m_kernel, which -- with its normalise-on-load experiment -- now lives
            // under csrc/experiments/, outside libctsi.so; profiles/r02_notes.md)
            p->form = &FORMS[K32_4x4x32];
        } else if (pick == W16) {
            // 16-wide levels: tile 4x4x16 (256 voxels) or 3x4x16 (192 voxels) of conv3_halo32_kernel -- whichever fills the 256
            // CUs better (48x16x16 x 512 couts: 192 vs 256 blocks)
            const bool t192 = score(p, H32_3x4x16, 1, EFF_HALO32_192) > score(p, H32_4x4x16, 1, EFF_HALO32);
            p->form = &FORMS[(e.h32w16 ? e.h32w16 == 2 : t192) ? H32_3x4x16 : H32_4x4x16];
        } else {
            p->form = &FORMS[H32_4x2x32];
        }
        // 384-voxel tile (3x4x32, 48 voxels per wave) of the k32 kernel where 512-voxel tiles fill the CUs badly: the
        // 48x32x32 x 512-cout layers are 384 blocks of 512 x 128 (1.5 rounds of the 256 CUs) or 512 blocks of 384 x 128
        // (2 rounds).
        const bool use384 = e.k32_384 == UNSET ? score(p, K32_3x4x32, 1, EFF_K32_384) > defended(p) : e.k32_384 == ON;
        if (use384) p->form = &FORMS[K32_3x4x32];
        // 16-wide levels with deep K and few voxels (48x16x16, 512 -> 512: 192 / 256 / 128 blocks with 512- / 192- / 384-
        // voxel tiles): 3x8x16 = 384 voxels with 2-way split-K = 256 blocks of half the channel chunks each (one round,
        // half the weight bytes per block).  Measured 0.141 ms per half-K block against 0.18 ms for the 192-voxel tile.
        // (round 4: not below 256 input channels -- a half-K block of a 128-channel layer walks 4 chunks, and its prologue,
        //  hand-off and epilogue cost more than the better fill returns: config-3 128 -> 128 @ 4 x 48^3 0.408 ms as
        //  2304 half-K blocks of 3x8x16, 0.331 ms as 864 blocks of 4x8x16; 256 -> 256 equal either way; profiles/r04_notes.md.
        //  CTSI_CONV_K32_SK384_MIN: that threshold, for A/B timing)
        const bool sk_ok = splitk_channels(p);
        bool use_sk = sk_ok && p->Cin >= e.sk384_min && score(p, K32_3x8x16, 2, EFF_K32_384) > defended(p);
        if (e.splitk == SK_OFF) use_sk = false;
        if (e.splitk == SK_ON && sk_ok) use_sk = true;
        // 2-way split-K on the 4x4x32 tile: pays where the 512-voxel grid fills the CUs badly AND K is deep enough to
        // amortise the parked accumulators (256 KB per tile): 1024 -> 512 @48x32x32 1325 -> 1400 TFLOP/s against the
        // 384-voxel tile, 512 -> 512 +0.5 %, 256 -> 512 -7 % (profiles/r02_notes.md).  Round 4: with the direct-store
        // epilogue (which the split-K form takes and the plain 384-voxel tile does not) 512 -> 512 is +5.6 % (1260 ->
        // 1330 TFLOP/s, profiles/r04_notes.md), 256 -> 512 still -3 %: the threshold is 512 input channels now
        const long long b512 = fit(p, FORMS[K32_4x4x32], 1, 1, 1.0).blocks;
        const bool sk512 = sk_ok && p->Cin >= e.sk512_min && p->Wr % 32 == 0 && p->Hr % 4 == 0 && p->Dr % 4 == 0 &&
                           cu_fill(b512) < 0.8 && cu_fill(2 * b512) >= 0.95 && e.splitk != SK_OFF;
        if ((e.splitk == SK_512 && sk_ok) || (sk512 && e.splitk != SK_ON && e.splitk != SK_PLAIN)) {
            p->form = &FORMS[K32_4x4x32];
            p->ksplit = 2;
        } else if (use_sk || e.splitk == SK_PLAIN) {
            p->form = &FORMS[K32_3x8x16];
            p->ksplit = use_sk ? 2 : 1;
        }
    }
    // 24- and 12-wide planes (the 48 x 24^2 / 48 x 12^2 levels of 192^2 patches: config 1, config 3, stitching windows): 16- and
    // 32-wide tiles cover them at 75 %.  The k32 kernel's 384-voxel tiles 4x4x24 / 8x4x12 cover them whole.  Taken only when
    // clearly ahead: 25 stitching windows at once 113 -> 101 ms per U-Net evaluation (L1 + L2 convs 57.9 ->
    // 46.2 ms), while at B = 4 (config 3) the fewer, larger tiles fill the CUs worse (L2: 288 blocks = 1.1 rounds) and
    // the 16-wide tiles stay (measured equal / slower: profiles/r04_notes.md).
    // 2-way split-K on these tiles where it fills the CUs better (B = 4, 48 x 24^2 x 256 couts: 576 blocks = 2.25 rounds ->
    // 1152 = 4.5; 48 x 12^2 x 512 couts: 288 -> 576)
    const double cur = p->form ? defended(p) : EFF_GATHER_STANDIN;
    const bool nsk_ok = splitk_channels(p) && e.narrow_sk != OFF;
    for (const FormId c : {K32_4x4x24, K32_8x4x12}) {
        if (e.narrow == OFF || !narrow_fits(p, FORMS[c])) continue;
        const double s1 = score(p, c, 1, EFF_K32_NARROW), s2 = nsk_ok ? score(p, c, 2, EFF_K32_NARROW) : 0.0;
        const bool sk2 = nsk_ok && (e.narrow_sk == ON || (p->Cin >= e.sk384_min && s2 > 1.1 * s1));
        if (e.narrow == ON || (sk2 ? s2 : s1) > 1.05 * cur) {
            p->form = &FORMS[c];
            p->ksplit = sk2 ? 2 : 0;
            break;
        }
    }
}

// ConvTranspose3d (3,4,4) / (1,2,2) on the k32 kernel: each parity class is a 12-tap convolution on the input grid with
// the 3x3x3 conv's halo tile (conv3_halo_k32.hip, TR = true); 4 classes x n-tiles blocks per input tile.
// Strided Conv3d (3,4,4) / (1,2,2) / pad 1 (Downsample3D, the VAE encoder's DownsampleBlock) on the k32 kernel: the four
// input-parity sub-grids are 3x2x2-tap stride-1 convolutions on the OUTPUT grid's halo tile (conv3_halo_k32.hip, DS = true);
// levels whose grid stays below one round of the 256 CUs with deep K take the 2-way split-K form of the 3x8x16 tile.
// (4x4x24 / 8x4x12: only where the plane divides: 25 stitching windows at once, Upsample + Downsample layers 12.4 -> 11.1 ms)
static void choose_k32_strided_form(ctsi_conv_plan* p, const PlanEnv& e) {
    const ctsi_conv_desc& d = p->d;
    const bool ds = !d.transposed;
    if (!(d.kd == 3 && d.kh == 4 && d.kw == 4 && d.sh == 2 && d.sw == 2 && d.pd == 1 && d.ph == 1 && d.pw == 1 && d.c2 == 0 &&
          d.c1 % 16 == 0 && d.cout >= 64 && d.cout % 8 == 0 && halo_fits(p) && (!ds || (d.hi % 2 == 0 && d.wi % 2 == 0))))
        return;
    const ConvForm* best = nullptr;
    TileFit bf = {0, 0.0, -1.0};
    for (int fi = K32_4x4x32; fi <= K32_8x4x12; ++fi) {   // (the 3x3x3 halo tiles; the planar rows have no depth halo)
        const ConvForm& c = FORMS[fi];
        if (c.tw % 16 != 0 && (!narrow_fits(p, c) || e.narrow == OFF)) continue;
        const TileFit f = fit(p, c, 1, ds ? 1 : 4, form_voxels(c) == 512 ? EFF_ST_512 : EFF_ST_384);
        if (ds && f.useful < 0.7 && !e.force_halo3) continue;   // (a 32-wide tile on a 16-wide plane)
        if (f.score > bf.score) { best = &c; bf = f; }
    }
    if (!(bf.useful >= 0.7 || e.force_halo3) || (ds ? e.k32d : e.k32t) == OFF || e.no_halo3) return;
    p->form = best;   // (never NULL here: a candidate that passed gave bf.useful)
    p->ds = ds;
    if (e.m512w16 != UNSET) p->form = &FORMS[e.m512w16 == ON ? K32_4x8x16 : K32_4x4x32];   // (tuning / test aid)
    if (e.k32_384 != UNSET) p->form = k32_sized(p->form, e.k32_384 == ON);                 // (test aid: a tile of that width)
    if (ds) {
        // split-K: 3x8x16 tiles, two blocks per (tile, n-tile) -- when even the best tile leaves the grid at <= half a
        // round of the CUs (48x16x16 x 512 couts: 128 blocks) and K is deep (48 taps x Cin)
        const long long t5 = fit(p, FORMS[K32_3x8x16], 1, 1, 1.0).blocks;
        bool use_sk = p->Cin % 32 == 0 && p->Cin >= 256 && bf.blocks <= 160 && 2 * t5 <= 512;
        if (e.splitk == SK_OFF) use_sk = false;
        if (e.splitk == SK_ON && p->Cin % 32 == 0) use_sk = true;
        if (use_sk) {
            p->form = &FORMS[K32_3x8x16];
            p->ksplit = 2;
        }
    }
}

// Planar Conv3d (1,3,3) / stride 1 / pad (0,1,1) with whole 16-channel chunks per source and >= 64 couts (the VGG-19 stack of
// the perceptual loss: images along depth) on the k32 kernel's planar form; the gather kernel re-stages the activation slab
// per tap.  Scored like the other forms -- useful tile rows x CU fill x efficiency; a form must cover the row grid at >= 70 %
// (planes too small for a tile stay on the gather kernel, as does the 3 -> 64 stem with its 8 stored channels).  Deep-K layers
// on a grid of at most half a round of the CUs (512 -> 512 over a few dozen 12^2 planes) also stay there: the gather kernel's
// 128-row tiles with S-way split-K (choose_gather_split) put 2-4 x as many blocks on the chip.
static void choose_planar_form(ctsi_conv_plan* p, const PlanEnv& e) {
    const ctsi_conv_desc& d = p->d;
    if (!(!d.transposed && d.kd == 1 && d.kh == 3 && d.kw == 3 && d.sh == 1 && d.sw == 1 && d.pd == 0 && d.ph == 1 && d.pw == 1 &&
          !p->dshift && d.c1 % 16 == 0 && d.c2 % 16 == 0 && d.cout >= 64 && d.cout % 8 == 0 && halo_fits(p)))
        return;
    if (e.planar == 0 || e.no_halo3) return;
    const ConvForm* best = nullptr;
    TileFit bf = {0, 0.0, -1.0};
    for (int f = PL_1x16x32; f <= PL_8x4x12; ++f) {
        const ConvForm& c = FORMS[f];
        if (c.tw % 16 != 0 && !narrow_fits(p, c)) continue;
        if (e.planar >= 16 && c.code != e.planar) continue;
        const TileFit t = fit(p, c, 1, 1, c.eff);
        if (t.useful < 0.7 && e.planar < 16) continue;
        if (t.score > bf.score) { best = &c; bf = t; }
    }
    if (!best) return;
    if (e.planar < 1 && bf.blocks <= 128 && p->Cin >= 256) return;
    p->form = best;
    p->planar = 1;
}

// few output channels (network heads: 128 -> 8, 128 -> 1)
static void choose_head_form(ctsi_conv_plan* p, const PlanEnv& e) {
    const ctsi_conv_desc& d = p->d;
    if (p->form || !is_k3(d) || p->small || d.c2 != 0 || d.c1 % 32 != 0 || d.cout > 16 || !halo_fits(p) || e.no_head3) return;
    if (!covers_70(p, HEAD_4x2x16) && !e.force_halo3) return;
    p->form = &FORMS[HEAD_4x2x16];
    p->head2 = ctsi_conv3_head2_supported(p->Cin, d.cout) && !e.no_head2;
}

// everything that follows from (BM, BN, TD, TH, TW): cout padding and tile counts
static void finish_tiles(ctsi_conv_plan* p) {
    p->CoutPad = ceil_div(p->d.cout, p->BN) * p->BN;
    p->ntiles_n = p->CoutPad / p->BN;
    p->lTH = ilog2(p->TH); p->lTW = ilog2(p->TW);
    p->tilesD = ceil_div(p->Dr, p->TD);
    p->tilesH = ceil_div(p->Hr, p->TH);
    p->tilesW = ceil_div(p->Wr, p->TW);
    p->tps = p->tilesD * p->tilesH * p->tilesW;
    p->mtiles = p->d.n * p->tps;
}

// gather kernel on small planes: a power-of-two box tile over e.g. a 6 x 6 plane is 44 % padding rows; runs of
// BM consecutive voxels have none (only the last tile of a sample is ragged)
static void choose_linear_rows(ctsi_conv_plan* p, const PlanEnv& e) {
    const long long rows = plan_rows(p), boxed = (long long)p->tps * p->BM;
    if (!((boxed * 100 > rows * 115 && e.linear != OFF) || e.linear == ON)) return;
    p->linear = 1;
    p->tps = (int)((rows + p->BM - 1) / p->BM);
    p->mtiles = p->d.n * p->tps;
    p->TD = (int)(p->BM / ((long long)p->Hr * p->Wr)) + 2;   // depth slices one tile can touch (fast-path extent)
}

// S-way split-K on the gather kernel: a layer that is a few dozen blocks (the 6 x 6 level of ONE 192^2 patch: 14 m-tiles
// x 4 n-tiles = 56 blocks on 256 CUs) with hundreds of sequential K-steps is bound by its K-step latency; S blocks
// per tile walk 1 / S of the steps each (csrc/conv_mfma.hip, hand-off by ticket).  CTSI_CONV_GSPLIT = 0 | 2..8 overrides.
static void choose_gather_split(ctsi_conv_plan* p, const PlanEnv& e) {
    if (p->small || p->BM != 128 || p->BN != 128) return;
    const long long blocks = (long long)p->nclass * p->mtiles * p->ntiles_n;
    int S = 0;
    if (blocks * 2 <= 256 && p->ksteps >= 32) {
        S = (int)(256 / blocks);
        if (S > 4) S = 4;
        while (S > 1 && p->ksteps / S < 16) --S;
    } else if (blocks <= 256 && p->ksteps >= 64) {
        S = 2;     // 129-256 blocks: the grid doubles past the ring mode's one-block-per-CU limit, so the two half-K blocks of
    }              // a tile share a CU in the 2-stage mode: 560 -> 700 TFLOP/s on the 6 x 6 level of config 3 (B = 4)
    if (e.has_gsplit) S = e.gsplit >= 2 && e.gsplit <= 8 && p->ksteps >= e.gsplit ? e.gsplit : 0;
    p->gsplit = S >= 2 ? S : 0;
}

extern "C" int ctsi_conv_plan_create(ctsi_conv_plan** out, const ctsi_conv_desc* desc) {
    CTSI_CHECK_ARG(out && desc, "ctsi_conv_plan_create: null argument");
    const ctsi_conv_desc& d = *desc;
    CTSI_CHECK_ARG(d.n > 0 && d.c1 > 0 && d.c2 >= 0 && d.cout > 0 && d.di > 0 && d.hi > 0 && d.wi > 0,
                   "ctsi_conv_plan_create: bad sizes n=%d c1=%d c2=%d cout=%d in=%dx%dx%d", d.n, d.c1,
                   d.c2, d.cout, d.di, d.hi, d.wi);
    CTSI_CHECK_ARG(d.c1 % 8 == 0 && d.c2 % 8 == 0,
                   "ctsi_conv_plan_create: source channel counts must be multiples of 8 (got %d, %d); "
                   "pad the tensor at the layout boundary", d.c1, d.c2);
    CTSI_CHECK_ARG(d.kd >= 1 && d.kh >= 1 && d.kw >= 1 && d.sh >= 1 && d.sw >= 1,
                   "ctsi_conv_plan_create: bad kernel/stride");
    ctsi_conv_plan* p = (ctsi_conv_plan*)calloc(1, sizeof(ctsi_conv_plan));
    CTSI_CHECK_ARG(p, "ctsi_conv_plan_create: out of host memory");
    p->d = d;
    const int rc = plan_geometry(p);
    if (rc != CTSI_OK) {   // the one exit of a refused descriptor
        free(p);
        return rc;
    }
    const PlanEnv e = read_plan_env();
    plan_k_walk(p);
    choose_gather_tile(p, e);
    if (is_k3(d)) choose_k3_form(p, e);
    else if (d.kd == 1 && d.kh == 3) choose_planar_form(p, e);
    else choose_k32_strided_form(p, e);
    choose_head_form(p, e);
    if (p->form) {
        p->BM = form_voxels(*p->form);
        p->BN = p->form->bn;
        p->TD = p->form->td; p->TH = p->form->th; p->TW = p->form->tw;
    } else {
        choose_box_tile(p);
    }
    finish_tiles(p);
    if (!p->form) choose_linear_rows(p, e);
    {   // buffer-addressed fast path: whole 64-channel chunks per source and a tile halo that fits 2^31 bytes
        const int cmax = d.c1 > d.c2 ? d.c1 : d.c2;
        const double extent = ((double)(p->TD + 4) * d.hi * d.wi + 2.0 * d.wi + 8) * cmax * 2.0;
        p->fast = !p->small && d.c1 % 64 == 0 && d.c2 % 64 == 0 && extent < 2.0e9 && !e.no_fast;
    }
    if (!p->form) choose_gather_split(p, e);
    *out = p;
    return CTSI_OK;
}

extern "C" void ctsi_conv_plan_destroy(ctsi_conv_plan* plan) { free(plan); }

extern "C" int ctsi_conv_plan_out_dims(const ctsi_conv_plan* p, int* d, int* h, int* w) {
    CTSI_CHECK_ARG(p, "ctsi_conv_plan_out_dims: null plan");
    if (d) *d = p->Do;
    if (h) *h = p->Ho;
    if (w) *w = p->Wo;
    return CTSI_OK;
}
extern "C" size_t ctsi_conv_plan_weight_bytes(const ctsi_conv_plan* p) {
    if (!p) return 0;
    if (p->stem) return ctsi_conv3_stem_weight_bytes(p->CoutPad);
    if (p->stream1) return (size_t)p->d.cout * p->Cin * 2;
    switch (conv_family(p)) {
    case CONV_HEAD:   // conv3_head's image (8 weight rows when cout <= 8; + 1 KB: its last DMA piece is read whole), then conv3_head2's
        return head1_bytes(p) + (ctsi_conv3_head2_supported(p->Cin, p->d.cout) ? ctsi_conv3_head2_weight_bytes(p->d.cout) : 0);
    case CONV_K32: return ctsi_conv3_halo_k32_weight_bytes(p->Cin, p->CoutPad, p->BN, conv_k32_image(p));   // entries padded to whole steps
    case CONV_HALO32: return (size_t)p->Cin * 27 * p->CoutPad * 2;   // [chunk][27][cout_pad][32 | 16 ch] bf16
    default: return (size_t)p->nclass * p->CoutPad * p->Ktot * 2;
    }
}
extern "C" int ctsi_conv_plan_tiles(const ctsi_conv_plan* p) { return p ? p->nclass * p->mtiles : 0; }
extern "C" int ctsi_conv_plan_tiles_per_sample(const ctsi_conv_plan* p) { return p ? p->tps : 0; }
extern "C" int ctsi_conv_plan_cout_pad(const ctsi_conv_plan* p) { return p ? p->CoutPad : 0; }
extern "C" double ctsi_conv_plan_flops(const ctsi_conv_plan* p) { return p ? p->flops : 0.0; }
extern "C" size_t ctsi_conv_plan_workspace_bytes(const ctsi_conv_plan* p) {
    // split-K plans: tickets / flags + fp32 partial accumulators (ctsi_conv_out.workspace; zero the first 8 * tiles bytes once)
    if (p && !p->form && p->gsplit >= 2) {   // gather kernel: [tile] tickets (padded to 256 B) + [tile][split][128 x 128] fp32
        const size_t tiles = (size_t)p->nclass * p->mtiles * p->ntiles_n;
        return (tiles * 4 + 255) / 256 * 256 + tiles * p->gsplit * (size_t)(128 * 128) * sizeof(float);
    }
    if (!p || p->ksplit != 2) return 0;
    return ctsi_conv3_halo_k32_splitk_bytes(p->mtiles * p->ntiles_n);
}
extern "C" int ctsi_conv_plan_config(const ctsi_conv_plan* p, int* bm, int* bn, int* mode) {
    CTSI_CHECK_ARG(p, "ctsi_conv_plan_config: null plan");
    if (bm) *bm = p->stream1 ? 16 : p->BM;
    if (bn) *bn = p->stream1 ? p->stream1 * 16 : p->BN;
    if (mode) *mode = p->stem ? 11 : p->stream1 ? 10 : (p->form ? p->form->mode : (p->small ? 1 : (p->fast ? 2 : 0)));
    return CTSI_OK;
}

extern "C" int ctsi_conv_plan_form(const ctsi_conv_plan* p, int out[8]) {
    CTSI_CHECK_ARG(p && out, "ctsi_conv_plan_form: null argument");
    memset(out, 0, 8 * sizeof(int));
    out[0] = p->TD; out[1] = p->TH; out[2] = p->TW;
    if (!p->stem && !p->stream1) out[3] = conv_family(p) == CONV_K32 ? p->ksplit : (p->form ? 0 : p->gsplit);
    out[4] = (p->linear ? 1 : 0) | (p->fast ? 2 : 0) | (p->head2 ? 4 : 0) | (p->ds ? 8 : 0) | (p->planar ? 16 : 0);
    return CTSI_OK;
}

// The packed-image layout ctsi_conv_plan_pack_weights writes, beyond the descriptor's channel / kernel fields, the cout
// padding and the weight's cin (see ctsi.h): the kernel family, and for the k32 kernel its form and whether the image is
// cout-permuted for the direct-store epilogue.  Mirrors the branches of ctsi_conv_plan_pack_weights (conv_mfma.hip).
extern "C" int ctsi_conv_plan_pack_layout(const ctsi_conv_plan* p) {
    if (!p) return 0;
    if (p->stem) return CTSI_PACK_STEM;
    if (p->stream1) return CTSI_PACK_STREAM_TAIL | (p->stream1 << 8);
    switch (conv_family(p)) {
    case CONV_K32: return CTSI_PACK_K32 | (conv_k32_image(p) << 4) | (conv_k32_direct(p) << 6) | ((p->BN / 16) << 8);
    case CONV_HEAD: return CTSI_PACK_HEAD | (ctsi_conv3_head2_supported(p->Cin, p->d.cout) ? 1 << 4 : 0);
    case CONV_HALO32: return CTSI_PACK_HALO;
    default: return p->small ? CTSI_PACK_GATHER_SMALL : CTSI_PACK_GATHER;
    }
}

// A 1x1x1 stride-1 conv that will run with the fused GroupNorm tail (ctsi_conv_out.gn_x) or as a plain bf16 conv + bias may
// take the streaming kernel of conv1_stream.hip (another packed-weight layout: call this BEFORE ctsi_conv_plan_weight_bytes /
// _pack_weights).  on = 1 selects it where the layer qualifies (whole 128-channel chunks per source, cout in whole n-tiles)
// and is a no-op otherwise -- ctsi_conv_plan_config reports mode 10 when it is active; on = 0 returns to the gather kernel.
// CTSI_CONV1_STREAM=0 (tuning / test aid) keeps every plan on the gather kernel.
extern "C" int ctsi_conv_plan_set_stream_tail(ctsi_conv_plan* p, int on) {
    CTSI_CHECK_ARG(p, "ctsi_conv_plan_set_stream_tail: null plan");
    p->stream1 = 0;
    if (!on || ctsi_conv1_stream_switch() == 0) return CTSI_OK;
    const ctsi_conv_desc& d = p->d;
    if (d.transposed || d.kd != 1 || d.kh != 1 || d.kw != 1 || d.sh != 1 || d.sw != 1 || d.pd || d.ph || d.pw || p->dshift)
        return CTSI_OK;
    p->stream1 = ctsi_conv1_stream_nt(d.c1, d.c2, d.cout);
    return CTSI_OK;
}

// The weight tensor may carry fewer input channels than the (padded) activation tensor: the
// VAE encoder's first conv sees a 1-channel volume stored as 8 channels (7 zero).
extern "C" int ctsi_conv_plan_set_weight_cin(ctsi_conv_plan* p, int cin_w) {
    CTSI_CHECK_ARG(p && cin_w > 0 && cin_w <= p->Cin, "ctsi_conv_plan_set_weight_cin: bad cin %d", cin_w);
    p->CinW = cin_w;
    // a 3x3x3 stride-1 conv of a ONE-channel volume (the VAE encoder's first layer: the CT volume is stored with 8 channels,
    // 7 of them padding) with >= 64 couts: the 27 taps become the K of one MFMA (conv3_stem.hip); CTSI_CONV_NO_STEM keeps the
    // gather kernel's small-Cin form (A/B timing, tests)
    const ctsi_conv_desc& d = p->d;
    if (cin_w == 1 && is_k3(d) && d.c2 == 0 && d.c1 == 8 && d.cout >= 64 && d.cout % 8 == 0 && !p->dshift &&
        !getenv("CTSI_CONV_NO_STEM")) {
        p->stem = 1;
        p->form = nullptr;
        p->gsplit = 0; p->linear = 0;
        p->BM = 512; p->BN = 128;
        ctsi_conv3_stem_tile(&p->TD, &p->TH, &p->TW);
        finish_tiles(p);
    }
    return CTSI_OK;
}
