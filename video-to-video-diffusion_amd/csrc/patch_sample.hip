// Training patches cut on the device from volumes that stay in HBM: the crop, the depth resample of the
// thick range, the two flips and the rotation by k * 90 degrees of the reference's patch dataset
// (data/patch_slice_interpolation_dataset.py:118-234) as one gather, one launch per batch.
//
// One block moves one 64 x 64 tile of one output slice.  The tile is read in SOURCE order -- rows of the volume, 16-byte lane
// loads along the volume's W -- into LDS, and written in DESTINATION order -- 16-byte stores along the patch's W.  The
// reversal (even k, flips) and the transpose (odd k) happen in the LDS read index, never in a global address pattern.
//
// Alignment: a source row starts at (y * W + x0 + c) elements from the volume's base, so it is 16-byte aligned only by luck
// (fp16 rows are 2-byte aligned).  Every row is cut on the 16-byte grid of its own address: whole chunks inside the window are
// one vector load, the partial chunk at either end is read element by element, and nothing outside the window is read.
//
// LDS banks (cdna_hip_programming.md section 2: ds_write_b32 / ds_read_b32 bank = (a / 4) % 32, conflicts inside a 32-lane
// half): the tile is [64][65] floats.  A half of a wave writes RW rows x LW chunks with RW * LW = 32 and LW * VEC = 32
// columns: address = a * 65 + q * VEC + const, bank = a + q * VEC + const with a over RW consecutive rows and q * VEC over
// LW multiples of VEC >= RW: 32 different banks.  A half reads 4 destination rows x 8 float4 columns; element e of the
// float4 of lane (rr, l) is at  (4 l + e) * 65 +- rr  (odd k: a column of the tile)  or  rr * 65 +- (4 l + e)  (even k: a
// row), bank 4 l +- rr + const: 32 different banks either way.  The pad column is what makes the odd-k case free.
#include "ctsi_internal.h"

#define PS_T 64
#define PS_P 65
#define PS_COLS 12

#define PS_GLOBAL __attribute__((address_space(1)))      // the table carries integers: say that they are global addresses

typedef _Float16 ps_h8 __attribute__((ext_vector_type(8)));
typedef float ps_f4 __attribute__((ext_vector_type(4)));

template <typename ST> struct PsLoad;
template <> struct PsLoad<float> {
    static constexpr int VEC = 4;
    typedef ps_f4 vec_t;
};
template <> struct PsLoad<_Float16> {
    static constexpr int VEC = 8;
    typedef ps_h8 vec_t;
};

template <typename ST>
__global__ void __launch_bounds__(256)
patch_sample_kernel(const long long* __restrict__ table, int depth_thin, int depth_thick, int ph, int pw, int tiles_j,
                    float* __restrict__ out_thin, float* __restrict__ out_thick) {
    constexpr int VEC = PsLoad<ST>::VEC;
    constexpr int CPR = PS_T / VEC;          // chunks of an aligned tile row (one more when the row is off the grid)
    constexpr int LW = 32 / VEC;             // chunks side by side in a 32-lane half: 32 columns
    constexpr int RW = 32 / LW;              // rows of a half
    typedef const ST PS_GLOBAL* src_t;
    typedef const typename PsLoad<ST>::vec_t PS_GLOBAL* vsrc_t;
    __shared__ float tile[PS_T * PS_P];

    const long long* row = table + (long long)blockIdx.z * PS_COLS;
    const int d_thin = (int)row[2], H = (int)row[4], W = (int)row[5];
    const int z = (int)row[6], y0 = (int)row[7], x0 = (int)row[8], k0 = (int)row[9], k1 = (int)row[10];
    const int flags = (int)row[11];
    const int tid = threadIdx.x;

    const bool is_thick = (int)blockIdx.y >= depth_thin;
    const int dd = is_thick ? (int)blockIdx.y - depth_thin : (int)blockIdx.y;
    const int I0 = ((int)blockIdx.x / tiles_j) * PS_T, J0 = ((int)blockIdx.x % tiles_j) * PS_T;
    const int ndi = min(PS_T, ph - I0), ndj = min(PS_T, pw - J0);
    float* out = (is_thick ? out_thick + ((long long)blockIdx.z * depth_thick + dd) * ph * pw
                           : out_thin + ((long long)blockIdx.z * depth_thin + dd) * ph * pw) + (long long)I0 * pw + J0;
    const bool vst = ((pw & 3) == 0) && ((((uintptr_t)out) & 15) == 0);

    // the in-plane map.  flip W, flip H, rot90 k compose to: (u, v) = k odd ? (j, i) : (i, j); source row = RI ? ph-1-u : u;
    // source column = RJ ? pw-1-v : v   (rot90: k = 1 reads C[j, n-1-i], k = 2 C[n-1-i, n-1-j], k = 3 C[n-1-j, i])
    const int kr = (flags >> 2) & 3;
    const bool TR = kr & 1;
    const bool RI = ((flags >> 1) ^ (kr >> 1)) & 1;
    const bool RJ = (flags ^ kr ^ (kr >> 1)) & 1;
    const int nu = TR ? ndj : ndi, nv = TR ? ndi : ndj;      // the tile in (u, v): rows and columns of the source

    const bool pad = !is_thick && z + dd >= d_thin;       // a thin slice past the end of the volume: air
    if (!pad) {
        const int U0 = TR ? J0 : I0, V0 = TR ? I0 : J0;
        const int clo = RJ ? pw - V0 - nv : V0;             // first source column of the tile, in patch coordinates
        const long long plane = (long long)H * W;
        src_t s0, s1;
        float l0 = 1.0f, l1 = 0.0f;
        if (is_thick) {
            // F.interpolate, trilinear, align_corners=False, along depth (H and W keep their size: weights 1 and 0 there)
            const int n_sub = k1 - k0;
            float s = ((float)n_sub / (float)depth_thick) * ((float)dd + 0.5f) - 0.5f;
            if (s < 0.0f) s = 0.0f;
            int i0 = (int)s;
            if (i0 > n_sub - 1) i0 = n_sub - 1;
            const int i1 = i0 + (i0 < n_sub - 1 ? 1 : 0);
            l1 = s - (float)i0;
            l0 = 1.0f - l1;
            s0 = (src_t)row[1] + (long long)(k0 + i0) * plane;
            s1 = (src_t)row[1] + (long long)(k0 + i1) * plane;
        } else {
            s0 = s1 = (src_t)row[0] + (long long)(z + dd) * plane;
        }
        // items: [0, 64 * CPR) the chunks 0 .. CPR-1 of every row, a half of a wave on RW rows x LW chunks;
        //        [64 * CPR, 64 * CPR + 64) chunk CPR of every row (only rows off the 16-byte grid have one)
        for (int item = tid; item < PS_T * CPR + PS_T; item += 256) {
            int a, q;
            if (item < PS_T * CPR) {
                a = (item / (32 * (CPR / LW))) * RW + (item / LW) % RW;
                q = ((item / 32) % (CPR / LW)) * LW + item % LW;
            } else {
                a = item - PS_T * CPR;
                q = CPR;
            }
            if (a >= nu) continue;
            const int u = U0 + a;
            const long long roff = (long long)(y0 + (RI ? ph - 1 - u : u)) * W + x0 + clo;
            const int sh = (int)((((uintptr_t)(s0 + roff)) / sizeof(ST)) & (VEC - 1));     // elements past the 16-byte grid
            const int b0 = q * VEC - sh;                                                  // tile column of the chunk's element 0
            const int lo = b0 < 0 ? -b0 : 0, hi = min(VEC, nv - b0);
            if (hi <= lo) continue;
            src_t p0 = s0 + roff + b0, p1 = s1 + roff + b0;
            float* t = tile + a * PS_P + b0;
            // one 16-byte load per slice when the chunk lies inside the window and (thick) both slices are on the grid
            if (lo == 0 && hi == VEC && ((((uintptr_t)p0) | ((uintptr_t)p1)) & 15) == 0) {
                const typename PsLoad<ST>::vec_t va = *(vsrc_t)p0;
                if (is_thick) {
                    const typename PsLoad<ST>::vec_t vb = *(vsrc_t)p1;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) t[e] = l0 * (float)va[e] + l1 * (float)vb[e];
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) t[e] = (float)va[e];
                }
            } else {                                      // the chunk at an end of the row: element by element
                for (int e = lo; e < hi; ++e)
                    t[e] = is_thick ? l0 * (float)p0[e] + l1 * (float)p1[e] : (float)p0[e];
            }
        }
        __syncthreads();
    }
    // destination order: float4 (i, j .. j+3) is tile[a][bb] at idx0 + e * step -- a row of the tile forwards or backwards
    // (even k), a column (odd k)
    const int step = TR ? PS_P : (RJ ? -1 : 1);
    for (int item = tid; item < PS_T * (PS_T / 4); item += 256) {
        const int di = (item / 64) * 4 + (item / 8) % 4;
        const int dj = (((item / 32) % 2) * 8 + item % 8) * 4;
        if (di >= ndi || dj >= ndj) continue;
        const int b = TR ? di : dj;
        const int idx0 = (TR ? dj : di) * PS_P + (RJ ? nv - 1 - b : b);
        float* o = out + (long long)di * pw + dj;
        if (vst) {                                        // pw is a multiple of 4, and so is ndj: all four are inside
            ps_f4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = pad ? -1.0f : tile[idx0 + e * step];
            *reinterpret_cast<ps_f4*>(o) = v;
        } else {
            for (int e = 0; e < min(4, ndj - dj); ++e) o[e] = pad ? -1.0f : tile[idx0 + e * step];
        }
    }
}

extern "C" int ctsi_patch_sample(const long long* table, int n, int storage, int depth_thin, int depth_thick, int ph, int pw,
                                 float* out_thin, float* out_thick, void* stream) {
    CTSI_CHECK_ARG(table && out_thin, "ctsi_patch_sample: null argument");
    CTSI_CHECK_ARG(aligned_to(table, 8) && aligned_to(out_thin, 4) && aligned_to(out_thick, 4),
                   "ctsi_patch_sample: misaligned table or output");
    CTSI_CHECK_ARG(storage == CTSI_PATCH_F32 || storage == CTSI_PATCH_F16,
                   "ctsi_patch_sample: storage must be CTSI_PATCH_F32 (0) or CTSI_PATCH_F16 (1), got %d", storage);
    CTSI_CHECK_ARG(n >= 1 && n <= 65535, "ctsi_patch_sample: n=%d outside [1, 65535]", n);
    CTSI_CHECK_ARG(depth_thin >= 1 && depth_thick >= 0 && depth_thin + depth_thick <= 65535,
                   "ctsi_patch_sample: bad patch depths thin=%d thick=%d", depth_thin, depth_thick);
    CTSI_CHECK_ARG((depth_thick > 0) == (out_thick != nullptr),
                   "ctsi_patch_sample: a thick output goes with depth_thick > 0 and only with it");
    CTSI_CHECK_ARG(ph >= 1 && pw >= 1 && ph <= 32768 && pw <= 32768, "ctsi_patch_sample: bad patch size %d x %d", ph, pw);
    const int tiles_i = ceil_div(ph, PS_T), tiles_j = ceil_div(pw, PS_T);
    const dim3 grid((unsigned)(tiles_i * tiles_j), (unsigned)(depth_thin + depth_thick), (unsigned)n);
    if (storage == CTSI_PATCH_F16)
        hipLaunchKernelGGL(patch_sample_kernel<_Float16>, grid, dim3(256), 0, (hipStream_t)stream, table, depth_thin,
                           depth_thick, ph, pw, tiles_j, out_thin, out_thick);
    else
        hipLaunchKernelGGL(patch_sample_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, table, depth_thin,
                           depth_thick, ph, pw, tiles_j, out_thin, out_thick);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
