// Differentiable MS-SSIM loss (reference models/losses.py:149-276) on the device: forward and backward, DESIGN.md section 14.
//
//   a = (pred + 1) / 2, b = (target + 1) / 2; every (b, c, d) plane of the contiguous NCDHW tensors is one H x W image.
//   level i (5 levels): SSIM map with the zero-padded Gaussian window (sigma 1.5), mean_i over all planes and pixels;
//   between levels a 2 x 2 average pool (floor).  loss = 1 - prod_i mean_i ^ w_i.
//
// Launches (11 for forward + backward):
//   msssim_fwd_kernel<R>   one per level.  A block owns a 32 x 32 tile of one plane (even origin): a, b with an R-pixel halo
//                          go to LDS, the horizontal pass of the five products (a, b, a^2, b^2, ab) to LDS, the vertical
//                          pass to registers (each thread 4 consecutive rows of one column: 2R + 4 LDS reads per product for
//                          4 outputs).  It writes one fp64 partial of the SSIM sum, the tile of the next level's two pooled
//                          images and -- when a gradient is wanted -- the three coefficient maps
//                            A = dS/dmu1 - 2 mu1 dS/dsigma1^2 - mu2 dS/dsigma12,  Bq = dS/dsigma1^2,  Cq = dS/dsigma12.
//   msssim_finalize_kernel ONE block: the partials of each level added in a fixed order (fp64), the five means, the loss and
//                          the factors f_i = -w_i P / (mean_i N_i).  No atomics anywhere: the same bits on every run.
//   msssim_bwd_kernel<R>   one per level, coarse to fine:
//                            g_i(p) = f_i sum_q w(q - p) [A(q) + 2 a(p) Bq(q) + b(p) Cq(q)] + 1/4 g_{i+1}(p >> 1)
//                          (the adjoint of the zero-padded symmetric window is the same separable filter on the three maps;
//                          the second term is the average pool's backward).  Level 0 multiplies by 1/2 and by the upstream
//                          gradient, read from a device pointer, and writes grad_pred in the tensor's own layout.
// fp32 arithmetic as the reference's, fp64 for every sum over pixels.  (Working on the centred images a - 1/2, b - 1/2, so that
// the moments cancelling in E[a^2] - mu^2 are at most 1/4, was built and measured: no consistent gain in the error against
// float64 -- 0.5x to 1.9x per case -- so the plain form stays.)
#include "ctsi_internal.h"
#include <math.h>

namespace {

constexpr int MS_T = 32;          // tile edge (outputs)
constexpr int MS_RMAX = 7;        // window <= 15
constexpr int MS_LEVELS = 5;
constexpr int MS_NTH = 256;

struct MsWin { float w[2 * MS_RMAX + 1]; };

struct MsLevel { int h, w, tx, ty; long long n, tiles; };   // n = planes * h * w, tiles = planes * tx * ty

struct MsLayout {
    MsLevel lv[MS_LEVELS];
    size_t partial_off[MS_LEVELS];          // doubles
    size_t table_off;                       // 16 floats: f_0..f_4
    size_t img_off[MS_LEVELS][2];           // pooled a, b of levels 1..4
    size_t coef_off[MS_LEVELS];             // A, Bq, Cq of a level, n floats each, back to back
    size_t grad_off[MS_LEVELS];             // g_i of levels 1..4
    size_t bytes;
};

MsLayout ms_layout(long long planes, int h, int w, int want_grad) {
    MsLayout L{};
    size_t off = 0;
    for (int i = 0; i < MS_LEVELS; ++i) {
        MsLevel& v = L.lv[i];
        v.h = h >> i; v.w = w >> i;
        v.tx = (v.w + MS_T - 1) / MS_T; v.ty = (v.h + MS_T - 1) / MS_T;
        v.n = planes * v.h * v.w;
        v.tiles = planes * v.tx * v.ty;
        L.partial_off[i] = off;
        off += (size_t)v.tiles * sizeof(double);
    }
    L.table_off = off;
    off += 64;
    for (int i = 1; i < MS_LEVELS; ++i)
        for (int k = 0; k < 2; ++k) { L.img_off[i][k] = off; off += (size_t)L.lv[i].n * 4; }
    if (want_grad) {
        for (int i = 0; i < MS_LEVELS; ++i) { L.coef_off[i] = off; off += (size_t)L.lv[i].n * 12; }
        for (int i = 1; i < MS_LEVELS; ++i) { L.grad_off[i] = off; off += (size_t)L.lv[i].n * 4; }
    }
    L.bytes = off;
    return L;
}

// g[x] = exp(-(x - R)^2 / (2 * 1.5^2)) rounded to fp32, divided in fp32 by the correctly rounded fp32 sum of those values
// (losses.py:177-183; torch's own fp32 sum gives these bits for every odd size up to 13, the default 11 among them)
MsWin ms_window(int R) {
    MsWin win{};
    float g[2 * MS_RMAX + 1];
    double dsum = 0.0;
    for (int x = 0; x <= 2 * R; ++x) {
        g[x] = (float)exp(-(double)((x - R) * (x - R)) / (2.0 * 1.5 * 1.5));
        dsum += (double)g[x];
    }
    const float sum = (float)dsum;
    for (int x = 0; x <= 2 * R; ++x) win.w[x] = g[x] / sum;
    return win;
}

template <int R>
__global__ void __launch_bounds__(MS_NTH)
msssim_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int h, int w, int level0, MsWin win,
                  double* __restrict__ partial, float* __restrict__ pool_a, float* __restrict__ pool_b,
                  float* __restrict__ coef) {
    constexpr int TS = MS_T + 2 * R;
    __shared__ float s_in[2][TS][TS + 1];
    __shared__ float s_h[5][TS][MS_T];
    __shared__ double s_red[MS_NTH];
    const int tid = threadIdx.x;
    const long long plane = blockIdx.z, hw = (long long)h * w;
    const int x0 = blockIdx.x * MS_T, y0 = blockIdx.y * MS_T;
    const float* pa = a + plane * hw;
    const float* pb = b + plane * hw;
    for (int e = tid; e < TS * TS; e += MS_NTH) {
        const int ty = e / TS, tx = e - ty * TS;
        const int y = y0 + ty - R, x = x0 + tx - R;
        float va = 0.0f, vb = 0.0f;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            va = pa[(long long)y * w + x];
            vb = pb[(long long)y * w + x];
            if (level0) { va = (va + 1.0f) * 0.5f; vb = (vb + 1.0f) * 0.5f; }
        }
        s_in[0][ty][tx] = va;
        s_in[1][ty][tx] = vb;
    }
    __syncthreads();
    // the next level's images: one pooled pixel per thread (16 x 16 per tile)
    if (pool_a) {
        const int px = tid & 15, py = tid >> 4;
        const int h2 = h >> 1, w2 = w >> 1;
        const int gx = (x0 >> 1) + px, gy = (y0 >> 1) + py;
        if (gx < w2 && gy < h2) {
            const int ly = R + 2 * py, lx = R + 2 * px;
            const long long o = plane * h2 * w2 + (long long)gy * w2 + gx;
            pool_a[o] = (s_in[0][ly][lx] + s_in[0][ly][lx + 1] + s_in[0][ly + 1][lx] + s_in[0][ly + 1][lx + 1]) * 0.25f;
            pool_b[o] = (s_in[1][ly][lx] + s_in[1][ly][lx + 1] + s_in[1][ly + 1][lx] + s_in[1][ly + 1][lx + 1]) * 0.25f;
        }
    }
    // horizontal pass
    for (int e = tid; e < TS * MS_T; e += MS_NTH) {
        const int r = e >> 5, c = e & 31;
        float sa = 0.0f, sb = 0.0f, saa = 0.0f, sbb = 0.0f, sab = 0.0f;
#pragma unroll
        for (int j = 0; j <= 2 * R; ++j) {
            const float va = s_in[0][r][c + j], vb = s_in[1][r][c + j], wj = win.w[j];
            sa += wj * va; sb += wj * vb; saa += wj * (va * va); sbb += wj * (vb * vb); sab += wj * (va * vb);
        }
        s_h[0][r][c] = sa; s_h[1][r][c] = sb; s_h[2][r][c] = saa; s_h[3][r][c] = sbb; s_h[4][r][c] = sab;
    }
    __syncthreads();
    // vertical pass: column lx, rows 4 * ry .. 4 * ry + 3
    const int lx = tid & 31, ry = tid >> 5;
    float acc[5][4];
#pragma unroll
    for (int p = 0; p < 5; ++p)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[p][k] = 0.0f;
#pragma unroll
    for (int j = 0; j < 2 * R + 4; ++j) {
        float v[5];
#pragma unroll
        for (int p = 0; p < 5; ++p) v[p] = s_h[p][4 * ry + j][lx];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j - k >= 0 && j - k <= 2 * R) {
#pragma unroll
                for (int p = 0; p < 5; ++p) acc[p][k] += win.w[j - k] * v[p];
            }
    }
    const float C1 = 1e-4f, C2 = 9e-4f;
    double sum = 0.0;
    const int x = x0 + lx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = y0 + 4 * ry + k;
        if (x < w && y < h) {
            const float mu1 = acc[0][k], mu2 = acc[1][k];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = acc[2][k] - mu1_sq, s2 = acc[3][k] - mu2_sq, s12 = acc[4][k] - mu12;
            const float n1 = 2.0f * mu12 + C1, n2 = 2.0f * s12 + C2;
            const float d1 = mu1_sq + mu2_sq + C1, d2 = s1 + s2 + C2;
            const float inv = 1.0f / (d1 * d2);
            const float S = (n1 * n2) * inv;
            sum += (double)S;
            if (coef) {
                const float dmu1 = 2.0f * mu2 * n2 * inv - 2.0f * mu1 * S / d1;
                const float dv1 = -S / d2;
                const float dv12 = 2.0f * n1 * inv;
                const long long o = plane * hw + (long long)y * w + x;
                const long long n = (long long)gridDim.z * hw;
                coef[o] = dmu1 - 2.0f * mu1 * dv1 - mu2 * dv12;
                coef[n + o] = dv1;
                coef[2 * n + o] = dv12;
            }
        }
    }
    s_red[tid] = sum;
    __syncthreads();
    for (int s = MS_NTH / 2; s > 0; s >>= 1) {
        if (tid < s) s_red[tid] += s_red[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[((long long)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s_red[0];
}

struct MsFinal {
    long long tiles[MS_LEVELS];
    long long off[MS_LEVELS];     // doubles from the workspace base
    double count[MS_LEVELS];
};

__global__ void __launch_bounds__(MS_NTH)
msssim_finalize_kernel(const double* __restrict__ ws, MsFinal q, float* __restrict__ out, float* __restrict__ table) {
    __shared__ double s_red[MS_NTH];
    __shared__ double s_mean[MS_LEVELS];
    const int tid = threadIdx.x;
    for (int i = 0; i < MS_LEVELS; ++i) {
        const double* src = ws + q.off[i];
        double acc = 0.0;
        for (long long t = tid; t < q.tiles[i]; t += MS_NTH) acc += src[t];
        s_red[tid] = acc;
        __syncthreads();
        for (int s = MS_NTH / 2; s > 0; s >>= 1) {
            if (tid < s) s_red[tid] += s_red[tid + s];
            __syncthreads();
        }
        if (tid == 0) s_mean[i] = s_red[0] / q.count[i];
        __syncthreads();
    }
    if (tid == 0) {
        const double wt[MS_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
        double P = 1.0;
        for (int i = 0; i < MS_LEVELS; ++i) P *= pow(s_mean[i], (double)(float)wt[i]);   // a negative mean: NaN, as torch.pow
        out[0] = (float)(1.0 - P);
        for (int i = 0; i < MS_LEVELS; ++i) {
            out[1 + i] = (float)s_mean[i];
            table[i] = (float)(-(double)(float)wt[i] * P / (s_mean[i] * q.count[i]));
        }
    }
}

template <int R>
__global__ void __launch_bounds__(MS_NTH)
msssim_bwd_kernel(const float* __restrict__ coef, const float* __restrict__ a, const float* __restrict__ b, int h, int w,
                  int level0, MsWin win, const float* __restrict__ table, const float* __restrict__ gnext,
                  float* __restrict__ gout, const float* __restrict__ upstream) {
    constexpr int TS = MS_T + 2 * R;
    __shared__ float s_in[3][TS][TS + 1];
    __shared__ float s_h[3][TS][MS_T];
    const int tid = threadIdx.x;
    const long long plane = blockIdx.z, hw = (long long)h * w, n = (long long)gridDim.z * hw;
    const int x0 = blockIdx.x * MS_T, y0 = blockIdx.y * MS_T;
    const float* pc = coef + plane * hw;
    for (int e = tid; e < TS * TS; e += MS_NTH) {
        const int ty = e / TS, tx = e - ty * TS;
        const int y = y0 + ty - R, x = x0 + tx - R;
        float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const long long o = (long long)y * w + x;
            v0 = pc[o]; v1 = pc[n + o]; v2 = pc[2 * n + o];
        }
        s_in[0][ty][tx] = v0; s_in[1][ty][tx] = v1; s_in[2][ty][tx] = v2;
    }
    __syncthreads();
    for (int e = tid; e < TS * MS_T; e += MS_NTH) {
        const int r = e >> 5, c = e & 31;
        float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
#pragma unroll
        for (int j = 0; j <= 2 * R; ++j) {
            const float wj = win.w[j];
            t0 += wj * s_in[0][r][c + j]; t1 += wj * s_in[1][r][c + j]; t2 += wj * s_in[2][r][c + j];
        }
        s_h[0][r][c] = t0; s_h[1][r][c] = t1; s_h[2][r][c] = t2;
    }
    __syncthreads();
    const int lx = tid & 31, ry = tid >> 5;
    float acc[3][4];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[p][k] = 0.0f;
#pragma unroll
    for (int j = 0; j < 2 * R + 4; ++j) {
        float v[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) v[p] = s_h[p][4 * ry + j][lx];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j - k >= 0 && j - k <= 2 * R) {
#pragma unroll
                for (int p = 0; p < 3; ++p) acc[p][k] += win.w[j - k] * v[p];
            }
    }
    const float f = table[0];
    const float up = upstream ? upstream[0] : 1.0f;
    const int h2 = h >> 1, w2 = w >> 1;
    const int x = x0 + lx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = y0 + 4 * ry + k;
        if (x < w && y < h) {
            const long long o = plane * hw + (long long)y * w + x;
            float va = a[o], vb = b[o];
            if (level0) { va = (va + 1.0f) * 0.5f; vb = (vb + 1.0f) * 0.5f; }
            float g = f * (acc[0][k] + 2.0f * va * acc[1][k] + vb * acc[2][k]);
            if (gnext && (y >> 1) < h2 && (x >> 1) < w2)
                g += 0.25f * gnext[plane * h2 * w2 + (long long)(y >> 1) * w2 + (x >> 1)];
            if (level0) g = (g * 0.5f) * up;    // d a / d pred = 1/2 (exact), then ONE multiplication by the upstream scalar
            gout[o] = g;
        }
    }
}

const char* ms_check(const char* fn, const void* pred, const void* target, long long planes, int h, int w, int window) {
    (void)fn;
    if (!pred || !target) return "bad arguments";
    if (planes <= 0 || planes > 65535) return "planes must be in [1, 65535]";
    if (h < 16 || w < 16) return "min(h, w) must be at least 16 (five levels)";
    if (h > 32768 || w > 32768) return "h, w must be at most 32768";
    if (window < 1 || !(window & 1) || window / 2 > MS_RMAX) return "window must be odd and at most 15";
    return nullptr;
}

#define MS_DISPATCH(R, CALL)                     \
    switch (R) {                                 \
        case 0: { constexpr int RR = 0; CALL; } break; \
        case 1: { constexpr int RR = 1; CALL; } break; \
        case 2: { constexpr int RR = 2; CALL; } break; \
        case 3: { constexpr int RR = 3; CALL; } break; \
        case 4: { constexpr int RR = 4; CALL; } break; \
        case 5: { constexpr int RR = 5; CALL; } break; \
        case 6: { constexpr int RR = 6; CALL; } break; \
        default: { constexpr int RR = 7; CALL; } break; \
    }

}  // namespace

extern "C" size_t ctsi_msssim_workspace_bytes(int planes, int h, int w, int window, int want_grad) {
    static const float dummy = 0.0f;
    const char* why = ms_check("ctsi_msssim_workspace_bytes", &dummy, &dummy, planes, h, w, window);
    if (why) {
        ctsi_set_error("ctsi_msssim_workspace_bytes: %s", why);
        return 0;
    }
    return ms_layout(planes, h, w, want_grad).bytes;
}

extern "C" int ctsi_msssim_fwd(const float* pred, const float* target, int planes, int h, int w, int window, int want_grad,
                               void* workspace, float* out, void* stream) {
    const char* why = ms_check("ctsi_msssim_fwd", pred, target, planes, h, w, window);
    CTSI_CHECK_ARG(!why, "ctsi_msssim_fwd: %s", why);
    CTSI_CHECK_ARG(workspace && out, "ctsi_msssim_fwd: bad arguments");
    const MsLayout L = ms_layout(planes, h, w, want_grad);
    const int R = window / 2;
    const MsWin win = ms_window(R);
    char* ws = (char*)workspace;
    for (int i = 0; i < MS_LEVELS; ++i) {
        const MsLevel& v = L.lv[i];
        const float* a = i ? (const float*)(ws + L.img_off[i][0]) : pred;
        const float* b = i ? (const float*)(ws + L.img_off[i][1]) : target;
        float* na = i + 1 < MS_LEVELS ? (float*)(ws + L.img_off[i + 1][0]) : nullptr;
        float* nb = i + 1 < MS_LEVELS ? (float*)(ws + L.img_off[i + 1][1]) : nullptr;
        float* coef = want_grad ? (float*)(ws + L.coef_off[i]) : nullptr;
        const dim3 grid(v.tx, v.ty, (unsigned)planes);
        MS_DISPATCH(R, hipLaunchKernelGGL(msssim_fwd_kernel<RR>, grid, dim3(MS_NTH), 0, (hipStream_t)stream, a, b, v.h, v.w,
                                          (int)(i == 0), win, (double*)(ws + L.partial_off[i]), na, nb, coef));
        CTSI_LAUNCH_CHECK();
    }
    MsFinal q;
    for (int i = 0; i < MS_LEVELS; ++i) {
        q.tiles[i] = L.lv[i].tiles;
        q.off[i] = (long long)(L.partial_off[i] / sizeof(double));
        q.count[i] = (double)L.lv[i].n;
    }
    hipLaunchKernelGGL(msssim_finalize_kernel, dim3(1), dim3(MS_NTH), 0, (hipStream_t)stream, (const double*)ws, q, out,
                       (float*)(ws + L.table_off));
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

extern "C" int ctsi_msssim_bwd(const float* pred, const float* target, int planes, int h, int w, int window, void* workspace,
                               const float* grad_loss, float* grad_pred, void* stream) {
    const char* why = ms_check("ctsi_msssim_bwd", pred, target, planes, h, w, window);
    CTSI_CHECK_ARG(!why, "ctsi_msssim_bwd: %s", why);
    CTSI_CHECK_ARG(workspace && grad_loss && grad_pred, "ctsi_msssim_bwd: bad arguments");
    const MsLayout L = ms_layout(planes, h, w, 1);
    const int R = window / 2;
    const MsWin win = ms_window(R);
    char* ws = (char*)workspace;
    const float* table = (const float*)(ws + L.table_off);
    for (int i = MS_LEVELS - 1; i >= 0; --i) {
        const MsLevel& v = L.lv[i];
        const float* a = i ? (const float*)(ws + L.img_off[i][0]) : pred;
        const float* b = i ? (const float*)(ws + L.img_off[i][1]) : target;
        const float* gnext = i + 1 < MS_LEVELS ? (const float*)(ws + L.grad_off[i + 1]) : nullptr;
        float* gout = i ? (float*)(ws + L.grad_off[i]) : grad_pred;
        const dim3 grid(v.tx, v.ty, (unsigned)planes);
        MS_DISPATCH(R, hipLaunchKernelGGL(msssim_bwd_kernel<RR>, grid, dim3(MS_NTH), 0, (hipStream_t)stream,
                                          (const float*)(ws + L.coef_off[i]), a, b, v.h, v.w, (int)(i == 0), win, table + i,
                                          gnext, gout, i ? (const float*)nullptr : grad_loss));
        CTSI_LAUNCH_CHECK();
    }
    return CTSI_OK;
}
