// Training-path kernels other than the convolutions (all HBM- or latency-bound):
//   q_sample + Min-SNR-5 weighted MSE loss        models/diffusion.py:81-106, 108-203
//   data-gradient weight re-layout, channel sums (bias gradients), small fp32 Linear backward (time embedding)
// Activations and their gradients are bf16 NDHWC with 16-byte (8-channel) accesses; statistics and parameter
// gradients are fp32 / fp64.  Reductions are two-stage with a fixed order (deterministic, no float atomics).
#include "ctsi_internal.h"
#include "gn_frame.h"

// ==== channel sums (bias gradients) ==================================================================================
// partial[b][c] over row blocks, then out[c] = scale * sum_b partial[b][c]
__global__ void __launch_bounds__(256)
channel_sum_partial_kernel(const bf16_t* __restrict__ x, long long rows, int c, int c_stride,
                           float* __restrict__ partial, long long rows_per_block) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* s_red = reinterpret_cast<float*>(smem_raw);  // [rows_par][c]
    const int cpr = c >> 3;
    const int rows_par = 256 / cpr;
    const int tid = threadIdx.x, q = tid % cpr, rl = tid / cpr;
    const long long v0 = (long long)blockIdx.x * rows_per_block;
    long long v1 = v0 + rows_per_block;
    if (v1 > rows) v1 = rows;
    float a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = 0.0f;
    if (rl < rows_par) {
        long long v = v0 + rl;
        for (; v + 3ll * rows_par < v1; v += 4ll * rows_par) {   // four rows in flight per thread, added in row order
            uint4 raw[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) raw[u] = *reinterpret_cast<const uint4*>(x + (v + (long long)u * rows_par) * c_stride + q * 8);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float f[8];
                gn_unpack8(raw[u], f);
#pragma unroll
                for (int k = 0; k < 8; ++k) a[k] += f[k];
            }
        }
        for (; v < v1; v += rows_par) {
            float f[8];
            gn_unpack8(*reinterpret_cast<const uint4*>(x + v * c_stride + q * 8), f);
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] += f[k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) s_red[rl * c + q * 8 + k] = a[k];
    }
    __syncthreads();
    for (int ch = tid; ch < c; ch += 256) {
        float t = 0.0f;
        for (int r = 0; r < rows_par; ++r) t += s_red[r * c + ch];
        partial[(long long)blockIdx.x * c + ch] = t;
    }
}
// one block = 16 channels x 16 lanes over the row blocks (one serial thread per channel took 50-100 us for the 432 partial rows
// of a 4 x 48^3 tensor); every lane sums its strided subset in order, lane 0 adds the 16 lane sums in order: a fixed order
__global__ void __launch_bounds__(256)
channel_sum_final_kernel(const float* __restrict__ partial, int blocks, int c, float* __restrict__ out, float scale) {
    __shared__ float s_part[16][17];
    const int cl = threadIdx.x & 15, r = threadIdx.x >> 4;
    const int ch = blockIdx.x * 16 + cl;
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
    if (ch < c) {
        int b = r;
        for (; b + 48 < blocks; b += 64) {
            t0 += partial[(long long)b * c + ch];
            t1 += partial[(long long)(b + 16) * c + ch];
            t2 += partial[(long long)(b + 32) * c + ch];
            t3 += partial[(long long)(b + 48) * c + ch];
        }
        for (; b < blocks; b += 16) t0 += partial[(long long)b * c + ch];
    }
    s_part[r][cl] = (t0 + t1) + (t2 + t3);
    __syncthreads();
    if (r == 0 && ch < c) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += s_part[k][cl];
        out[ch] = t * scale;
    }
}
#define CHSUM_ROWS 1024
extern "C" size_t ctsi_channel_sum_workspace_floats(long long rows, int c) {
    return (size_t)(((rows + CHSUM_ROWS - 1) / CHSUM_ROWS) * c);
}
extern "C" int ctsi_channel_sum(const void* x, long long rows, int c, int c_stride, float* workspace, float* out,
                                float scale, void* stream) {
    CTSI_CHECK_ARG(x && workspace && out && rows > 0 && c > 0 && c % 8 == 0 && c <= 2048 && c_stride % 8 == 0 &&
                       c_stride >= c, "ctsi_channel_sum: bad arguments (c=%d stride=%d)", c, c_stride);
    const long long blocks = (rows + CHSUM_ROWS - 1) / CHSUM_ROWS;
    const int rows_par = 256 / (c >> 3);
    hipLaunchKernelGGL(channel_sum_partial_kernel, dim3((unsigned)blocks), dim3(256), (size_t)rows_par * c * sizeof(float),
                       (hipStream_t)stream, (const bf16_t*)x, rows, c, c_stride, workspace, (long long)CHSUM_ROWS);
    CTSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(channel_sum_final_kernel, dim3((c + 15) / 16), dim3(256), 0, (hipStream_t)stream, workspace,
                       (int)blocks, c, out, scale);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ==== small elementwise helpers ======================================================================================
// (one contiguous batch of 4 x 256 16-byte chunks per block, blocks in address order: see ctsi_gn_apply)
__global__ void __launch_bounds__(256) add_bf16_kernel(bf16_t* __restrict__ a, const bf16_t* __restrict__ b, long long chunks) {
    const long long e0 = (long long)blockIdx.x * 1024 + threadIdx.x;
    uint4 ra[4], rb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (e0 + u * 256 < chunks) {
            ra[u] = *reinterpret_cast<const uint4*>(a + (e0 + u * 256) * 8);
            rb[u] = *reinterpret_cast<const uint4*>(b + (e0 + u * 256) * 8);
        }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (e0 + u * 256 < chunks) {
            float fa[8], fb[8];
            gn_unpack8(ra[u], fa);
            gn_unpack8(rb[u], fb);
#pragma unroll
            for (int k = 0; k < 8; ++k) fa[k] += fb[k];
            *reinterpret_cast<uint4*>(a + (e0 + u * 256) * 8) = gn_pack8(fa);
        }
}
extern "C" int ctsi_add_bf16(void* a, const void* b, long long count, void* stream) {
    CTSI_CHECK_ARG(a && b && count >= 0 && count % 8 == 0, "ctsi_add_bf16: count must be a multiple of 8");
    if (count == 0) return CTSI_OK;
    const long long chunks = count / 8;
    const long long blocks = (chunks + 1023) / 1024;
    hipLaunchKernelGGL(add_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (bf16_t*)a,
                       (const bf16_t*)b, chunks);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// fp32 [rows][c] -> bf16 [rows][c]
__global__ void __launch_bounds__(256) f32_to_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long long count) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < count; e += (long long)gridDim.x * 256)
        dst[e] = f32_to_bf16(src[e]);
}
extern "C" int ctsi_f32_to_bf16(const float* src, void* dst, long long count, void* stream) {
    CTSI_CHECK_ARG(src && dst && count >= 0, "ctsi_f32_to_bf16: bad arguments");
    if (count == 0) return CTSI_OK;
    long long blocks = (count + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, count);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// out (cout' = ci_cnt, cin' = cout, T):  out[(ci' * cout + co) * T + (T-1-t)] = w[(co * cin + ci_off + ci') * T + t]
__global__ void __launch_bounds__(256)
weight_dgrad_layout_kernel(const float* __restrict__ w, float* __restrict__ out, int cout, int cin, int taps, int ci_off,
                           int ci_cnt, long long total) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int t = (int)(e % taps);
        const long long r = e / taps;
        const int co = (int)(r % cout);
        const int ci = (int)(r / cout);
        out[e] = w[((long long)co * cin + ci_off + ci) * taps + (taps - 1 - t)];
    }
}
extern "C" int ctsi_weight_dgrad_layout(const float* w, float* out, int cout, int cin, int taps, int ci_off, int ci_cnt,
                                        void* stream) {
    CTSI_CHECK_ARG(w && out && cout > 0 && cin > 0 && taps > 0 && ci_off >= 0 && ci_cnt > 0 && ci_off + ci_cnt <= cin,
                   "ctsi_weight_dgrad_layout: bad arguments");
    const long long total = (long long)ci_cnt * cout * taps;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(weight_dgrad_layout_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, out, cout,
                       cin, taps, ci_off, ci_cnt, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ==== q_sample and the loss ============================================================================================
// z_t = sqrt_ac[t_b] * z0 + sqrt_1mac[t_b] * noise     (fp32 NCDHW in) -> bf16 NDHWC channels [c_off, c_off + c)
__global__ void __launch_bounds__(256)
q_sample_kernel(const float* __restrict__ z0, const float* __restrict__ noise, const float* __restrict__ sqrt_ac,
                const float* __restrict__ sqrt_1mac, const int* __restrict__ t, bf16_t* __restrict__ dst, int c,
                long long vox, int c_total, int c_off, long long total /* n*vox */) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long nb = e / vox, v = e - nb * vox;
        const int tt = t[nb];
        const float a = sqrt_ac[tt], s = sqrt_1mac[tt];
        for (int ch = 0; ch < c; ++ch) {
            const long long i = (nb * c + ch) * vox + v;
            dst[e * c_total + c_off + ch] = f32_to_bf16(a * z0[i] + s * noise[i]);
        }
    }
}
extern "C" int ctsi_q_sample(const float* z0, const float* noise, const float* sqrt_ac, const float* sqrt_1mac,
                             const int* t, void* dst, int n, int c, int d, int h, int w, int c_total, int c_off,
                             void* stream) {
    CTSI_CHECK_ARG(z0 && noise && sqrt_ac && sqrt_1mac && t && dst && n > 0 && c > 0 && c_off >= 0 && c_off + c <= c_total,
                   "ctsi_q_sample: bad arguments");
    const long long vox = (long long)d * h * w, total = vox * n;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(q_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z0, noise, sqrt_ac,
                       sqrt_1mac, t, (bf16_t*)dst, c, vox, c_total, c_off, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// loss = sum_b norm[b] * sum_e mask * (pred - noise)^2.   pred: fp32 NDHWC (n, vox, c); noise: fp32 NCDHW;
// mask: fp32 (n, c, d) or NULL.  Also d_pred (bf16 NDHWC, c_stride channels per voxel) = 2*norm[b]*mask*(pred-noise)*gscale.
// Stage 1: per-block partial sums in double; stage 2 (one block): loss_out[0] = total, loss_out[1+b] = per-sample
// unnormalised sums.
#define LOSS_BLOCKS_PER_SAMPLE 64
__global__ void __launch_bounds__(256)
mse_loss_partial_kernel(const float* __restrict__ pred, const float* __restrict__ noise, const float* __restrict__ mask,
                        int c, long long vox, long long hw, int d, double* __restrict__ partial) {
    __shared__ double s_red[256];
    const int nb = blockIdx.y;
    const long long total = vox * c;
    double acc = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int ch = (int)(e % c);
        const long long v = e / c;
        float df = pred[(long long)nb * total + e] - noise[((long long)nb * c + ch) * vox + v];
        float m = 1.0f;
        if (mask) m = mask[((long long)nb * c + ch) * d + (v / hw)];
        acc += (double)(m * df * df);
    }
    s_red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(long long)nb * gridDim.x + blockIdx.x] = s_red[0];
}
__global__ void mse_loss_final_kernel(const double* __restrict__ partial, const float* __restrict__ norm, int n, int bps,
                                      float* __restrict__ loss_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double total = 0.0;
    for (int b = 0; b < n; ++b) {
        double s = 0.0;
        for (int k = 0; k < bps; ++k) s += partial[(long long)b * bps + k];
        loss_out[1 + b] = (float)s;
        total += (double)norm[b] * s;
    }
    loss_out[0] = (float)total;
}
extern "C" int ctsi_mse_loss_fwd(const float* pred, const float* noise, const float* mask, const float* norm, int n,
                                 int c, int d, int h, int w, double* workspace, float* loss_out, void* stream) {
    CTSI_CHECK_ARG(pred && noise && norm && workspace && loss_out && n > 0 && c > 0, "ctsi_mse_loss_fwd: bad arguments");
    const long long hw = (long long)h * w, vox = hw * d;
    hipLaunchKernelGGL(mse_loss_partial_kernel, dim3(LOSS_BLOCKS_PER_SAMPLE, n), dim3(256), 0, (hipStream_t)stream, pred,
                       noise, mask, c, vox, hw, d, workspace);
    CTSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(mse_loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, workspace, norm, n,
                       LOSS_BLOCKS_PER_SAMPLE, loss_out);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
extern "C" size_t ctsi_mse_loss_workspace_doubles(int n) { return (size_t)n * LOSS_BLOCKS_PER_SAMPLE; }

__global__ void __launch_bounds__(256)
mse_loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ noise, const float* __restrict__ mask,
                    const float* __restrict__ norm, const float* __restrict__ gscale, int c, long long vox, long long hw,
                    int d, bf16_t* __restrict__ dpred, int c_stride, long long total /* n*vox*c_stride */) {
    const float gs = gscale ? gscale[0] : 1.0f;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int ch = (int)(e % c_stride);
        const long long nv = e / c_stride;
        const long long nb = nv / vox, v = nv - nb * vox;
        float out = 0.0f;
        if (ch < c) {
            const float df = pred[nv * c + ch] - noise[(nb * c + ch) * vox + v];
            float m = 1.0f;
            if (mask) m = mask[(nb * c + ch) * d + (v / hw)];
            out = 2.0f * norm[nb] * m * df * gs;
        }
        dpred[e] = f32_to_bf16(out);
    }
}
extern "C" int ctsi_mse_loss_bwd(const float* pred, const float* noise, const float* mask, const float* norm,
                                 const float* gscale, int n, int c, int d, int h, int w, void* dpred, int c_stride,
                                 void* stream) {
    CTSI_CHECK_ARG(pred && noise && norm && dpred && n > 0 && c > 0 && c_stride >= c, "ctsi_mse_loss_bwd: bad arguments");
    const long long hw = (long long)h * w, vox = hw * d, total = vox * n * c_stride;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(mse_loss_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred, noise, mask,
                       norm, gscale, c, vox, hw, d, (bf16_t*)dpred, c_stride, total);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ==== fp32 Linear backward for the time embedding (rows <= 64) ========================================================
// y = act_in(x) W^T + b with act_in = SiLU when silu_in (x is then the pre-activation):
//   dw[o][i] = sum_r dy[r][o] * a[r][i];  db[o] = sum_r dy[r][o];  dx[r][i] = (sum_o dy[r][o] w[o][i]) * act_in'(x[r][i])
__global__ void __launch_bounds__(256)
linear_bwd_w_kernel(const float* __restrict__ x, const float* __restrict__ dy, int rows, int in_dim, int out_dim,
                    int silu_in, float* __restrict__ dw, float* __restrict__ db) {
    const long long total = (long long)out_dim * in_dim;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int o = (int)(e / in_dim), i = (int)(e - (long long)o * in_dim);
        float s = 0.0f;
        for (int r = 0; r < rows; ++r) {
            float a = x[(long long)r * in_dim + i];
            if (silu_in) a = a / (1.0f + expf(-a));
            s += dy[(long long)r * out_dim + o] * a;
        }
        dw[e] = s;
        if (i == 0 && db) {
            float b = 0.0f;
            for (int r = 0; r < rows; ++r) b += dy[(long long)r * out_dim + o];
            db[o] = b;
        }
    }
}
// grid (in_dim/32, rows): 32 consecutive inputs x 8 output lanes per block, LDS reduction over the lanes
__global__ void __launch_bounds__(256)
linear_bwd_x_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ dy, int rows,
                    int in_dim, int out_dim, int silu_in, float* __restrict__ dx) {
    __shared__ float s_red[8][32];
    const int il = threadIdx.x & 31, ol = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + il, r = blockIdx.y;
    float s = 0.0f;
    if (i < in_dim)
        for (int o = ol; o < out_dim; o += 8) s += dy[(long long)r * out_dim + o] * w[(long long)o * in_dim + i];
    s_red[ol][il] = s;
    __syncthreads();
    if (ol == 0 && i < in_dim) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += s_red[k][il];
        if (silu_in) {
            const float z = x[(long long)r * in_dim + i];
            const float sg = 1.0f / (1.0f + expf(-z));
            t *= sg * (1.0f + z * (1.0f - sg));
        }
        dx[(long long)r * in_dim + i] = t;
    }
}
extern "C" int ctsi_linear_bwd(const float* x, const float* w, const float* dy, int rows, int in_dim, int out_dim,
                               int silu_in, float* dw, float* db, float* dx, void* stream) {
    CTSI_CHECK_ARG(x && w && dy && rows > 0 && rows <= 64 && in_dim > 0 && out_dim > 0, "ctsi_linear_bwd: bad arguments");
    if (dw) {
        const long long total = (long long)out_dim * in_dim;
        long long blocks = (total + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(linear_bwd_w_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, dy, rows,
                           in_dim, out_dim, silu_in, dw, db);
        CTSI_LAUNCH_CHECK();
    }
    if (dx) {
        hipLaunchKernelGGL(linear_bwd_x_kernel, dim3((in_dim + 31) / 32, rows), dim3(256), 0, (hipStream_t)stream, x, w, dy,
                           rows, in_dim, out_dim, silu_in, dx);
        CTSI_LAUNCH_CHECK();
    }
    return CTSI_OK;
}

// ==== weight + bias gradients of many SMALL pointwise layers in one launch ============================================
// The 22 pointwise layers inside the 11 TemporalAttention blocks (proj_out and the V third of qkv: models/unet3d.py:152-153,
// 185-190) act on depth-summed tensors of 144-2304 rows: their weight gradients were 22 x (split-K kernel + reduce pass) and
// their bias gradients 22 x (partial + final channel sum) = 88 launches of 5-10 us, 14 TFLOP/s (0.9 ms per config-3 micro-step).
// Their operands are tiny (<= 1.2 MB), so the training engine keeps them until the end of the backward pass and issues ONE
// launch: a block owns a 64 x 64 tile of one layer's dW (and, in the first cin tile, 64 entries of db) and walks ALL rows in
// order -- fp32 FMAs on bf16 operands staged through LDS, no split, no atomics: deterministic.
struct LinGradEntry {
    const bf16_t* x;     // [rows][cin]   layer input
    const bf16_t* dy;    // [rows][cout]  output gradient
    float* dw;           // [cout][dw_stride] (+ element offset applied by the host)
    float* db;           // [cout] or NULL
    int rows, cin, cout, dw_stride;
    float b_scale;
    int pad_;
};
struct LinGradBlock { int entry, ct, it, pad_; };

__global__ void __launch_bounds__(256)
linear_wgrad_multi_kernel(const LinGradEntry* __restrict__ entries, const LinGradBlock* __restrict__ blocks) {
    __shared__ __attribute__((aligned(16))) bf16_t s_dy[32][64 + 8];   // (+8: rows 16 B apart mod 128 B)
    __shared__ __attribute__((aligned(16))) bf16_t s_x[32][64 + 8];
    const LinGradBlock b = blocks[blockIdx.x];
    const LinGradEntry e = entries[b.entry];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int co0 = b.ct * 64, ci0 = b.it * 64;
    const int lr = tid >> 3, lc = (tid & 7) * 8;                        // staging: row lr, 8 channels from lc
    float acc[4][4], bs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bs[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    }
    for (int r0 = 0; r0 < e.rows; r0 += 32) {
        const int r = r0 + lr;
        uint4 vd = make_uint4(0, 0, 0, 0), vx = make_uint4(0, 0, 0, 0);
        if (r < e.rows) {
            if (co0 + lc < e.cout) vd = *reinterpret_cast<const uint4*>(e.dy + (long long)r * e.cout + co0 + lc);
            if (ci0 + lc < e.cin) vx = *reinterpret_cast<const uint4*>(e.x + (long long)r * e.cin + ci0 + lc);
        }
        __syncthreads();
        *reinterpret_cast<uint4*>(&s_dy[lr][lc]) = vd;
        *reinterpret_cast<uint4*>(&s_x[lr][lc]) = vx;
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            const uint2 d2 = *reinterpret_cast<const uint2*>(&s_dy[k][ty * 4]);
            const uint2 x2 = *reinterpret_cast<const uint2*>(&s_x[k][tx * 4]);
            const float dv[4] = {__uint_as_float(d2.x << 16), __uint_as_float(d2.x & 0xffff0000u), __uint_as_float(d2.y << 16),
                                 __uint_as_float(d2.y & 0xffff0000u)};
            const float xv[4] = {__uint_as_float(x2.x << 16), __uint_as_float(x2.x & 0xffff0000u), __uint_as_float(x2.y << 16),
                                 __uint_as_float(x2.y & 0xffff0000u)};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bs[i] += dv[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(dv[i], xv[j], acc[i][j]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = co0 + ty * 4 + i;
        if (co >= e.cout) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ci = ci0 + tx * 4 + j;
            if (ci < e.cin) e.dw[(long long)co * e.dw_stride + ci] = acc[i][j];
        }
        if (e.db != nullptr && b.it == 0 && tx == 0) e.db[co] = bs[i] * e.b_scale;
    }
}

// entries / blocks: device tables built by the caller (n_blocks rows of {entry, cout tile, cin tile}); channel counts multiples of 8
extern "C" int ctsi_linear_wgrad_multi(const void* entries, const void* blocks, int n_blocks, void* stream) {
    CTSI_CHECK_ARG(entries && blocks && n_blocks > 0, "ctsi_linear_wgrad_multi: bad arguments");
    hipLaunchKernelGGL(linear_wgrad_multi_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const LinGradEntry*)entries, (const LinGradBlock*)blocks);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
