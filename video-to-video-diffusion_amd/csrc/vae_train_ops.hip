// VAE training kernels (the backward of SliceInterpolationVAE.forward, see vae_train_engine.py):
//   ctsi_vae_head_grad   the tanh head's output gradient / the encoder-output gradient at the latent seam
//   ctsi_thin_wgrad      weight gradient of a 3x3x3 stride-1 'same' conv with ONE input channel (the stem) or ONE output
//                        channel (the head): a direct two-pass reduction instead of the MFMA kernel on 8x padded channels
#include "ctsi_internal.h"

// ==== head / seam gradient ================================================================================================
// mode 0: dst[b][v][ch] = bf16(scale * g[b][ch][v] * (1 - y[b][ch][v]^2)) for ch < c, 0 for c <= ch < c_stride
// mode 1: dst[b][v][ch] = bf16(dst[b][v][ch] + scale * g[b][ch][v]) for ch < c; channels >= c untouched (y unused)
// One thread per voxel and 8-channel chunk: the NCDHW reads are coalesced along the voxels, the NDHWC store is 16 bytes.
__global__ void __launch_bounds__(256)
vae_head_grad_kernel(const float* __restrict__ g, const float* __restrict__ y, bf16_t* __restrict__ dst, int c, int c_stride,
                     long long vox, long long total /* n*vox */, float scale, int mode) {
    const int chunks = c_stride >> 3;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total * chunks; e += (long long)gridDim.x * 256) {
        const long long r = e % total;           // voxel index over (n, vox): consecutive threads, consecutive voxels
        const int q = (int)(e / total);          // channel chunk
        const long long b = r / vox, v = r - b * vox;
        bf16_t* o = dst + r * c_stride + q * 8;
        float f[8];
        if (mode == 1) {
            const uint4 old = *reinterpret_cast<const uint4*>(o);
            const uint32_t ow[4] = {old.x, old.y, old.z, old.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) f[k] = bf16_to_f32((bf16_t)(ow[k >> 1] >> (16 * (k & 1))));
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int ch = q * 8 + k;
            if (ch < c) {
                const long long i = (b * c + ch) * vox + v;
                const float gv = g[i];
                if (mode == 0) {
                    const float yv = y[i];
                    f[k] = scale * gv * (1.0f - yv * yv);
                } else {
                    f[k] += scale * gv;
                }
            } else if (mode == 0) {
                f[k] = 0.0f;
            }
        }
        uint4 out;
        out.x = pack_bf16x2(f[0], f[1]); out.y = pack_bf16x2(f[2], f[3]);
        out.z = pack_bf16x2(f[4], f[5]); out.w = pack_bf16x2(f[6], f[7]);
        *reinterpret_cast<uint4*>(o) = out;
    }
}

extern "C" int ctsi_vae_head_grad(const float* g, const float* y, int n, int c, int d, int h, int w, float scale, int mode,
                                  void* dst, int c_stride, void* stream) {
    CTSI_CHECK_ARG(g && dst && n > 0 && c > 0 && d > 0 && h > 0 && w > 0, "ctsi_vae_head_grad: bad arguments");
    CTSI_CHECK_ARG(mode == 0 || mode == 1, "ctsi_vae_head_grad: mode must be 0 (tanh head) or 1 (add)");
    CTSI_CHECK_ARG(mode == 1 || y, "ctsi_vae_head_grad: mode 0 needs the saved tanh output y");
    CTSI_CHECK_ARG(c_stride >= c && c_stride % 8 == 0, "ctsi_vae_head_grad: channel stride %d must be >= c (%d) and a "
                   "multiple of 8", c_stride, c);
    CTSI_CHECK_ARG(((uintptr_t)dst & 15) == 0, "ctsi_vae_head_grad: dst must be 16-byte aligned");
    const long long vox = (long long)d * h * w, total = vox * n;
    long long blocks = (total * (c_stride / 8) + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(vae_head_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, y, (bf16_t*)dst,
                       c, c_stride, vox, total, scale, mode);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ==== thin-channel weight gradient ========================================================================================
// S[c][t] = sum_u wide[u][c] * thin[u + off(t)]   (off(t) = (kd-1, kh-1, kw-1) for tap t = (kd*3 + kh)*3 + kw; zero outside)
//   stem (cin = 1):  wide = output gradient, thin = layer input            dW[c][0][t] = scale * S[c][t]
//   head (cout = 1): wide = layer input,     thin = output gradient        dW[0][c][t] = scale * S[c][26 - t]
// Both weight layouts are dw[c * 27 + t].  Pass 1: one block per (sample, depth slice, TW_ROWS rows); the thin tile with its
// one-voxel halo sits in LDS as fp32; each thread owns one channel and a share of the tile's rows and slides a 3x3 column
// window along w (9 LDS reads per 27 FMAs); partial sums per block go to the workspace.  Pass 2 sums the blocks in a fixed
// order (deterministic).
#define TW_ROWS 4
#define TW_MAX_LDS 65536

static long long thin_wgrad_blocks(int n, int d, int h) { return (long long)n * d * ((h + TW_ROWS - 1) / TW_ROWS); }
static size_t thin_wgrad_lds(int w) { return (size_t)3 * (TW_ROWS + 2) * (w + 2) * sizeof(float); }

__global__ void __launch_bounds__(256)
thin_wgrad_partial_kernel(const bf16_t* __restrict__ wide, int c, int c_stride, const bf16_t* __restrict__ thin,
                          int thin_stride, int d, int h, int w, float* __restrict__ partial) {
    extern __shared__ float s_thin[];         // [3][TW_ROWS + 2][w + 2]
    const int hb = (h + TW_ROWS - 1) / TW_ROWS;
    const int blk = blockIdx.x;
    const int b = blk / (d * hb), rem = blk - b * d * hb;
    const int z = rem / hb, h0 = (rem - (rem / hb) * hb) * TW_ROWS;
    const int wp = w + 2, rows = TW_ROWS + 2;
    for (int i = threadIdx.x; i < 3 * rows * wp; i += 256) {
        const int dz = i / (rows * wp), r2 = i - dz * rows * wp;
        const int hr = r2 / wp, wc = r2 - hr * wp;
        const int zz = z + dz - 1, hh = h0 + hr - 1, ww = wc - 1;
        float v = 0.0f;
        if (zz >= 0 && zz < d && hh >= 0 && hh < h && ww >= 0 && ww < w)
            v = bf16_to_f32(thin[((((long long)b * d + zz) * h + hh) * w + ww) * thin_stride]);
        s_thin[i] = v;
    }
    __syncthreads();
    const int lanes = 256 / c;                // c divides 256 (checked on the host)
    const int ch = threadIdx.x % c, lane = threadIdx.x / c;
    float acc[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) acc[t] = 0.0f;
    if (lane < lanes) {
        // work items: (row, column segment); a lane takes items lane, lane + lanes, ...
        const int segs = lanes > TW_ROWS ? lanes / TW_ROWS : 1;
        const int seg_w = (w + segs - 1) / segs;
        for (int item = lane; item < TW_ROWS * segs; item += lanes) {
            const int r = item % TW_ROWS, sg = item / TW_ROWS;
            const int hh = h0 + r;
            if (hh >= h) continue;
            const int w_lo = sg * seg_w, w_hi = min(w, w_lo + seg_w);
            if (w_lo >= w_hi) continue;
            const bf16_t* wrow = wide + ((((long long)b * d + z) * h + hh) * w) * c_stride + ch;
            // column window win[dz][dh][dw] = s_thin[dz][r + dh][x + dw] for the current x (tile columns are offset by one)
            float win[3][3][3];
#pragma unroll
            for (int dz = 0; dz < 3; ++dz)
#pragma unroll
                for (int dh = 0; dh < 3; ++dh) {
                    const float* sr = s_thin + (dz * rows + r + dh) * wp + w_lo;
                    win[dz][dh][0] = 0.0f;
                    win[dz][dh][1] = sr[0];
                    win[dz][dh][2] = sr[1];
                }
            for (int x = w_lo; x < w_hi; ++x) {
#pragma unroll
                for (int dz = 0; dz < 3; ++dz)
#pragma unroll
                    for (int dh = 0; dh < 3; ++dh) {
                        win[dz][dh][0] = win[dz][dh][1];
                        win[dz][dh][1] = win[dz][dh][2];
                        win[dz][dh][2] = s_thin[(dz * rows + r + dh) * wp + x + 2];
                    }
                const float gv = bf16_to_f32(wrow[(long long)x * c_stride]);
#pragma unroll
                for (int dz = 0; dz < 3; ++dz)
#pragma unroll
                    for (int dh = 0; dh < 3; ++dh)
#pragma unroll
                        for (int dw = 0; dw < 3; ++dw) acc[(dz * 3 + dh) * 3 + dw] += gv * win[dz][dh][dw];
            }
        }
    }
    // fixed-order reduction over the lanes of a channel (through LDS, after the tile is no longer needed)
    __syncthreads();
    float* s_red = s_thin;                     // needs 256 * 27 floats: the host sizes LDS for that too
    for (int t = 0; t < 27; ++t) s_red[t * 256 + threadIdx.x] = acc[t];
    __syncthreads();
    for (int i = threadIdx.x; i < c * 27; i += 256) {
        const int cc = i / 27, t = i - cc * 27;
        float s = 0.0f;
        for (int l = 0; l < lanes; ++l) s += s_red[t * 256 + l * c + cc];
        partial[(long long)blk * c * 27 + i] = s;
    }
}

__global__ void __launch_bounds__(256)
thin_wgrad_reduce_kernel(const float* __restrict__ partial, long long nblk, int c, float scale, int flip, float* __restrict__ dw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c * 27) return;
    float s = 0.0f;
    for (long long k = 0; k < nblk; ++k) s += partial[k * c * 27 + i];
    const int cc = i / 27, t = i - cc * 27;
    dw[cc * 27 + (flip ? 26 - t : t)] = scale * s;
}

extern "C" size_t ctsi_thin_wgrad_workspace_bytes(int n, int c, int d, int h, int w) {
    if (n <= 0 || c <= 0 || d <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)thin_wgrad_blocks(n, d, h) * c * 27 * sizeof(float);
}

extern "C" int ctsi_thin_wgrad_supported(int c, int w, int kd, int kh, int kw) {
    const size_t lds = thin_wgrad_lds(w) > 256 * 27 * sizeof(float) ? thin_wgrad_lds(w) : 256 * 27 * sizeof(float);
    return kd == 3 && kh == 3 && kw == 3 && c >= 8 && c <= 256 && c % 8 == 0 && 256 % c == 0 && w > 0 && lds <= TW_MAX_LDS;
}

extern "C" int ctsi_thin_wgrad(const void* wide, int c, int c_stride, const void* thin, int thin_stride, int head, int n, int d,
                               int h, int w, int kd, int kh, int kw, void* workspace, size_t workspace_bytes, float* dw,
                               float scale, void* stream) {
    CTSI_CHECK_ARG(wide && thin && dw && workspace, "ctsi_thin_wgrad: null pointer");
    CTSI_CHECK_ARG(n > 0 && d > 0 && h > 0 && w > 0 && c > 0, "ctsi_thin_wgrad: bad shape");
    CTSI_CHECK_ARG(c_stride >= c && thin_stride >= 1, "ctsi_thin_wgrad: channel stride %d < channels %d (or thin stride %d < 1)",
                   c_stride, c, thin_stride);
    CTSI_CHECK_ARG(ctsi_thin_wgrad_supported(c, w, kd, kh, kw), "ctsi_thin_wgrad: unsupported geometry (kernel %dx%dx%d, "
                   "c=%d, w=%d): needs a 3x3x3 kernel, c a multiple of 8 dividing 256, w <= 908", kd, kh, kw, c, w);
    CTSI_CHECK_ARG(workspace_bytes >= ctsi_thin_wgrad_workspace_bytes(n, c, d, h, w), "ctsi_thin_wgrad: workspace too small");
    const long long nblk = thin_wgrad_blocks(n, d, h);
    size_t lds = thin_wgrad_lds(w);
    if (lds < 256 * 27 * sizeof(float)) lds = 256 * 27 * sizeof(float);
    hipLaunchKernelGGL(thin_wgrad_partial_kernel, dim3((unsigned)nblk), dim3(256), lds, (hipStream_t)stream,
                       (const bf16_t*)wide, c, c_stride, (const bf16_t*)thin, thin_stride, d, h, w, (float*)workspace);
    CTSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(thin_wgrad_reduce_kernel, dim3((unsigned)((c * 27 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)workspace, nblk, c, scale, head ? 1 : 0, dw);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
