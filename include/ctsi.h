/*
 * ctsi.h — C ABI of the MI355X (gfx950) CT slice-interpolation engine.
 *
 * This is the drop-in boundary underneath the reference's Python module surface
 * (models.* / inference.*).  The reference has no FFI of its own: every entry point
 * below replaces a PyTorch op family that the reference calls on its hot path, cited
 * as `reference file:line`.  The Python host (video-to-video-diffusion_amd/) binds
 * these with ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *  - extern "C", plain pointers / sizes / ints, no torch or C++ types.
 *  - every function returns 0 on success, <0 on error; ctsi_last_error() returns a
 *    thread-local message.  Nothing throws.
 *  - no entry point allocates device memory, synchronises the stream or the device:
 *    the caller passes all buffers (query sizes with the *_bytes/_floats helpers).
 *    All launches go to the `stream` argument (a hipStream_t passed as void*), so a
 *    caller may capture any sequence of calls into a hipGraph (ctsi_graph_*).
 *  - activations inside the engine are bf16, channels-last ("NDHWC": n, d, h, w, c with
 *    c fastest).  The API boundary tensors of the reference are fp32 NCDHW; the two
 *    conversion entry points sit at that boundary.  Accumulation, GroupNorm statistics,
 *    the time embedding and the DDIM/DDPM state are fp32.
 */
#ifndef CTSI_H
#define CTSI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTSI_OK 0
#define CTSI_ERR_INVALID (-1)
#define CTSI_ERR_UNSUPPORTED (-2)
#define CTSI_ERR_HIP (-3)

/* library / error handling ------------------------------------------------------------ */
int ctsi_version(void);
/* 1 for a build with the timing-only ablation switches compiled in (`make ablate`: libctsi_ablate.so, for tools/ only:
 * CTSI_DEBUG_FLAGS / CTSI_DEBUG_KSTEPS can make its kernels skip work); 0 for the release library, which ignores them. */
int ctsi_ablation_build(void);
const char* ctsi_last_error(void);
/* 1 when a HIP device is visible to this process, 0 otherwise (never raises). */
int ctsi_device_available(void);

/* boundary layout conversion ---------------------------------------------------------- *
 * fp32 NCDHW (reference API tensors, models/model.py:252-259) <-> bf16 NDHWC (engine).
 * `c_total`/`c_off` let the caller write a channel slice of a wider NDHWC tensor
 * (used for torch.cat([x, c], dim=1), models/unet3d.py:372).                            */
int ctsi_ncdhw_f32_to_ndhwc_bf16(const float* src, void* dst, int n, int c, int d, int h, int w,
                                 int c_total, int c_off, void* stream);
int ctsi_ndhwc_bf16_to_ncdhw_f32(const void* src, float* dst, int n, int c, int d, int h, int w,
                                 void* stream);
/* fp32 NDHWC <-> fp32 NCDHW (sampler state z lives as fp32 NDHWC inside the engine). */
int ctsi_ncdhw_f32_to_ndhwc_f32(const float* src, float* dst, int n, int c, int d, int h, int w,
                                void* stream);
int ctsi_ndhwc_f32_to_ncdhw_f32(const float* src, float* dst, int n, int c, int d, int h, int w,
                                void* stream);

/* convolution family ------------------------------------------------------------------ *
 * One gather-GEMM MFMA kernel serves nn.Conv3d k=3 p=1 (models/unet3d.py:56,96,257,331;
 * models/vae.py:27,45,134,188), k=1 (unet3d.py:102,152-153; vae.py:137,161),
 * k=(3,4,4) s=(1,2,2) p=1 (unet3d.py:204-207; vae.py:65-68) and
 * nn.ConvTranspose3d k=(3,4,4) s=(1,2,2) p=1 (unet3d.py:218-221; vae.py:86-89).
 *
 * A plan is a host-only opaque object (no device memory) describing one layer at one
 * input shape.  The input may be the channel concatenation of two NDHWC tensors
 * (c1 + c2 channels; c2 = 0 for a single source) so torch.cat along channels
 * (unet3d.py:372, 401) is never materialised.                                           */
typedef struct ctsi_conv_plan ctsi_conv_plan;

typedef struct ctsi_conv_desc {
    int transposed;      /* 0: Conv3d, 1: ConvTranspose3d                                   */
    int kd, kh, kw;      /* kernel size                                                     */
    int sh, sw;          /* stride in H, W (depth stride is always 1 on this path)         */
    int pd, ph, pw;      /* padding                                                         */
    int n, c1, c2;       /* batch, channels of source 1 and source 2 (c2 may be 0)        */
    int cout;
    int di, hi, wi;      /* input spatial size                                             */
    int halo_d;          /* 1: the input tensor carries one halo slice below and above its own
                            di-2 slices (depth-sharded volume); outputs cover the own slices only */
} ctsi_conv_desc;

/* epilogue description for ctsi_conv_fwd */
typedef struct ctsi_conv_out {
    void* y;             /* output tensor                                                   */
    int mode;            /* 0: bf16 NDHWC, channel stride = cout_stride, offset c_off      */
                         /* 1: fp32 with explicit element strides (sn, sc, sd, sh, sw)     */
    int cout_stride;     /* mode 0: channels per voxel of y (>= c_off + cout)              */
    int c_off;           /* mode 0: first channel written                                   */
    long long sn, sc, sd, sh, sw; /* mode 1 strides, in elements                           */
    int act;             /* 0: none, 1: tanh (models/vae.py:203), 2: ReLU -- planar (1,3,3)
                            halo-tile plans only (ctsi_conv_plan_form, bit 16), bf16 output,
                            no colsum; ctsi_conv_fwd refuses it on every other plan      */
    float* colsum;       /* optional: per-tile column sums for a following GroupNorm
                            ([2][ctsi_conv_plan_tiles()][cout_pad] floats), or NULL       */
    /* optional fused ResBlock tail (models/unet3d.py:130-133, `self.activation(h + self.residual_conv(x))` with h =
     * GroupNorm(conv2 output)): when gn_x != NULL the conv result r is not stored as is but
     *     y = silu?( gn(gn_x) * gamma + beta + r ),   gn statistics from gn_sums (as ctsi_gn_apply reads them),
     * so the residual tensor never goes to HBM.  mode 0 only, no colsum, no act; gn_x has y's shape and channel
     * stride and may alias y (in place).  The gather-GEMM kernel implements it (1x1x1 residual convs).           */
    const void* gn_x;        /* bf16 NDHWC, channel stride cout_stride, offset c_off                              */
    const double* gn_sums;   /* [n][groups][2] fp64 (sum, sumsq) of gn_x                                          */
    const float* gn_gamma;
    const float* gn_beta;
    int gn_groups;
    float gn_eps;
    long long gn_count;      /* elements per (sample, group) the statistics were taken over                       */
    int gn_silu;             /* 1: SiLU after the add                                                             */
    /* split-K plans (ctsi_conv_plan_workspace_bytes() > 0): device scratch of that size that belongs to THIS layer; zero it
     * once before the first launch (it holds the hand-off tickets), the kernel leaves it ready for the next launch      */
    void* workspace;
} ctsi_conv_out;

int ctsi_conv_plan_create(ctsi_conv_plan** plan, const ctsi_conv_desc* desc);
/* the weight tensor carries only `cin_w` (< c1+c2) input channels; the remaining activation
 * channels are layout padding (the 1-channel CT volume is stored with 8 channels).       */
int ctsi_conv_plan_set_weight_cin(ctsi_conv_plan* plan, int cin_w);
/* A 1x1x1 stride-1 layer that will run with the fused GroupNorm tail (ctsi_conv_out.gn_x: the ResBlock tails of
 * models/unet3d.py:102, 112-133) or as a plain bf16 conv + bias may take the streaming kernel (csrc/conv1_stream.hip: weights
 * resident in LDS, every voxel row read once straight into the MFMA layout).  Call it BEFORE ctsi_conv_plan_weight_bytes /
 * _pack_weights: the packed image differs.  on = 1 selects it where the layer qualifies (every source a multiple of 128
 * channels, K = 128 .. 512, 768 or 1024, cout in whole n-tiles) and is a no-op otherwise; ctsi_conv_plan_config reports
 * mode 10 when it is active.  Such a plan emits no column sums and no activation.                                  */
int ctsi_conv_plan_set_stream_tail(ctsi_conv_plan* plan, int on);
void ctsi_conv_plan_destroy(ctsi_conv_plan* plan);
/* output spatial size of the layer */
int ctsi_conv_plan_out_dims(const ctsi_conv_plan* plan, int* d_out, int* h_out, int* w_out);
/* bytes of the packed bf16 weight image this plan consumes */
size_t ctsi_conv_plan_weight_bytes(const ctsi_conv_plan* plan);
/* number of row tiles (all samples, all parity classes) and padded cout: sizes the colsum slab */
int ctsi_conv_plan_tiles(const ctsi_conv_plan* plan);
int ctsi_conv_plan_tiles_per_sample(const ctsi_conv_plan* plan);
int ctsi_conv_plan_cout_pad(const ctsi_conv_plan* plan);
/* bytes of ctsi_conv_out.workspace this plan needs (0 for most plans) */
size_t ctsi_conv_plan_workspace_bytes(const ctsi_conv_plan* plan);
/* algorithmic FLOPs (2*MAC, dense direct convolution) of one forward of this layer */
double ctsi_conv_plan_flops(const ctsi_conv_plan* plan);
/* which kernel variant the plan launches: MFMA tile (bm x bn) and staging mode
 * (0: general gather, 1: small-cin tap-packed K, 2: buffer-addressed whole-chunk gather)      */
int ctsi_conv_plan_config(const ctsi_conv_plan* plan, int* bm, int* bn, int* mode);
/* what ctsi_conv_plan_config cannot tell apart (host-only; tests and tools/conv_plan_sweep.py): out[0..2] the tile TD, TH, TW
 * (linear-row gather plans: TD = depth slices a tile can touch), out[3] the split-K factor (ksplit of a k32 plan, gsplit of a
 * gather plan, else 0), out[4] flag bits 1 linear, 2 fast, 4 head2, 8 ds, 16 planar (the (1,3,3) form of the k32 kernel: TD
 * counts depth slices, which are independent images; CTSI_CONV_PLANAR=0, read at plan creation, keeps such layers on the
 * gather kernel); out[5..7] are reserved (0).                                                                            */
int ctsi_conv_plan_form(const ctsi_conv_plan* plan, int out[8]);
/* which packed-weight image ctsi_conv_plan_pack_weights writes for this plan, as far as the descriptor's channel / kernel
 * fields, ctsi_conv_plan_cout_pad and the weight cin (ctsi_conv_plan_set_weight_cin) do not already say: bits 0-3 the
 * kernel family (CTSI_PACK_*); k32 plans add their form << 4 (0 Conv3d 3x3x3, 1 ConvTranspose3d, 2 strided Conv3d, 3 planar
 * Conv3d (1,3,3)), the
 * cout-permuted direct-store image << 6 and bn / 16 << 8; head plans set bit 4 when the image carries the conv3_head2
 * part; stream-tail plans add their n-tile count << 8.  Plans of equal descriptor channel / kernel fields, cout_pad, weight
 * cin and pack layout pack byte-identical images (a cache of packed images may key on exactly these).  0: null plan. */
#define CTSI_PACK_GATHER 1
#define CTSI_PACK_GATHER_SMALL 2
#define CTSI_PACK_HALO 3
#define CTSI_PACK_K32 4
#define CTSI_PACK_HEAD 5
#define CTSI_PACK_STREAM_TAIL 6
#define CTSI_PACK_STEM 7
int ctsi_conv_plan_pack_layout(const ctsi_conv_plan* plan);
/* re-layout reference weights (fp32, PyTorch layout: Conv3d (cout,cin,kd,kh,kw),
 * ConvTranspose3d (cin,cout,kd,kh,kw)) into the kernel's bf16 [class][cout_pad][K] image. */
int ctsi_conv_plan_pack_weights(const ctsi_conv_plan* plan, const float* w_f32, void* packed,
                                void* stream);
/* y = conv(cat(x1,x2)) + bias, optional activation, optional GroupNorm column sums. */
int ctsi_conv_fwd(const ctsi_conv_plan* plan, const void* x1, const void* x2, const void* packed_w,
                  const float* bias, const ctsi_conv_out* out, void* stream);

/* GroupNorm (+SiLU, +time bias, +residual) ----------------------------------------------- *
 * nn.GroupNorm(eps=1e-5, affine) + SiLU + the ResBlock tail of models/unet3d.py:70-74,
 * 116-133 and models/vae.py:31-35, 50-56, 72-76, 93-97.
 * Statistics are two-stage: per-tile column sums (from the conv epilogue, or from
 * ctsi_gn_colsum for tensors that no conv produced) -> ctsi_gn_finalize -> (sum, sumsq)
 * per (sample, group) in fp64 -> ctsi_gn_apply.                                          */
int ctsi_gn_colsum(const void* x_bf16, float* colsum, int n, int c, int d, int h, int w,
                   int* tiles_per_sample, void* stream);
int ctsi_gn_colsum_tiles(int d, int h, int w);
/* sums[n][g][2] (double) = sum over tiles/columns: WRITTEN, not accumulated (no zeroing needed), by one block per
 * (sample, group) with a fixed-order reduce -- bit-identical from run to run (no atomics).
 * nclass > 1: tiles of class k of sample i start at (k*n + i)*tiles_per_sample.          */
/* accumulate != 0: sums += instead of sums = (a tensor produced by several conv launches -- the interior / boundary split
 * of a depth-sharded conv -- is finalised slab by slab; still deterministic: the launches are ordered on the stream). */
int ctsi_gn_finalize(const float* colsum, double* sums, int n, int c, int c_pad, int groups,
                     int tiles_per_sample, int nclass, int accumulate, void* stream);
/* y = [silu]( gn(x)*gamma+beta ) [+ tbias[n][c]] [+ residual] ; [silu] again if silu_post */
/* tbias row used for sample i: (step_ptr ? *step_ptr : 0) * n + i  (row length tbias_stride).
 * d_stat: depth the statistics in `sums` were accumulated over (== d on one GPU; the whole volume's
 * depth when the tensor is one depth slab of a volume sharded across GPUs and `sums` was all-reduced). */
int ctsi_gn_apply(const void* x_bf16, void* y_bf16, const double* sums, const float* gamma,
                  const float* beta, int n, int c, int d, int h, int w, int d_stat, int groups, float eps,
                  int silu_pre, const float* tbias, int tbias_stride, const int* step_ptr,
                  const void* residual_bf16, int silu_post, void* stream);

/* TemporalAttention, fused middle: P[n][pos][co] = bias[co] + sum_ci W[co][ci] * (gamma rstd (S - D mean) + D beta)[n][pos][ci]
 * -- ctsi_attn_normsum and the folded (proj_out . V-projection) 1x1x1 conv (models/unet3d.py:152-153, 181-192) in one
 * launch.  depthsum / sums / gamma / beta as for ctsi_attn_normsum; w_bf16 = bf16 [c][c] row-major (cout, cin); bias fp32 [c];
 * out bf16 [n][h*w][c].  ctsi_attn_pv_supported(c, groups) != 0 where the kernel applies (c in {128,256,512,1024}, 8 | c / groups);
 * other shapes use ctsi_attn_normsum + a 1x1x1 ctsi_conv_fwd. */
int ctsi_attn_pv_supported(int c, int groups);
int ctsi_attn_pv(const float* depthsum, const double* sums, const float* gamma, const float* beta, const void* w_bf16,
                 const float* bias, void* out, int n, int c, int d, int h, int w, int groups, float eps, void* stream);

/* TemporalAttention (models/unet3d.py:136-194) --------------------------------------------- *
 * The reference's second einsum 'bhqk,bhvc->bhqc' contracts k and v independently, so the
 * module equals proj_out(rowsum(softmax) * sum_t V_t) + x with rowsum(softmax) == 1.
 * mode 0 (fast) uses that identity; mode 1 (exact) additionally evaluates
 * rowsum(softmax(q k^T * hd^-0.5)) in fp32 per (position, head, query) and multiplies by it. */
/* pass 1: GroupNorm column sums of x and depth sums S[n][h][w][c] = sum_d x (fp32) */
int ctsi_attn_depthsum(const void* x_bf16, float* depthsum, float* colsum, int n, int c, int d,
                       int h, int w, void* stream);
int ctsi_attn_depthsum_tiles(int c, int h, int w);
/* pass 2: xhat_sum = gamma*rstd*(S - D*mean) + D*beta as bf16 (n, 1, h, w, c) */
int ctsi_attn_normsum(const float* depthsum, const double* sums, const float* gamma,
                      const float* beta, void* out_bf16, int n, int c, int d, int h, int w,
                      int groups, float eps, void* stream);
/* pass 3 (after a 1x1x1 conv of xhat_sum with W_proj*W_v): y = x + p[n][h][w][c] broadcast over d.
 * rowsum (exact mode, fp32 [n][d][h][w][heads]) may be NULL (== 1).                       */
int ctsi_attn_broadcast_add(const void* x_bf16, const void* p_bf16, const float* rowsum, int heads,
                            void* y_bf16, int n, int c, int d, int h, int w, void* stream);
/* exact mode helper: rowsum[n][d][h][w][head] = sum_k softmax_k(q.k * hd^-0.5) from
 * qk = conv1x1(gn(x)) restricted to the q and k thirds (bf16 NDHWC with 2*c channels). */
int ctsi_attn_softmax_rowsum(const void* qk_bf16, float* rowsum, int n, int c, int d, int h, int w,
                             int heads, void* stream);

/* True depth attention (attention_mode='softmax'): A[q] = sum_k softmax_k(q.k / sqrt(hd)) v_k over the d depth positions of one
 * (sample, position, head).  qkv = bf16 NDHWC with 3*c channels [q | k | v], heads split inside each third (as the reference's
 * 'b (head c) t h w'); out = bf16 NDHWC with c channels.  bf16 MFMAs with fp32 accumulation, fp32 softmax; the probabilities
 * are rounded to bf16 for the P V product.  Head dimension c / heads in {8, 16, 32, 64, 128}; d * (2 * hd + 32) <= 65536 bytes
 * of LDS per item (backward: d * (4 * hd + 76)); anything else is CTSI_ERR_INVALID.  csrc/attention_core.hip. */
int ctsi_attn_core(const void* qkv_bf16, void* out_bf16, int n, int c, int d, int h, int w, int heads, void* stream);
/* its backward: dqkv (bf16, 3*c channels, every element written) from the saved qkv and dA = dLoss/dA (bf16, c channels);
 * S and P are recomputed.  dV = P^T dA, dP = dA V^T, dS = P o (dP - rowsum(P o dP)), dQ = dS K / sqrt(hd), dK = dS^T Q / sqrt(hd). */
int ctsi_attn_core_bwd(const void* qkv_bf16, const void* da_bf16, void* dqkv_bf16, int n, int c, int d, int h, int w, int heads,
                       void* stream);

/* In-plane (spatial) attention (SpatialAttention): A[i] = sum_j softmax_j(q_i.k_j / sqrt(hd)) v_j over the
 * N = h * w positions of one (sample, depth slice, head), flash-attention style -- query blocks per workgroup, K / V tiles of 64
 * keys streamed through LDS, online softmax; any N >= 1, no LDS limit on N.  qkv / out as for ctsi_attn_core; lse = fp32
 * [n][d][heads][h*w], ln sum_j exp(s_ij) of the scaled scores, may be NULL (inference).  Head dimension c / heads in
 * {8, 16, 32, 64, 128}; anything else is CTSI_ERR_INVALID.  csrc/attention_plane.hip. */
int ctsi_attn_plane(const void* qkv_bf16, void* out_bf16, float* lse, int n, int c, int d, int h, int w, int heads, void* stream);
/* its backward: dqkv (bf16, 3*c channels, every element written) from the saved qkv, the forward's out (A, as stored) and lse,
 * and dA (bf16, c channels).  Two grids, no atomics: a query-block pass writes dQ, a key-block pass dK and dV; P is recomputed
 * from lse, delta = rowsum(dA o A).  Bit-identical run to run. */
int ctsi_attn_plane_bwd(const void* qkv_bf16, const void* out_bf16, const void* da_bf16, const float* lse,
                        void* dqkv_bf16, int n, int c, int d, int h, int w, int heads, void* stream);

/* time embedding (models/unet3d.py:18-48 and the per-block Linear of :88-91, 123-125) ------- *
 * temb = Linear2(SiLU(Linear1(sincos(t))));  tbias[r][o] = W_all[o] . SiLU(temb[r]) + b_all[o]
 * for the concatenation of every ResBlock's time_mlp.1 (`total_out` rows of W_all).
 * `t_rows` holds `rows` timestep values on the device (all steps x batch of a sampling loop are
 * embedded in one call, the schedule being known up front); scratch = rows*(dim+2*time_dim) floats. */
int ctsi_time_embed_fwd(const int* t_rows, int rows, int dim, int time_dim, const float* w1,
                        const float* b1, const float* w2, const float* b2, const float* w_all,
                        const float* b_all, int total_out, float* scratch, float* tbias_out,
                        void* stream);

/* ctsi_time_embed_fwd with fractional timesteps: `t_rows` holds `rows` fp32 values (the EDM sampler's t(sigma),
 * UNet3D.forward with a non-integer t).  An integer-valued row gives the bit-identical embedding of the int entry. */
int ctsi_time_embed_fwd_tf(const float* t_rows, int rows, int dim, int time_dim, const float* w1,
                           const float* b1, const float* w2, const float* b2, const float* w_all,
                           const float* b_all, int total_out, float* scratch, float* tbias_out,
                           void* stream);

/* trilinear depth upsample (F.interpolate(..., 'trilinear', align_corners=False) with h, w
 * unchanged: models/model.py:284-289, 191-196).  fp32 NCDHW in -> bf16 NDHWC channel slice
 * [c_off, c_off+c) of a c_total-channel tensor, plus an optional fp32 NCDHW copy.            */
int ctsi_trilinear_depth_fwd(const float* src_f32_ncdhw, void* dst_bf16_ndhwc, int n, int c,
                             int d_in, int d_out, int h, int w, int c_total, int c_off,
                             float* dst_f32_ncdhw, void* stream);

/* sampler updates --------------------------------------------------------------------------- *
 * DDIM (inference/sampler.py:294-334) and DDPM (models/diffusion.py:270-338) elementwise
 * updates with the reference's epsilons, clamps and nan_to_num guards folded in.
 * coef is a device table of 8 floats per step (see video-to-video-diffusion_amd/sampler.py);
 * the row used is coef[*step_ptr] (row 0 when step_ptr is NULL).  z (fp32 NDHWC) is updated in
 * place and a bf16 copy is written into channels [c_off, c_off+c) of the U-Net input tensor.
 * noise (fp32 NCDHW, the layout torch.randn_like(z) has) may be NULL.
 * ctsi_step_advance increments the device-side step counter (last node of a step graph).   */
/* nonfinite (DDIM only, may be NULL): int32 table [steps][6], row *step_ptr += {noise_pred NaN, Inf, z_0_pred NaN, Inf,
 * z-after-update NaN, Inf} -- what the reference's per-step guards report through logger.error (inference/sampler.py:
 * 288-292, 307-311, 331-334); the host reads it once after the loop (no sync inside the captured step).             */
int ctsi_ddim_step(float* z, const float* eps, const float* noise_ncdhw, void* zin_bf16,
                   int c_total, int c_off, const float* coef, const int* step_ptr, int n, int c,
                   int d, int h, int w, int* nonfinite, void* stream);
int ctsi_ddpm_step(float* z, const float* eps, const float* noise_ncdhw, void* zin_bf16,
                   int c_total, int c_off, const float* coef, const int* step_ptr, int n, int c,
                   int d, int h, int w, void* stream);
/* DDPM posterior with PER-SAMPLE timesteps on fp32 NCDHW tensors (replaces the arithmetic of GaussianDiffusion.
 * _predict_z_0_from_noise, p_mean_variance and p_sample: models/diffusion.py:249-268, 270-308, 310-338).  Sample b uses
 * coef[b*8 ..] = {sqrt(1-abar_t), sqrt(abar_t), posterior_mean_coef1, posterior_mean_coef2, [t != 0] exp(0.5 logvar)}.
 * z0_out (may be NULL) <- (z - c0 eps) / c1, clamped to [-1, 1] when clip != 0; out (may be NULL) <- c2 z0 + c3 z
 * (+ c4 noise when noise != NULL).  per_sample = C*D*H*W.                                                               */
int ctsi_ddpm_posterior(const float* z, const float* eps, const float* noise, float* z0_out, float* out,
                        const float* coef, int n, long long per_sample, int clip, void* stream);
int ctsi_step_advance(int* step_ptr, void* stream);
/* x <- nan_to_num(x, nan=0, posinf=1, neginf=-1) on a flat fp32 buffer (model.py:262-341) */
int ctsi_nan_to_num_f32(float* x, long long count, void* stream);
/* counts[0] += #NaN, counts[1] += #Inf of x; sanitize != 0 also applies nan_to_num (sampler.py:268-275 checkpoints) */
int ctsi_count_nonfinite_f32(float* x, long long count, int sanitize, int* counts, void* stream);

/* ---- training path (models/diffusion.py:81-247, models/model.py:158-228; backward = what autograd derives) ---- */
/* Weight gradient of Conv3d / ConvTranspose3d:  dw[cr*stride_r + cg*stride_g + t*stride_t] =
 *   scale * sum_v R[v][cr] * G[map(v,t)][cg],  map(v,t) = (n, d-pd+kd, h*sh-ph+kh, w*sw-pw+kw), zero outside G.
 * Conv3d: R = grad of the output, G = layer input (weight (cout,cin,kd,kh,kw): stride_r = cin*T, stride_g = T,
 * stride_t = 1).  ConvTranspose3d: R = layer input, G = grad of the output (weight (cin,cout,kd,kh,kw)).
 * bf16 NDHWC tensors, channel counts multiples of 8; a concatenated input is two calls with dw offset by the
 * first source's channels.  Deterministic (split-K partials in `workspace`, summed in a fixed order). */
typedef struct ctsi_wgrad_desc {
    int kd, kh, kw;
    int sh, sw;
    int pd, ph, pw;
    int n;
    int dr, hr, wr;        /* spatial size of R */
    int dg, hg, wg;        /* spatial size of G */
    int cr, cr_stride;     /* channels of R used / channels per voxel of R */
    int cg, cg_stride;
} ctsi_wgrad_desc;
size_t ctsi_wgrad_workspace_bytes(const ctsi_wgrad_desc* desc);
double ctsi_wgrad_flops(const ctsi_wgrad_desc* desc);
/* workspace_bytes: size of `workspace`; the call fails (nothing is launched) when it is smaller than what
 * ctsi_wgrad_workspace_bytes(desc) returns at launch time */
int ctsi_wgrad(const ctsi_wgrad_desc* desc, const void* r, const void* g, void* workspace, size_t workspace_bytes, float* dw,
               long long stride_r, long long stride_g, long long stride_t, float scale, void* stream);

/* out (ci_cnt, cout, T) with out[ci'][co][T-1-t] = w[co][ci_off+ci'][t]: the weight of the stride-1 'same' Conv3d
 * that computes the data gradient of a stride-1 'same' Conv3d with weight w (cout, cin, T) for the input-channel
 * slice [ci_off, ci_off+ci_cnt).  (Strided Conv3d <-> ConvTranspose3d data gradients use the weights as they are.) */
int ctsi_weight_dgrad_layout(const float* w, float* out, int cout, int cin, int taps, int ci_off, int ci_cnt,
                             void* stream);

/* Weight and bias gradients of MANY small pointwise layers (the proj_out / V layers of the TemporalAttention blocks, whose
 * operands are depth-summed tensors of a few hundred rows) in ONE launch.  entries: device array of
 *   { const bf16* x [rows][cin]; const bf16* dy [rows][cout]; float* dw [cout][dw_stride]; float* db or NULL;
 *     int rows, cin, cout, dw_stride; float b_scale; int pad }                                     (56 bytes each)
 * blocks: device array of { int entry, cout_tile, cin_tile, pad } -- one row per 64 x 64 tile of an entry's dW (16 bytes each).
 * dw[co][ci] = sum_r dy[r][co] * x[r][ci] (WRITTEN, not accumulated), db[co] = b_scale * sum_r dy[r][co]; deterministic. */
int ctsi_linear_wgrad_multi(const void* entries, const void* blocks, int n_blocks, void* stream);

/* Backward of ctsi_gn_apply (GroupNorm [+SiLU] [+time bias] [+residual] [+SiLU]).  x: the tensor that was normalised,
 * dy: gradient of the output (depth-broadcast (n,1,h,w,c) tensor when dy_bcast_d), sums: the forward's fp64 statistics,
 * residual: the forward's residual input (needed when silu_post).  Writes g_buf = gradient of the GroupNorm output
 * (== gradient of the residual when !silu_pre), dx (+ add when given), dgamma/dbeta (c floats) and, when dtbias is
 * given, dtbias[n][c] (row stride dtbias_stride) = per-sample channel sums of the gradient after the outer SiLU, and,
 * when dxsum is given, dxsum[c] = sum over samples and voxels of dx (before `add`) = the bias gradient of the
 * convolution that produced x, evaluated in fp32 from the statistics instead of re-reading dx.
 * g_buf may be NULL when there is neither a residual nor an outer SiLU (nothing but dx needs that gradient: the second pass
 * re-derives it from dy; same dx bit for bit, one tensor write less).
 * workspace: ctsi_gn_bwd_workspace_floats() floats (the statistics tile shrinks from 512 rows for small tensors, so that
 * function -- not ctsi_gn_bwd_tiles, the tile count at 512 rows -- sizes it). */
int ctsi_gn_bwd_tiles(int d, int h, int w);
size_t ctsi_gn_bwd_workspace_floats(int n, int c, int d, int h, int w, int groups);
int ctsi_gn_bwd(const void* x, const void* dy, int dy_bcast_d, const double* sums, const float* gamma,
                const float* beta, int n, int c, int d, int h, int w, int groups, float eps, int silu_pre,
                const void* residual, int silu_post, const void* add, void* g_buf, void* dx, float* workspace,
                float* dgamma, float* dbeta, float* dtbias, long long dtbias_stride, float* dxsum, void* stream);

/* out[c] = scale * sum over rows of x[row][c]  (bf16 rows of c_stride channels; conv bias gradients) */
size_t ctsi_channel_sum_workspace_floats(long long rows, int c);
int ctsi_channel_sum(const void* x, long long rows, int c, int c_stride, float* workspace, float* out, float scale,
                     void* stream);
int ctsi_add_bf16(void* a, const void* b, long long count, void* stream);        /* a += b */
int ctsi_f32_to_bf16(const float* src, void* dst, long long count, void* stream);

/* ---- VAE training (SliceInterpolationVAE.forward's backward) ---- */
/* Output gradient of the decoder's tanh head / encoder-output gradient at the latent seam.  g (and y): fp32 NCDHW
 * (n, c, d, h, w); dst: bf16 NDHWC with c_stride channels per voxel (c_stride >= c, a multiple of 8, 16-byte aligned).
 * mode 0: dst = bf16(scale * g * (1 - y^2)), channels c .. c_stride-1 zero.  mode 1: dst += scale * g (y unused, padding
 * channels untouched). */
int ctsi_vae_head_grad(const float* g, const float* y, int n, int c, int d, int h, int w, float scale, int mode, void* dst,
                       int c_stride, void* stream);
/* Weight gradient of a 3x3x3 stride-1 padding-1 Conv3d with ONE input channel (head = 0: wide = output gradient (c channels),
 * thin = layer input) or ONE output channel (head = 1: wide = layer input, thin = output gradient).  bf16 NDHWC tensors of
 * shape (n, d, h, w); the thin tensor's channel 0 is read at stride thin_stride.  dw[c * 27 + t] = scale * (the weight
 * gradient), WRITTEN; deterministic (per-block partials in `workspace`, summed in a fixed order).  Supported when
 * ctsi_thin_wgrad_supported(c, w, kd, kh, kw); the call fails without launching otherwise. */
size_t ctsi_thin_wgrad_workspace_bytes(int n, int c, int d, int h, int w);
int ctsi_thin_wgrad_supported(int c, int w, int kd, int kh, int kw);
int ctsi_thin_wgrad(const void* wide, int c, int c_stride, const void* thin, int thin_stride, int head, int n, int d, int h,
                    int w, int kd, int kh, int kw, void* workspace, size_t workspace_bytes, float* dw, float scale,
                    void* stream);

/* q_sample (models/diffusion.py:81-106): z_t = sqrt_alphas_cumprod[t_b]*z0 + sqrt_one_minus_alphas_cumprod[t_b]*noise,
 * fp32 NCDHW in, bf16 NDHWC channel slice out (the U-Net input tensor [z_t | cond]). */
int ctsi_q_sample(const float* z0, const float* noise, const float* sqrt_ac, const float* sqrt_1mac, const int* t,
                  void* dst, int n, int c, int d, int h, int w, int c_total, int c_off, void* stream);
/* Min-SNR weighted MSE (models/diffusion.py:147-203): loss_out[0] = sum_b norm[b] * sum mask*(pred-noise)^2,
 * loss_out[1+b] = per-sample sums.  pred fp32 NDHWC, noise fp32 NCDHW, mask fp32 (n,c,d) or NULL; the caller folds the
 * SNR weight and the normalisation of the reference's three cases into norm[b].  _bwd writes
 * d_pred = 2*norm[b]*mask*(pred-noise)*gscale[0] as bf16 NDHWC with c_stride channels per voxel (extra ones zero). */
size_t ctsi_mse_loss_workspace_doubles(int n);
int ctsi_mse_loss_fwd(const float* pred, const float* noise, const float* mask, const float* norm, int n, int c,
                      int d, int h, int w, double* workspace, float* loss_out, void* stream);
int ctsi_mse_loss_bwd(const float* pred, const float* noise, const float* mask, const float* norm,
                      const float* gscale, int n, int c, int d, int h, int w, void* dpred, int c_stride, void* stream);

/* time embedding for training: as ctsi_time_embed_fwd, but scratch = [sincos | first Linear PRE-activation | temb] */
int ctsi_time_embed_train_fwd(const int* t_rows, int rows, int dim, int time_dim, const float* w1, const float* b1,
                              const float* w2, const float* b2, const float* w_all, const float* b_all,
                              int total_out, float* scratch, float* tbias_out, void* stream);
/* backward of y = act(x) W^T + b (act = SiLU when silu_in, x then is the pre-activation); rows <= 64; any of
 * dw/db/dx may be NULL */
int ctsi_linear_bwd(const float* x, const float* w, const float* dy, int rows, int in_dim, int out_dim, int silu_in,
                    float* dw, float* db, float* dx, void* stream);

/* sliding-window stitching (inference/sampler.py:63-172, 338-453): Gaussian-weighted accumulation of one decoded
 * patch (fp32 NCDHW, nc = batch*channels planes) into the full-volume accumulator and weight map, and the final
 * acc / (wsum + 1e-8).  wd/wh/ww are the 1-D windows exp(-(x-(n-1)/2)^2 / (2 (n/6)^2)) on the device.          */
int ctsi_blend_accumulate(float* acc, float* wsum, const float* patch, const float* wd, const float* wh,
                          const float* ww, int nc, int pd, int ph, int pw, int d_full, int h_full, int w_full,
                          int d0, int h0, int w0, void* stream);
int ctsi_blend_normalize(float* acc, const float* wsum, long long count, void* stream);

/* validation metrics (utils/metrics.py:14-193) on device: for fp32 (n,c,d,h,w) volumes a, b writes, per depth
 * slice, out[slice][4] = (mean squared difference, mean SSIM, NaN count of a, NaN count of b) over (n,c,h,w).
 * SSIM = the reference's avg_pool2d box-window form (window odd <= 15, zeros counted at the borders, variances
 * clamped at 0, map clamped to [0,1]); PSNR = 20 log10(max_val / sqrt(max(mse, 1e-8))) is left to the caller. */
size_t ctsi_slice_metrics_workspace_doubles(int n, int c, int d, int h, int w);
int ctsi_slice_metrics(const float* a, const float* b, int n, int c, int d, int h, int w, int window, float max_val,
                       double* workspace, double* out, void* stream);

/* multi-planar and 3-D volume metrics (csrc/volume_metrics.hip): the SSIM of ctsi_slice_metrics under a separable window of
 * radii (rd, rh, rw) <= 7 -- axial (0,R,R), coronal (R,0,R), sagittal (R,R,0), volumetric (Rd,R,R) -- over fp32 (n,c,d,h,w)
 * volumes read in place, zero padding counted in the window.  gd/gh/gw: 2r+1 normalised fp32 weights each on the device, or
 * all three NULL for the box window.  axis 0/1/2 = d/h/w names the tables' index: out[len(axis)][4] = (SUM of squared
 * differences, SUM of SSIM, NaN count of a, NaN count of b) over every voxel with that index; the caller divides by the
 * slice's voxel count.  workspace: ctsi_volume_metrics_workspace_doubles() doubles (enough for any axis; 0 for an invalid shape
 * or radius).  Two launches, no atomics: the same bits on every run. */
size_t ctsi_volume_metrics_workspace_doubles(int n, int c, int d, int h, int w, int rd, int rh, int rw);
int ctsi_volume_metrics(const float* a, const float* b, int n, int c, int d, int h, int w, int rd, int rh, int rw,
                        const float* gd, const float* gh, const float* gw, int axis, float max_val, double* workspace,
                        double* out, void* stream);

/* hipMemsetAsync on the engine stream (zeroing GroupNorm accumulators / padded channels);
 * capturable as a memset node.                                                              */
int ctsi_memset_async(void* ptr, int value, size_t bytes, void* stream);

/* ---- optimizer step on the device (training/train.py:172-212 Adam / AdamW over parameter groups; trainer.py:237-247) ----
 * ctsi_adamw_multi: ONE launch over device tables built by the host (optim.py):
 *   tensors[i] = { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; long long numel; int group; int pad }
 *   groups[j]  = { float lr, beta1, beta2, eps, weight_decay, step_size (= lr / (1 - beta1^t)), bc2_sqrt (= sqrt(1 - beta2^t)),
 *                  decay (= 1 - lr weight_decay), one_m_b1, one_m_b2, grad_scale; int decoupled (1 AdamW, 0 Adam + L2),
 *                  maximize, pad[3] }   (64 bytes; the derived constants are rounded from the host's doubles, as torch's are)
 *   chunks[b]  = { int tensor; int first_element / 4 }: block b updates ctsi_adamw_chunk_elems() elements of that tensor.
 * fp32 throughout, torch.optim.AdamW's single-tensor arithmetic operation by operation.
 * ctsi_copy_scale_multi: dst[i] = scale * src[i] over a table segs[k] = { const float* src; float* dst; long long n; float
 * scale; int pad }, pieces[b] = { int seg; int first_element / 4096 } -- every small fp32 operand of a program refreshed from
 * the parameters in one launch. */
int ctsi_adamw_chunk_elems(void);
int ctsi_adamw_multi(const void* tensors, const void* groups, const void* chunks, int nchunks, void* stream);
int ctsi_copy_scale_multi(const void* segs, const void* pieces, int npieces, void* stream);

/* ---- the rest of the device-side optimizer step: EMA of the weights and global-norm clipping ----
 * All of these take a tensor table of their own plus a chunk table laid out as ctsi_adamw_multi's ({ int tensor; int
 * first_element / 4 }, ctsi_adamw_chunk_elems() elements per block); null tables / negative counts return CTSI_ERR_INVALID
 * before any launch, nchunks == 0 returns CTSI_OK.  16-byte accesses where every pointer of a row is 16-byte aligned.
 * ctsi_ema_multi: ema = ema + w (p - ema) over tensors[i] = { float* ema; const float* p; long long numel; int group; int pad },
 *   w = weights[group] = (float)(1 - decay), a device row (torch's lerp_ for w < 0.5).
 * ctsi_swap_multi: exchanges the values of a and b over pairs[i] = { float* a; float* b; long long numel; long long pad }.
 * ctsi_grad_norm_multi: partials[b] = sum over chunk b of (scale * g)^2 in fp64, tensors[i] = { float* grad; long long numel;
 *   float scale; int pad }.  ctsi_grad_norm_finalize: ONE block adds the partials in a fixed order and writes out = { float
 *   total_norm; float clip_coef = min(1, max_norm / (total_norm + 1e-6)) } (torch.nn.utils.clip_grad_norm_'s fp32 arithmetic;
 *   a NaN norm gives a NaN coefficient).  No atomics: the same bits on every run.
 * ctsi_grad_scale_multi: grad *= *dev_scale in place over the table of the norm pass (nothing is written when it is 1).
 * ctsi_adamw_ema_multi: ctsi_adamw_multi's update over the wider row tensors[i] = { float* param; const float* grad; float*
 *   exp_avg; float* exp_avg_sq; float* ema (NULL: none); long long numel; int group; int ema_group; long long pad } (64 bytes);
 *   dev_grad_scale (nullable) is ONE device float multiplied into every group's grad_scale (the clip_coef above: out + 1),
 *   ema_weights (nullable: no shadow is touched) holds (float)(1 - decay) per ema group; the shadow is updated from the NEW
 *   parameter.  With both NULL, param / exp_avg / exp_avg_sq come out as ctsi_adamw_multi's, bit for bit. */
int ctsi_ema_multi(const void* tensors, const void* weights, const void* chunks, int nchunks, void* stream);
int ctsi_swap_multi(const void* pairs, const void* chunks, int nchunks, void* stream);
int ctsi_grad_norm_multi(const void* tensors, const void* chunks, int nchunks, double* partials, void* stream);
int ctsi_grad_norm_finalize(const double* partials, int nchunks, float max_norm, float* out, void* stream);
int ctsi_grad_scale_multi(const void* tensors, const void* chunks, int nchunks, const float* dev_scale, void* stream);
int ctsi_adamw_ema_multi(const void* tensors, const void* groups, const void* chunks, int nchunks,
                         const float* dev_grad_scale, const float* ema_weights, void* stream);

/* ---- differentiable MS-SSIM loss on the device (models/losses.py:149-276; csrc/msssim.hip) ----
 * pred, target: fp32, `planes` = B*C*D contiguous h x w images in [-1, 1] (the NCDHW tensor as it lies); five levels, the
 * zero-padded Gaussian window (sigma 1.5, `window` odd, 1..15), 2 x 2 average pools between levels (floor),
 * loss = 1 - prod_i mean_i ^ w_i.  min(h, w) >= 16, planes <= 65535.  fp32 arithmetic, fp64 sums in a fixed order, no
 * atomics: loss and gradient are the same bits on every run.  No allocation, no synchronisation, capture-safe; bad arguments
 * return CTSI_ERR_INVALID before any launch (ctsi_msssim_workspace_bytes returns 0 and sets ctsi_last_error).
 * ctsi_msssim_workspace_bytes: with n_i = planes (h >> i)(w >> i) and t_i = planes ceil((h >> i) / 32) ceil((w >> i) / 32):
 *     8 sum_{i=0..4} t_i  (fp64 partials)  +  64  (factor table)  +  8 sum_{i=1..4} n_i  (pooled images)
 *     + (want_grad ? 12 sum_{i=0..4} n_i  (coefficient maps)  +  4 sum_{i=1..4} n_i  (level gradients) : 0).
 * ctsi_msssim_fwd: 5 level launches + 1 finalize; out[0] = loss, out[1..5] = the five level means (device floats).  With
 *   want_grad = 0 the coefficient maps are neither part of the workspace nor written.
 * ctsi_msssim_bwd: 5 level launches, coarse to fine, on the workspace of a want_grad = 1 forward of the same operands;
 *   grad_pred = *grad_loss * d loss / d pred (grad_loss is a DEVICE float), fp32 in pred's layout.  target gets no gradient. */
size_t ctsi_msssim_workspace_bytes(int planes, int h, int w, int window, int want_grad);
int ctsi_msssim_fwd(const float* pred, const float* target, int planes, int h, int w, int window, int want_grad,
                    void* workspace, float* out, void* stream);
int ctsi_msssim_bwd(const float* pred, const float* target, int planes, int h, int w, int window, void* workspace,
                    const float* grad_loss, float* grad_pred, void* stream);

/* Device-side errors recorded since the last call with reset != 0 (0 on a healthy run): today the only source is a split-K
 * conv block whose bounded wait for its partner's partial sums expired (csrc/conv3_halo_k32.hip): that tile's output is
 * then invalid, and this sticky count is what tells the host so.  *detail (may be NULL) = that tile's index.
 * SYNCHRONOUS 8-byte device-to-host read: the samplers call it once per sample(), where they read the non-finite table. */
int ctsi_device_error_status(unsigned int* count, unsigned int* detail, int reset);

/* fp32 inference mode (csrc/conv_f32.hip, csrc/f32_ops.hip) ---------------------------------------------------------------- *
 * The reference's generate() runs the VAE and the sampler in fp32 (models/model.py:254-259).  In this mode activations are
 * fp32 NDHWC and every convolution multiplies fp32 operands on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered
 * fmaf chain) with fp32 accumulation.  GroupNorm statistics still go through ctsi_gn_finalize (fp64); the time embedding,
 * the trilinear depth upsample and the fp32 layout converters above are shared with the bf16 path.  Depth sharding
 * (halo_d = 1) is not supported.
 *
 * Convolution: the ctsi_conv_desc of the bf16 path, any channel counts (c1 + c2 >= 1, cout >= 1), geometries 3x3x3 p1,
 * 1x1x1 p0, Conv3d (3,4,4) s(1,2,2) p1 and ConvTranspose3d (3,4,4) s(1,2,2) p1 (evaluated as 4 output parity classes of
 * 3x2x2 taps).  No plan object: the descriptor is the plan.
 *   _supported   1 when the fp32 kernel covers the descriptor, 0 otherwise (the reason in ctsi_last_error)
 *   _weight_bytes  bytes of the packed fp32 image (0 when unsupported)
 *   _geometry    output dims, row tiles per (sample, class), classes (4 for the transposed form), padded cout: a colsum
 *                slab is [2][nclass * n * tiles_per_sample][cout_pad] floats, as ctsi_gn_finalize reads it (nclass > 1:
 *                tiles of class k of sample i start at (k * n + i) * tiles_per_sample)
 *   _pack_weights  reference weights (fp32, PyTorch layout) -> the kernel's fp32 image [class][tap * cpad + ci][cout_pad]
 *   _fwd         y = act(conv(cat(x1, x2)) + bias + residual); `out` as for ctsi_conv_fwd with mode 0 = fp32 NDHWC (channel
 *                stride cout_stride, offset c_off) and mode 1 = fp32 with element strides; act 0 / 1 (tanh); colsum
 *                optional; gn_x must be NULL and workspace is ignored.  `residual` (may be NULL) is fp32 and addressed exactly
 *                like y.  Fixed summation order, no atomics: a relaunch is bit-identical.                                   */
int ctsi_conv_f32_supported(const ctsi_conv_desc* desc);
size_t ctsi_conv_f32_weight_bytes(const ctsi_conv_desc* desc);
double ctsi_conv_f32_flops(const ctsi_conv_desc* desc);
int ctsi_conv_f32_geometry(const ctsi_conv_desc* desc, int* d_out, int* h_out, int* w_out, int* tiles_per_sample,
                           int* nclass, int* cout_pad);
int ctsi_conv_f32_pack_weights(const ctsi_conv_desc* desc, const float* w_f32, void* packed, void* stream);
int ctsi_conv_f32_fwd(const ctsi_conv_desc* desc, const float* x1, const float* x2, const void* packed_w, const float* bias,
                      const float* residual, const ctsi_conv_out* out, void* stream);
/* bf16x3 inference mode (csrc/conv_bf16x3.hip) ----------------------------------------------------------------------------- *
 * The convolution of the fp32 mode on the bf16 MFMA (v_mfma_f32_32x32x16_bf16): tensors stay fp32, and inside the kernel each
 * fp32 operand v is split as hi = bf16(v) (round to nearest even), lo = bf16(v - float(hi)); the kernel sums
 * xh wh + xh wl + xl wh in fp32 (each product exact).  Everything else of the fp32 mode (GroupNorm, attention, sampler
 * updates, layout converters) is reused unchanged.  Same descriptor, same output struct, same geometries, same rejections,
 * same colsum slab layout and same epilogue as ctsi_conv_f32_*; differences:
 *   _weight_bytes  bytes of the packed image: a hi and a lo bf16 image [class][tap * cpad / 32 + ci / 32][cout_pad][32], cpad =
 *                c1 + c2 rounded up to 32 (zero rows / columns cover the padding)
 *   _flops       the useful 2 M N K, not the three products
 *   _fwd         `packed_w` must be 16-byte aligned.  Fixed summation order, no atomics: a relaunch is bit-identical and a
 *                sample's result does not depend on the batch around it.                                                    */
int ctsi_conv_bf16x3_supported(const ctsi_conv_desc* desc);
size_t ctsi_conv_bf16x3_weight_bytes(const ctsi_conv_desc* desc);
double ctsi_conv_bf16x3_flops(const ctsi_conv_desc* desc);
int ctsi_conv_bf16x3_geometry(const ctsi_conv_desc* desc, int* d_out, int* h_out, int* w_out, int* tiles_per_sample,
                              int* nclass, int* cout_pad);
int ctsi_conv_bf16x3_pack_weights(const ctsi_conv_desc* desc, const float* w_f32, void* packed, void* stream);
int ctsi_conv_bf16x3_fwd(const ctsi_conv_desc* desc, const float* x1, const float* x2, const void* packed_w, const float* bias,
                         const float* residual, const ctsi_conv_out* out, void* stream);
/* GroupNorm on fp32 NDHWC: column sums in 512-voxel tiles (ctsi_gn_colsum_f32_tiles per sample) and the apply pass with every
 * option of ctsi_gn_apply (SiLU before, time bias row (step_ptr ? *step_ptr : 0) * n + i, fp32 residual, SiLU after). */
int ctsi_gn_colsum_f32_tiles(int d, int h, int w);
int ctsi_gn_colsum_f32(const float* x, float* colsum, int n, int c, int d, int h, int w, int* tiles_per_sample, void* stream);
int ctsi_gn_apply_f32(const float* x, float* y, const double* sums, const float* gamma, const float* beta, int n, int c,
                      int d, int h, int w, int d_stat, int groups, float eps, int silu_pre, const float* tbias,
                      int tbias_stride, const int* step_ptr, const float* residual, int silu_post, void* stream);
/* The ResBlock's middle pass with the ADM-style options (norm_act.hip, f32_ops.hip, norm_bwd.hip).  ctsi_gn_apply_mod has the argument
 * list of ctsi_gn_apply plus: film (0: y = silu(gn(x)) + e, the time row holds c values; 1: y = silu(gn(x) * (1 + s) + b), the
 * time row holds (s | b), 2c values, scale first), p_thr16 (dropout threshold in 1/65536 units, 0 = none: an element is kept iff
 * its 16-bit Philox lane >= p_thr16), inv_keep (65536 / (65536 - p_thr16)), seed (DEVICE pointer to one 64-bit seed; may be
 * NULL when p_thr16 == 0) and layer_id.  It serves that pass only: silu_pre != 0, tbias != NULL, residual == NULL,
 * silu_post == 0 (anything else is an argument error).  tbias points at the block's first column of the time rows.
 * Keep rule: one Philox4x32-10 call per 16-byte chunk g = ((sample * vox + voxel) * c + ch) / 8 of the logical NDHWC tensor,
 * counter (lo32(g), hi32(g), layer_id, 0), key (seed_lo, seed_hi); channel j of the chunk takes
 * (out[j >> 1] >> (16 * (j & 1))) & 0xffff.                                                                            */
int ctsi_gn_apply_mod(const void* x_bf16, void* y_bf16, const double* sums, const float* gamma, const float* beta, int n,
                      int c, int d, int h, int w, int d_stat, int groups, float eps, int silu_pre, const float* tbias,
                      int tbias_stride, const int* step_ptr, const void* residual_bf16, int silu_post, int film,
                      int p_thr16, float inv_keep, const void* seed, int layer_id, void* stream);
/* fp32-activation twin for the fp32 inference mode (no dropout: inference never drops). */
int ctsi_gn_apply_mod_f32(const float* x, float* y, const double* sums, const float* gamma, const float* beta, int n, int c,
                          int d, int h, int w, int d_stat, int groups, float eps, int silu_pre, const float* tbias,
                          int tbias_stride, const int* step_ptr, const float* residual, int silu_post, int film,
                          void* stream);
/* Backward of ctsi_gn_apply_mod.  tbias: the forward's time rows (row i for sample i, no step_ptr: training), read for s in
 * scale-shift mode.  Writes dx, dgamma / dbeta (c floats), dxsum (optional: sum over samples and voxels of dx = the bias
 * gradient of the conv that produced x) and, when dtbias is given, row i of the time-row gradient: (d_s | d_b), 2c floats,
 * in scale-shift mode, d_e (c floats) in additive mode.  Deterministic (fixed-order reductions, no float atomics).
 * workspace: ctsi_gn_bwd_mod_workspace_floats() floats.                                                                */
size_t ctsi_gn_bwd_mod_workspace_floats(int n, int c, int d, int h, int w, int groups);
int ctsi_gn_bwd_mod(const void* x, const void* dy, const double* sums, const float* gamma, const float* beta, int n, int c,
                    int d, int h, int w, int groups, float eps, const float* tbias, int tbias_stride, int film, int p_thr16,
                    float inv_keep, const void* seed, int layer_id, void* dx, float* workspace, float* dgamma,
                    float* dbeta, float* dtbias, long long dtbias_stride, float* dxsum, void* stream);
/* Test windows onto the keep rule: the keep bytes (1 = kept) of the first `count` elements of a layer, on the device (seed: device
 * pointer) and on the host, and the generator itself (host only; ctr: 4, key: 2, out: 4 words).                          */
int ctsi_dropout_mask(const void* seed, int layer_id, int p_thr16, long long count, void* out_u8, void* stream);
int ctsi_dropout_mask_host(unsigned long long seed, int layer_id, int p_thr16, long long count, void* out_u8);
int ctsi_philox4x32_10_host(const uint32_t* ctr, const uint32_t* key, uint32_t* out);
/* TemporalAttention fast mode on fp32: depth sums + GroupNorm column sums (tiles of 64 positions per sample), the normalised
 * depth sum (fp32 [n][h*w][c]; the folded (proj_out . W_v) product is then one fp32 1x1x1 conv), and y = x + p broadcast
 * over depth.  Exact mode has no fp32 form (it is the same mathematics). */
int ctsi_attn_depthsum_f32_tiles(int h, int w);
int ctsi_attn_depthsum_f32(const float* x, float* depthsum, float* colsum, int n, int c, int d, int h, int w, void* stream);
int ctsi_attn_normsum_f32(const float* depthsum, const double* sums, const float* gamma, const float* beta, float* out,
                          int n, int c, int d, int h, int w, int groups, float eps, void* stream);
int ctsi_attn_broadcast_add_f32(const float* x, const float* p, float* y, int n, int c, int d, int h, int w, void* stream);
/* ctsi_ddim_step / ctsi_ddpm_step with the U-Net input slice `zin` written in fp32 (NDHWC, c_total channels, offset c_off). */
int ctsi_ddim_step_f32(float* z, const float* eps, const float* noise, float* zin, int c_total, int c_off, const float* coef,
                       const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite, void* stream);
int ctsi_ddpm_step_f32(float* z, const float* eps, const float* noise, float* zin, int c_total, int c_off, const float* coef,
                       const int* step_ptr, int n, int c, int d, int h, int w, void* stream);

/* DPM-Solver++(2M) update (multistep, data prediction; csrc/multistep.hip).  The arguments of ctsi_ddim_step /
 * ctsi_ddim_step_f32 without `noise` (the solver is deterministic), plus x0_prev: a persistent fp32 NDHWC buffer of z's
 * shape, allocated zeroed, that holds the previous step's data prediction; it is read and then overwritten with this
 * step's.  Row coef[*step_ptr] = {1/alpha_i, sigma_i/alpha_i, a_i, b_i, c_i, 0, 0, 0}:
 *   x0_i = clamp(nan_to_num(z_i/alpha_i - (sigma_i/alpha_i) eps_i), -10, 10),  z_{i+1} = a_i z_i + b_i x0_i + c_i x0_prev.
 * Writes z, x0_prev and the U-Net input slice (bf16 / fp32, channels [c_off, c_off+c) of c_total).  nonfinite as for
 * ctsi_ddim_step.  Capture-safe: no allocation, no synchronisation.                                                    */
int ctsi_dpm_step(float* z, const float* eps, float* x0_prev, void* zin_bf16, int c_total, int c_off, const float* coef,
                  const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite, void* stream);
int ctsi_dpm_step_f32(float* z, const float* eps, float* x0_prev, float* zin, int c_total, int c_off, const float* coef,
                      const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite, void* stream);

/* EDM Heun / Euler update (Karras et al. 2022, Algorithm 2; csrc/multistep.hip), one call per U-Net evaluation.  z
 * holds zhat, the VP latent of the churned state; d1: a persistent fp32 NDHWC buffer of z's shape, allocated zeroed, that
 * holds the predictor's data prediction; noise: fp32 NCDHW churn noise of the next step, or NULL (read only by rows with
 * c7 != 0).  Row coef[*step_ptr] = {c0, c1, c2, kind, c4, c5, c6, c7} (sampler.heun_coef_rows):
 *   D = clamp(nan_to_num(c0 z + c1 d1 - c2 eps), -10, 10)
 *   kind 0 (predictor): d1 = D, zin = c4 z + c5 D;   kind 1 (closing): z = zin = c4 z + c5 D + c6 d1 + c7 noise.
 * zin (the U-Net input slice, bf16 / fp32, channels [c_off, c_off+c) of c_total) is required: a predictor row writes
 * the corrector's input there only.  nonfinite as for ctsi_dpm_step.  Capture-safe: no allocation, no synchronisation. */
int ctsi_heun_step(float* z, const float* eps, float* d1, const float* noise, void* zin_bf16, int c_total, int c_off,
                   const float* coef, const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite,
                   void* stream);
int ctsi_heun_step_f32(float* z, const float* eps, float* d1, const float* noise, float* zin, int c_total, int c_off,
                       const float* coef, const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite,
                       void* stream);

/* Classifier-free guidance between the U-Net and the sampler update (csrc/guidance.hip).  `eps` is
 * the fp32 NDHWC noise prediction of a batch of 2n: rows [0, n) conditional (eps_c), rows [n, 2n) evaluated on the null
 * conditioning (eps_u).  Row scale[*step_ptr] = {s, phi} (row 0 when step_ptr is NULL): a device table, so a captured
 * graph serves every guidance scale.
 * ctsi_cfg_combine: rows [0, n) <- m_b (eps_u + s (eps_c - eps_u)) in place, m_b = phi stats[4 b + 2] + (1 - phi); m_b = 1
 *   when stats is NULL or phi == 0 (no statistics are read).  fp32 arithmetic, one fma per element.
 * ctsi_cfg_stats: partials[(b * ctsi_cfg_stats_blocks(c d h w) + x) * 4 ..] = fp64 sums of eps_c, eps_c^2, eps_g, eps_g^2
 *   (eps_g = eps_u + s (eps_c - eps_u) in fp64) over block x's share of sample b.
 * ctsi_cfg_stats_finalize: one block per sample adds its partials in a fixed order and writes stats[4 b ..] = { std_b(eps_c),
 *   std_b(eps_g), their ratio (1 when std_b(eps_g) == 0), element count }, unbiased as torch.std.  No atomics: the same
 *   bits on every run.
 * ctsi_cfg_mirror: `rows` rows of row_bytes at a pitch of stride_bytes copied from src to dst (the z half of the network
 *   input, rows [0, n) -> rows [n, 2n), after the update); sizes even, 16-byte accesses when sizes and pointers allow.
 * Null pointers / non-positive sizes return CTSI_ERR_INVALID before any launch.  Capture-safe. */
int ctsi_cfg_stats_blocks(long long per_sample);
int ctsi_cfg_combine(float* eps, const float* scale, const int* step_ptr, const double* stats, int n, int c, int d, int h,
                     int w, void* stream);
int ctsi_cfg_stats(const float* eps, const float* scale, const int* step_ptr, double* partials, int n, int c, int d, int h,
                   int w, void* stream);
int ctsi_cfg_stats_finalize(const double* partials, double* stats, int n, int c, int d, int h, int w, void* stream);
int ctsi_cfg_mirror(const void* src, void* dst, long long rows, int row_bytes, int stride_bytes, void* stream);

/* v-prediction (csrc/prediction.hip): the network predicts v = sqrt(abar) eps - sqrt(1 - abar) z_0.
 * ctsi_pred_to_eps: the model output becomes eps in place, fp32, elementwise over n rows of per_sample contiguous floats
 *   (any layout: the NDHWC step buffers and the NCDHW single-step tensors alike):
 *     out[b, i] <- a out[b, i] + b0 z[b % z_rows, i] + b1 hist[b % z_rows, i]
 *   {a, b0, b1, 0} = rows[(*step_ptr * rows_per_step + b % rows_per_step) * 4 ..], a device table (*step_ptr = 0 when
 *   step_ptr is NULL), so a captured graph serves every step.  z is loaded only by rows with b0 != 0, hist only by rows
 *   with b1 != 0; hist may be NULL (the caller then builds no row with b1 != 0).  z_rows <= n: a guided batch of 2n rows
 *   reads the n rows of z twice.  One product and one fma per term; 16-byte accesses when per_sample % 4 == 0 and every
 *   pointer is 16-byte aligned.
 * ctsi_q_sample_v: ctsi_q_sample (the same bf16 NDHWC z_t slice, the same bits) that also writes the training target
 *   v_target = sqrt_ac[t_b] noise - sqrt_1mac[t_b] z0 (fp32 NCDHW) in the same pass.
 * Null pointers / non-positive sizes / rows_per_step or z_rows outside [1, n] return CTSI_ERR_INVALID before any launch.
 * Capture-safe: no allocation, no synchronisation. */
int ctsi_pred_to_eps(float* out, const float* z, const float* hist, const float* rows, const int* step_ptr,
                     int rows_per_step, int n, int z_rows, long long per_sample, void* stream);
int ctsi_q_sample_v(const float* z0, const float* noise, const float* sqrt_ac, const float* sqrt_1mac, const int* t,
                    void* dst, float* v_target, int n, int c, int d, int h, int w, int c_total, int c_off, void* stream);

/* x0-form sampler update (csrc/x0_step.hip): the DDIM, DDPM and DPM-Solver++ updates of a v-prediction
 * model on the data prediction -- no division by alpha = sqrt(abar), which is 0 at the last step of a zero-terminal-SNR
 * schedule.  z, v (the network's raw output) and hist are fp32 NDHWC, noise fp32 NCDHW, zin the U-Net input slice as in
 * ctsi_ddim_step / ctsi_ddim_step_f32 (bf16 / fp32, channels [c_off, c_off+c) of c_total).  Row coef[*step_ptr] (row 0 when
 * step_ptr is NULL) = {alpha, sigma, a, b, c, s, clip, 0} (sampler.x0_coef_rows, float64 rounded once):
 *   X = clamp(nan_to_num(fma(alpha, z, -sigma v)), -clip, clip)   (clip = 0: no clamp)
 *   z <- zin <- a z + b X + c hist + s noise,   hist <- X.
 * hist is read only by rows with c != 0 and written whenever it is not NULL; noise is read only by rows with s != 0; hist,
 * noise, zin, step_ptr and nonfinite may be NULL.  nonfinite as for ctsi_ddim_step: row *step_ptr counts {v NaN, Inf, X NaN,
 * Inf, z after update NaN, Inf}; v and the result pass through nan_to_num.  16-byte accesses when c % 4 == 0 and the
 * pointers allow, one element per thread otherwise.  Null z / v / coef, non-positive sizes or a channel slice outside
 * c_total return CTSI_ERR_INVALID before any launch.  Capture-safe: no allocation, no synchronisation. */
int ctsi_x0_step(float* z, const float* v, float* hist, const float* noise_ncdhw, void* zin_bf16, int c_total, int c_off,
                 const float* coef, const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite, void* stream);
int ctsi_x0_step_f32(float* z, const float* v, float* hist, const float* noise_ncdhw, float* zin, int c_total, int c_off,
                     const float* coef, const int* step_ptr, int n, int c, int d, int h, int w, int* nonfinite,
                     void* stream);

/* Learned reverse variance and the respaced ancestral step (csrc/learned_sigma.hip; Nichol & Dhariwal 2021).
 * ctsi_sigma_split: out2 is the fp32 NDHWC output of a 2L-channel head, n rows.  One pass writes channels [0, L) of every row,
 *   packed, into eps (fp32 NDHWC, L channels, n rows) and -- when vraw is not NULL -- channels [L, 2L) of rows [0, n_keep) into
 *   vraw (fp32 NDHWC, L channels, n_keep rows; under guidance the conditional half).  n_keep in [1, n] with vraw, [0, n] without.
 * ctsi_ddpm_lv_step / _f32: ctsi_ddpm_step / ctsi_ddpm_step_f32 with the reverse variance taken per element.  Row coef[*step_ptr]
 *   (row 0 when step_ptr is NULL) = {sqrt(1 - abar), sqrt(abar), coef1', coef2', log beta', log beta~' (clipped), s, clip}
 *   with s = [not the last step] exp(log beta~' / 2), the fixed-small noise scale (learned_sigma.respaced_ddpm_rows, float64
 *   rounded once; on the full chain the fp32 values of ctsi_ddpm_step's rows):
 *     z0   = clamp(nan_to_num((z - c0 nan_to_num(eps)) / c1), -clip, clip)      (clip = 0: no clamp)
 *     mean = c2 z0 + c3 z
 *     lv   = f c4 + (1 - f) c5,  f = (vraw + 1) / 2  (not clamped)               (vraw == NULL: lv = c5, the fixed-small variance)
 *     z <- zin <- nan_to_num(mean + s exp((lv - c5) / 2) noise)                   (= [not last] exp(lv / 2) noise; evaluated as
 *                                                                                  s exp(f (c4 - c5) / 2), s alone when vraw == NULL;
 *                                                                                  noise == NULL: the mean)
 *   z, eps, vraw fp32 NDHWC; noise fp32 NCDHW; zin as in ctsi_ddpm_step.  With vraw == NULL, clip = 1 and the rows of the
 *   full-length chain the result has ctsi_ddpm_step's bits on every row: the scale is the same fp32 number and the mean is
 *   written with the same roundings.
 * ctsi_ddpm_posterior_lv: the same step on fp32 NCDHW tensors with one row per sample (coef[b * 8 ..]), as ctsi_ddpm_posterior:
 *   out (may be NULL) <- the updated sample, logvar_out (may be NULL; needs vraw) <- lv per element.
 * ctsi_hybrid_loss_fwd / _bwd: the training loss L_simple + lambda L_vb of a learn_sigma model.  pred2: fp32 NDHWC, 2L channels
 *   ([0, L) the prediction p, [L, 2L) the variance channels v); z0, noise: fp32 NCDHW; t: n device ints in [0, timesteps); sched:
 *   one row per timestep {sqrt(abar), sqrt(1 - abar), coef1, coef2, log beta, log beta~ (clipped), log beta - log beta~, 0}
 *   (learned_sigma.loss_schedule_rows); v_pred: 0 = p is eps, 1 = p is v; mask: fp32 (n, L, d) or NULL; norm[b] / norm_vb[b]: the
 *   per-sample factors of the two terms (batch, element count, loss weight; lambda / ln 2 for the bound), folded on the host.
 *   Per element, with z_t = a z0 + s noise rebuilt in registers, z0_pred = (z_t - s p) / a  |  a z_t - s p (not clipped),
 *   lv = f c4 + (1 - f) c5 = c5 + f c6, f = (v + 1) / 2 (c6 is the float64 difference rounded once: at large t the two logs agree to
 *   a few 1e-3 and the bound's terms are of that order):
 *     mse term = (p - target)^2,  target = noise | a noise - s z0
 *     t > 0: vb term = 1/2 (-1 + lv - c5 + e^(c5 - lv) + (c1 (z0 - z0_pred))^2 e^-lv)     KL(q(z_{t-1} | z_t, z_0) || p_theta), nats
 *     t = 0: vb term = 1/2 (ln 2 pi + lv + (z0 - c1 z0_pred - c2 z_t)^2 e^-lv)             continuous Gaussian NLL, nats
 *   forward: loss_out = {total, mse, vb, S_0 .. S_{n-1}, V_0 .. V_{n-1}} with S_b / V_b the sample's masked sums of the two
 *   terms, mse = sum_b norm[b] S_b, vb = sum_b norm_vb[b] V_b, total = mse + vb; fp64 partials (workspace:
 *   ctsi_hybrid_loss_workspace_doubles(n) doubles) added in a fixed order.
 *   backward: dpred (bf16 NDHWC, c_stride >= 2L channels per voxel, padding channels zeroed) <- gscale[0] (1 when NULL) times
 *   2 norm[b] mask (p - target) in channels [0, L) and norm_vb[b] mask d(vb term)/dv in channels [L, 2L), d lv / dv = (c4 - c5) / 2;
 *   the bound sends no gradient to p (the mean is detached, as in the paper).
 * 16-byte accesses in the split and the steps when L (c) % 4 == 0 and the pointers allow, one element per thread otherwise.  Null
 * pointers / non-positive sizes / a channel slice outside c_total / n_keep outside its range / c_stride < 2L return
 * CTSI_ERR_INVALID before any launch.  No atomics: every result is bit-identical run to run.  Capture-safe: no allocation, no
 * synchronisation. */
int ctsi_sigma_split(const float* out2, float* eps, float* vraw, int n, int n_keep, int L, int d, int h, int w, void* stream);
int ctsi_ddpm_lv_step(float* z, const float* eps, const float* vraw, const float* noise_ncdhw, void* zin_bf16, int c_total,
                      int c_off, const float* coef, const int* step_ptr, int n, int c, int d, int h, int w, void* stream);
int ctsi_ddpm_lv_step_f32(float* z, const float* eps, const float* vraw, const float* noise_ncdhw, float* zin, int c_total,
                          int c_off, const float* coef, const int* step_ptr, int n, int c, int d, int h, int w, void* stream);
int ctsi_ddpm_posterior_lv(const float* z, const float* eps, const float* vraw, const float* noise, float* out,
                           float* logvar_out, const float* coef, int n, long long per_sample, void* stream);
size_t ctsi_hybrid_loss_workspace_doubles(int n);
int ctsi_hybrid_loss_fwd(const float* pred2, const float* z0, const float* noise, const int* t, const float* sched,
                         int timesteps, int v_pred, const float* mask, const float* norm, const float* norm_vb, int n, int L,
                         int d, int h, int w, double* workspace, float* loss_out, void* stream);
int ctsi_hybrid_loss_bwd(const float* pred2, const float* z0, const float* noise, const int* t, const float* sched,
                         int timesteps, int v_pred, const float* mask, const float* norm, const float* norm_vb,
                         const float* gscale, int n, int L, int d, int h, int w, void* dpred_bf16, int c_stride, void* stream);

/* VGG-19 perceptual loss (csrc/vgg_loss.hip): the passes around its planar (1,3,3) convolutions, which run
 * on conv plans.  Images are bf16 channels-last [image][h][w][c]; c and every `count` are multiples of 8 (16-byte accesses).
 * ctsi_vgg_prep: image i = b * num + s <- slice slices[s] of sample b of x (fp32 NCDHW, C = 1): channels 0-2 are
 *   ((x + 1) / 2 - norm[c]) / norm[3 + c] (norm = {mean[3], std[3]}, device), channels 3-7 zero.  slices: num device ints
 *   in [0, d), all different.
 * ctsi_vgg_prep_bwd: grad_pred (fp32, the shape of x) = sum_c g_c / (2 std_c) on the sampled slices and exactly zero on the
 *   others (the entry clears the tensor itself when num < d); g: the 8-channel image gradient.
 * ctsi_maxpool2_fwd / _bwd: 2 x 2 / stride 2 max pooling of n images (h, w >= 2) to h / 2 x w / 2; an odd last row / column
 *   takes part in no window (torch's floor).  The backward routes each gradient to the FIRST maximum of its window in (h, w)
 *   row-major order (torch's tie rule) and writes zeros to the other three positions and to an odd last row / column.
 * ctsi_relu_bf16: x <- max(x, 0) in place.
 * ctsi_feat_loss_fwd: partials[0 .. ctsi_feat_loss_blocks()) <- fixed-order fp64 partial sums of |pred - target| (squared 0)
 *   or (pred - target)^2 over `count` elements.  ctsi_feat_loss_finalize: out[1 + l] = (sum of layer l's partials, stored at
 *   partials + l * ctsi_feat_loss_blocks()) / counts[l], out[0] = the average of the `layers` (<= 64) means; one launch.
 * ctsi_feat_grad_relu_bwd: g_out = (g_in + coef * grad_loss[0] * f(y - target)) * [y > 0] over `count` elements; kind 1: f =
 *   sign, kind 2: f(v) = 2 v, kind 0: no loss term (target, grad_loss unused; g_in required); relu 0: no mask; g_in may be
 *   NULL for kind != 0; g_out may alias g_in.  y is the stored (post-ReLU where masked) activation: no mask is stored.
 * No entry allocates, synchronises or keeps state; no float atomics: every result is bit-identical run to run.  Bad
 * arguments return CTSI_ERR_INVALID before any launch. */
int ctsi_vgg_prep(const float* x, const int* slices, const float* norm, void* dst, int b, int d, int num, int h, int w,
                  void* stream);
int ctsi_vgg_prep_bwd(const void* g, const int* slices, const float* norm, float* grad_pred, int b, int d, int num, int h,
                      int w, void* stream);
int ctsi_maxpool2_fwd(const void* x, void* y, int n, int h, int w, int c, void* stream);
int ctsi_maxpool2_bwd(const void* x, const void* gy, void* gx, int n, int h, int w, int c, void* stream);
int ctsi_relu_bf16(void* x, long long count, void* stream);
int ctsi_feat_loss_blocks(void);
int ctsi_feat_loss_fwd(const void* pred, const void* target, long long count, int squared, double* partials, void* stream);
int ctsi_feat_loss_finalize(const double* partials, const long long* counts, int layers, float* out, void* stream);
int ctsi_feat_grad_relu_bwd(const void* g_in, const void* y, const void* target, void* g_out, long long count, float coef,
                            int kind, int relu, const float* grad_loss, void* stream);

/* LPIPS perceptual distance (csrc/lpips.hip): what lpips 0.1.x (net = 'vgg') adds to a VGG-16 stack that
 * runs on the entries above.  Features are bf16 channels-last [image][positions][c]; a ROW is the c channels of one position,
 * c / 8 lanes of one 16-byte load: c is 64, 128, 256 or 512.  eps = 1e-10.
 * ctsi_lpips_prep: image n of x (fp32 NCHW, c = 1 or 3; c = 1: the grey value in all three channels) -> the 8-channel bf16
 *   image, channel k < 3 = (v - shift_k) / scale_k (shift = -0.030, -0.088, -0.188; scale = 0.458, 0.448, 0.450), v = x or, with
 *   normalize, 2 x - 1; channels 3-7 zero.  ctsi_lpips_prep_bwd: grad (fp32, the shape of x) from the 8-channel image gradient
 *   g: g_k / scale_k (twice that with normalize), c = 1: the sum of the three.
 * ctsi_lpips_dist_fwd: one tap.  u = y / (|y| + eps), v = target / (|target| + eps) per row (|.| the row's 2-norm);
 *   partials[i * ctsi_lpips_blocks() + b] <- fixed-order fp64 partial sums of sum_c w_c (u_c - v_c)^2 over the rows of image i
 *   (0 for a block without rows).  w: c device floats.  Each feature element is read once; nothing else is written.
 * ctsi_lpips_finalize: partials of `taps` (<= 16) taps stored as [tap][image][ctsi_lpips_blocks()]; out[i] = sum over taps of
 *   (image i's sum) / positions[tap], tap_means[tap] = the mean over the images of that quotient; one launch.
 * ctsi_lpips_grad_relu_bwd: g_out = (g_in + grad_out[image] / positions * d) * [y > 0] with r = 2 w (u - v) and
 *   d = r / (a + eps) - y (y . r) / (a (a + eps)^2), a = |y|; a row with a = 0 gets exact zeros, never a NaN or Inf.  The row
 *   norms are recomputed, not stored by the forward.  g_in may be NULL; g_out may alias g_in.  grad_out: `images` device floats.
 * No entry allocates, synchronises or keeps state; no float atomics: every result is bit-identical run to run.  Bad
 * arguments return CTSI_ERR_INVALID before any launch. */
int ctsi_lpips_blocks(void);
int ctsi_lpips_prep(const float* x, void* dst, int n, int c, int h, int w, int normalize, void* stream);
int ctsi_lpips_prep_bwd(const void* g, float* grad, int n, int c, int h, int w, int normalize, void* stream);
int ctsi_lpips_dist_fwd(const void* y, const void* target, const float* w, int images, long long positions, int c,
                        double* partials, void* stream);
int ctsi_lpips_finalize(const double* partials, const long long* positions, int taps, int images, float* out,
                        float* tap_means, void* stream);
int ctsi_lpips_grad_relu_bwd(const void* g_in, const void* y, const void* target, const float* w, void* g_out, int images,
                             long long positions, int c, const float* grad_out, void* stream);

/* hipGraph helpers (one captured graph per denoising step) -------------------------------- */
typedef struct ctsi_graph ctsi_graph;
int ctsi_graph_begin_capture(void* stream);
int ctsi_graph_end_capture(void* stream, ctsi_graph** graph);
int ctsi_graph_launch(ctsi_graph* graph, void* stream);
void ctsi_graph_destroy(ctsi_graph* graph);

/* Latent-space window fusion (csrc/window_fuse.hip): the overlapping windows of a stitched volume share
 * one latent; per U-Net evaluation the network runs on all windows as one batch and these two passes move the data.
 * Rows: the full tensors hold `batch` samples per guidance half; window row (g nw + k) batch + b is window k of sample b in
 * half g, k = (kd nwh + kh) nww + kw over the product grid of per-axis window starts.  All tensors are NDHWC.
 * ctsi_window_gather / _f32: dst row (g nw + k) batch + b <- the (td, lh, lw) window of src row b at starts[3k .. 3k+2]
 *   (int32 device table of latent starts); channels [0, L) of c_total per voxel on either side, bf16 / fp32.  `halves` (1 | 2)
 *   destination halves read the same `batch` source rows.  A pure copy, bit exact; the widest of 16- / 8- / 4- / 2-byte
 *   accesses that divides L and both pitches and matches the pointers.  Every start must lie in [0, full - window]: the kernel does not check.
 * ctsi_window_blend: full[g batch + b][v] = sum over (kd, kh, kw) of wd wh ww win[(g nw + k) batch + b][v - s_k], fp32, C
 *   channels (a multiple of 4), in that fixed order with one fma per term: no accumulator tensor, no atomics.  tab_i: per axis
 *   (d, h, w in turn; P = full size, K = kd | kh | kw = the largest number of windows over one position) int32 [P] counts,
 *   [P][K] window indices along the axis, [P][K] positions inside that window; tab_w: per axis fp32 [P][K] weights, normalised
 *   per axis to sum to 1 at every position (window_fuse.axis_table, which validates the windows; the kernel trusts the table).
 * Null pointers / bad sizes return CTSI_ERR_INVALID before any launch.  Capture-safe: no allocation, no synchronisation. */
int ctsi_window_gather(const void* src_bf16, void* dst_bf16, const int* starts, int batch, int halves, int nw, int D, int H,
                       int W, int td, int lh, int lw, int L, int src_c_total, int dst_c_total, void* stream);
int ctsi_window_gather_f32(const float* src, float* dst, const int* starts, int batch, int halves, int nw, int D, int H, int W,
                           int td, int lh, int lw, int L, int src_c_total, int dst_c_total, void* stream);
int ctsi_window_blend(const float* win, float* full, const int* tab_i, const float* tab_w, int batch, int halves, int nwd,
                      int nwh, int nww, int D, int H, int W, int td, int lh, int lw, int C, int kd, int kh, int kw, void* stream);

/* Image-space loss terms of the diffusion stage (csrc/image_loss.hip): the training step's predicted clean
 * latent as a second, differentiable output, and the loss-head backward that takes its gradient back in.
 * ctsi_z0_pred: out (fp32 NCDHW (n, c, d, h, w)) = the clean latent the training step's prediction stands for.  z0, noise:
 *   fp32 NCDHW; pred: the raw network output, fp32 NDHWC with c_stride >= c floats per voxel; sqrt_ac / sqrt_1mac: the
 *   schedule tables q_sample reads, indexed by t[b]; active: int32 (n).  With z_t = sqrt_ac[t] z0 + sqrt_1mac[t] noise,
 *     v_prediction == 0:  out = (z_t - sqrt_1mac[t] pred) / sqrt_ac[t]      (ctsi_ddpm_posterior's z_0: one fma, one division)
 *     v_prediction != 0:  out = sqrt_ac[t] z_t - sqrt_1mac[t] pred          (no division)
 *   Rows with active[b] == 0 are copies of z0 (bit for bit): nothing non-finite and no 1 / sqrt_ac blow-up at t -> T, whatever
 *   pred holds there.  16-byte accesses when c, c_stride and d h w are multiples of 4 and every pointer is 16-byte aligned,
 *   element-wise otherwise.
 * ctsi_loss_bwd_z0: ctsi_mse_loss_bwd with the gradient g_z0 (fp32 NCDHW) of ctsi_z0_pred's output added in fp32 BEFORE the
 *   one rounding to bf16:
 *     dpred = bf16(2 norm[b] mask (pred - target) gscale[0] + active[b] coef[b] g_z0),   channels c .. c_stride-1 zero,
 *   coef[b] = d out / d pred of the row: -sqrt_1mac[t_b] / sqrt_ac[t_b] (epsilon) or -sqrt_1mac[t_b] (v), formed by the caller.
 *   pred: fp32 NDHWC with c floats per voxel, target: fp32 NCDHW, mask: fp32 (n, c, d) or NULL (it acts on the first term
 *   only), gscale: NULL = 1.  g_z0 of a row with active[b] == 0 is not read.  g_z0 == 0 gives ctsi_mse_loss_bwd's bits.
 * Null pointers / non-positive sizes / c_stride < c return CTSI_ERR_INVALID before any launch.  Capture-safe: no
 * allocation, no synchronisation. */
int ctsi_z0_pred(const float* z0, const float* noise, const float* pred, int c_stride, const float* sqrt_ac,
                 const float* sqrt_1mac, const int* t, const int* active, int v_prediction, int n, int c, int d, int h, int w,
                 float* out, void* stream);
int ctsi_loss_bwd_z0(const float* pred, const float* target, const float* mask, const float* norm, const float* gscale,
                     const float* g_z0, const int* active, const float* coef, int n, int c, int d, int h, int w, void* dpred,
                     int c_stride, void* stream);

/* timing helpers used by bench.py (HIP events on the engine's own stream) ----------------- */
typedef struct ctsi_event ctsi_event;
int ctsi_event_create(ctsi_event** ev);
int ctsi_event_record(ctsi_event* ev, void* stream);
/* device-side wait of `stream` for `ev` (no host sync; forks / joins a stream capture) */
int ctsi_stream_wait_event(void* stream, ctsi_event* ev);
int ctsi_event_elapsed_ms(ctsi_event* start, ctsi_event* stop, float* ms);
void ctsi_event_destroy(ctsi_event* ev);

/* Data consistency along depth (csrc/depth_consistency.hip).  x is a thin fp32 NCDHW volume of d_out
 * slices, y the acquired thick one of d_in slices; planes = N C, hw = H W, a column is the depth vector at one (plane,
 * position).  W [d_in][d_out] fp32 is the slice profile (rows sum to 1), P [d_out][d_in] fp32 = W^T (W W^T)^-1; band /
 * band_w [d_in][2] and band_p [d_out][2] (int32) hold the first and last non-zero column of each row of W and of P.
 * ctsi_depth_measure: y_out = W x.  ctsi_depth_measure_adj: g_x = scale W^T g_y (accumulate == 0) or g_x += ... (!= 0).
 * ctsi_depth_project: in place, `iters` times x <- x + P (y - W x) with x <- clamp(x, clamp_lo, clamp_hi) between
 *   iterations; after the last iteration the clamp is applied only when clamp_mode == 2.  clamp_mode 0: no clamp; 1: clamp
 *   between iterations, ending on a projection (exactly consistent, may leave the range); 2: ending on a clamp (in range,
 *   approximately consistent).  One block stages a tile of whole columns in LDS: x is read once and written once whatever
 *   iters is.  partials (may be NULL): 5 fp64 values per slot, ctsi_depth_project_blocks(planes, hw) slots (one per 32
 *   positions of a plane: the count does not depend on the depths), every slot written by one block.
 * ctsi_depth_project_finalize: one block per plane folds its slots in index order into stats[5 plane ..] = { sum r^2 before,
 *   sum r^2 after, max |r| before, max |r| after, number of clamped voxels (every clamp application counts) }, r = y - W x
 *   evaluated in fp64 on the kernel's fp32 input / output values.  No atomics: the same bits on every run.
 * Limits d_in <= 64, d_out <= 512.  Null pointers, non-positive sizes, iters < 1, clamp_lo > clamp_hi, a bad clamp_mode and
 * depths over the limits return CTSI_ERR_INVALID before any launch.  Capture-safe: no allocation, no synchronisation. */
int ctsi_depth_measure(const float* x, const float* W, const int* band, float* y_out, int planes, int d_in, int d_out,
                       int hw, void* stream);
int ctsi_depth_measure_adj(const float* g_y, const float* W, const int* band, float* g_x, float scale, int accumulate,
                           int planes, int d_in, int d_out, int hw, void* stream);
int ctsi_depth_project(float* x, const float* y, const float* W, const float* P, const int* band_w, const int* band_p,
                       int iters, float clamp_lo, float clamp_hi, int clamp_mode, double* partials, int planes, int d_in,
                       int d_out, int hw, void* stream);
int ctsi_depth_project_blocks(int planes, int hw);
int ctsi_depth_project_finalize(const double* partials, double* stats, int planes, int hw, int d_in, void* stream);

/* Ensemble statistics (csrc/ensemble.hip): per-voxel mean and spread over the members of an ensemble of
 * fp32 volumes, kept as a running state so that memory does not grow with the number of members.
 * ctsi_ensemble_accumulate: x holds `rows` members of `count` contiguous values each; (mean, m2) [count] is the state over the
 *   `seen` members folded in before.  Per element the state is read once, the sequential Welford recurrence runs over the
 *   rows in order (k = seen + r + 1, d = x - mean, mean += d / k, m2 += d (x - mean), every operation rounded on its own) and
 *   the state is written once.  seen == 0: the state is NOT read (no memset before the first call) and member 1 sets
 *   mean = x, m2 = 0.  Any split of the members over calls gives the same bits.  Traffic (rows + 4) * 4 bytes per element,
 *   (rows + 2) * 4 on the first call.  16-byte accesses when x, its rows, mean and m2 reach a 16-byte boundary after the same
 *   number of leading elements, else 8-byte or scalar ones.
 * ctsi_ensemble_finalize: std = sqrt(max(m2, 0) / (members - (unbiased != 0))), exactly 0 when members == 1, written to a buffer
 *   of its own (the state stays valid: more members may follow), and stats[planes][3] (fp64) = { sum std, sum std^2, max std }
 *   over each plane of `plane` consecutive voxels.  partials: 4 fp64 values per slot, ctsi_ensemble_blocks(planes, plane)
 *   slots (one per 4096 voxels of a plane; 0 for sizes that are invalid), every slot written by one block; a second launch
 *   folds each plane's slots in index order.
 * ctsi_ensemble_calibration: stats[planes][4] (fp64) = { sum (mean - target)^2, sum std^2, #(|mean - target| <= std),
 *   #(|mean - target| <= 2 std) } per plane, decided in fp64 on the fp32 values; partials as above.
 * Null pointers, pointers that are not 4-byte aligned, rows < 1, count < 1, seen < 0, seen + rows > INT_MAX, members < 1,
 * planes < 1 and plane < 1 return CTSI_ERR_INVALID before any launch.  Capture-safe: no allocation, no synchronisation, no
 * atomics; the same bits on every run. */
int ctsi_ensemble_accumulate(const float* x, int rows, long long count, int seen, float* mean, float* m2, void* stream);
int ctsi_ensemble_blocks(int planes, long long plane);
int ctsi_ensemble_finalize(const float* m2, float* std_out, int members, int unbiased, int planes, long long plane,
                           double* partials, double* stats, void* stream);
int ctsi_ensemble_calibration(const float* mean, const float* std_in, const float* target, int planes, long long plane,
                              double* partials, double* stats, void* stream);

/* Measurement guidance (csrc/measure_guide.hip): the device passes of one guided sampler evaluation around
 * the decoder's data-gradient tape.  Latents are n samples of c channels on d x h x w voxels.
 * ctsi_guide_z0: the predicted clean latent, z0_out (fp32 NCDHW) from z_t and eps (both fp32 NDHWC, c floats per voxel):
 *   mode 0  z0 = clip(nan_to_num((z_t - sigma nan_to_num(eps)) / alpha))     (the eps-form updates; alpha != 0)
 *   mode 1  z0 = clip(nan_to_num(fma(alpha, z_t, -(sigma nan_to_num(eps)))))  (the x0 form on the raw v, and rows that hold
 *           1 / alpha and sigma / alpha);  clip(v) = clamp(v, -clip, clip), clip == 0: no clamp.
 * ctsi_depth_residual_adj: x a thin fp32 NCDHW volume (n, c, d_out, hw), y the thick one (n, c, d_in, hw), W [d_in][d_out] and
 *   band [d_in][2] as for ctsi_depth_measure.  One pass: g_x = -W^T (y - W x) (fp32, x's shape; it may not alias x) and
 *   sumsq[b] (fp64, n values) = sum over sample b of r^2, r = y - W x re-evaluated in fp64 on the fp32 values.  A block stages
 *   a tile of whole depth columns in LDS, so x is read once and g_x written once.  partials: one fp64 per slot,
 *   ctsi_depth_project_blocks(n c, hw) slots, every slot written by one block; a second launch folds each sample's slots in
 *   index order.  No atomics: the same bits on every run.  Limits d_in <= 64, d_out <= 512.
 * ctsi_guide_apply: per sample b, s_b = 1 / sqrt(sumsq[b]) (normalize == 1; a sample whose sumsq is 0 or not finite is left
 *   untouched, bit for bit) or 1 (normalize == 0, sumsq may be NULL); in fp32, c_z = coef_z s_b and c_h = coef_hist s_b (the
 *   products formed in fp64 and rounded once).  z (fp32 NDHWC, in place) <- nan_to_num(fma(c_z, g_z, z)) with g_z fp32 NCDHW;
 *   hist (fp32 NDHWC, may be NULL) <- nan_to_num(fma(c_h, g_z, hist)); zin (bf16, may be NULL: voxel stride c_total, channel
 *   offset c_off -- the operands of ctsi_x0_step) <- bf16(z) for every sample; its other channels are not touched.  The
 *   factors are read from device memory: no host synchronisation.
 * Null pointers (other than the optional ones), non-positive sizes, a bad mode / normalize flag / channel slice, clip < 0,
 * alpha == 0 in mode 0 and depths over the limits return CTSI_ERR_INVALID before any launch.  Capture-safe: no allocation,
 * no synchronisation. */
int ctsi_guide_z0(const float* z_t, const float* eps, float alpha, float sigma, int mode, float clip, float* z0_out, int n,
                  int c, int d, int h, int w, void* stream);
int ctsi_depth_residual_adj(const float* x, const float* y, const float* W, const int* band, float* g_x, double* partials,
                            double* sumsq, int n, int c, int d_in, int d_out, int hw, void* stream);
int ctsi_guide_apply(float* z, float* hist, const float* g_z, const double* sumsq, float coef_z, float coef_hist,
                     int normalize, void* zin, int c_total, int c_off, int n, int c, int d, int h, int w, void* stream);

/* Training patches from volumes resident in HBM (csrc/patch_sample.hip): the crop, depth resample, flips
 * and rot90 of the reference's patch dataset for a whole batch in one launch.
 * table: n rows of CTSI_PATCH_COLS int64 on the device --
 *   { thin pointer, thick pointer, d_thin, d_thick, h, w, z, y0, x0, k0, k1, flags }
 *   -- the two volumes of the sample ((d, h, w) contiguous, `storage` elements: CTSI_PATCH_F32 or CTSI_PATCH_F16), their
 *   sizes, the corner of the thin window, the thick slice range [k0, k1) and flags = flip W | flip H << 1 | k << 2.
 * out_thin (n, 1, depth_thin, ph, pw) fp32: out[d, i, j] = src[z + d, y0 + i', x0 + j'] with (i', j') the preimage of (i, j)
 *   under "flip W, then flip H, then rot90 k" (torch.flip / torch.rot90 on the last two axes); slices d >= d_thin - z are -1.
 * out_thick (n, 1, depth_thick, ph, pw) fp32: the k1 - k0 thick slices of the same window resampled linearly along depth as
 *   F.interpolate(mode='trilinear', align_corners=False) does in fp32, under the same in-plane map.  depth_thick == 0 with
 *   out_thick == NULL writes no thick output (the thick pointer of the rows is then not read).
 * A pure gather: no atomics, every output element written once, nothing read outside the windows.  Odd k needs ph == pw.
 * The table lives on the device, so its rows are the caller's to validate (device_data.DevicePatchSampler does); null
 * pointers, a bad storage type, non-positive sizes and n > 65535 return CTSI_ERR_INVALID before any launch.  Capture-safe:
 * no allocation, no synchronisation. */
#define CTSI_PATCH_COLS 12
#define CTSI_PATCH_F32 0
#define CTSI_PATCH_F16 1
int ctsi_patch_sample(const long long* table, int n, int storage, int depth_thin, int depth_thick, int ph, int pw,
                      float* out_thin, float* out_thick, void* stream);

/* depth-sharding collectives (RCCL over xGMI, one process per GPU) --------------------------- *
 * a volume's depth is cut into `world` slabs; before a depth-3 conv a slab needs one boundary
 * slice of each depth neighbour (models/unet3d.py:56,96,204-207,218-221; models/vae.py:27,65-69,86-90), GroupNorm needs
 * (sum, sumsq) over the whole depth (unet3d.py:59,97,151,329) and TemporalAttention the depth sum.  Each call below is
 * ONE sync point on `stream` (one RCCL group) and is stream-capture safe.  RCCL is bound at run time (dlopen; a librccl
 * already in the process is reused).
 *   host protocol: rank 0 calls ctsi_comm_unique_id, the 128 bytes are broadcast by the host (torch.distributed, MPI, a
 *   file ...), every rank calls ctsi_comm_init with the current HIP device set.                                        */
typedef struct ctsi_comm ctsi_comm;
int ctsi_comm_unique_id(void* id128);
/* world == 1 with id128 == NULL: no RCCL at all (every exchange degenerates to the volume-end zero fill). */
int ctsi_comm_init(ctsi_comm** comm, const void* id128, int rank, int world);
void ctsi_comm_destroy(ctsi_comm* comm);
int ctsi_comm_rank(const ctsi_comm* comm);
int ctsi_comm_world(const ctsi_comm* comm);
/* lo_halo <- rank-1's hi_own, hi_halo <- rank+1's lo_own (`bytes` each; zeros at the volume's ends). */
int ctsi_halo_exchange(ctsi_comm* comm, const void* lo_own, const void* hi_own, void* lo_halo, void* hi_halo,
                       size_t bytes, void* stream);
/* the same exchange plus, in the same sync point, sums[nsums] (fp64) and f32[nf32] summed over all ranks in place
 * (GroupNorm statistics travel with the boundary slices of the tensor they normalise); any part may be absent. */
int ctsi_halo_exchange_reduce(ctsi_comm* comm, const void* lo_own, const void* hi_own, void* lo_halo, void* hi_halo,
                              size_t bytes, double* sums, int nsums, float* f32, long long nf32, void* stream);
/* GroupNorm statistics (and optionally the TemporalAttention depth sum, fp32) summed over all ranks in place. */
int ctsi_gn_allreduce(ctsi_comm* comm, double* sums, int nsums, float* f32, long long nf32, void* stream);
/* recv = concatenation over ranks of `bytes` from each rank's send (result gather along depth). */
int ctsi_comm_allgather(ctsi_comm* comm, const void* send, void* recv, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTSI_H */
