// Optimizer step of the training path on the device (reference: training/train.py:172-212 builds
// torch.optim.Adam / AdamW over per-module parameter groups with their own learning rates, training/trainer.py:237-247 steps
// it once per accumulation window).
//
// ONE launch for all tensors of all parameter groups ("multi-tensor apply"): a device table of tensors {param, grad, exp_avg,
// exp_avg_sq, numel, group} and a table of 64 Ki-element chunks {tensor, first element}; block b owns chunk b.  HBM-bound:
// 16 B read + 12 B written per element (fp32 master weights and both moments; 264.66 M parameters = 7.4 GB per step).  The
// arithmetic is torch.optim.AdamW's single-tensor form, operation by operation in fp32 (decoupled decay first, lerp, addcmul,
// bias corrections folded into step_size / denominator the way torch folds them), so parameters track torch's to rounding.
// The bf16 kernel images the conv kernels read are re-packed by the engine right behind this launch (engine.Program.
// fast_repack: one ctsi_copy_scale_multi for every small fp32 operand + one pack launch per conv image).
#include "ctsi_internal.h"

struct CtsiOptTensor {       // 48 bytes
    float* p;
    const float* g;
    float* m;
    float* v;
    long long numel;
    int group;
    int pad;
};
struct CtsiOptGroup {        // 64 bytes per hyper-parameter row, refreshed by the host before every step.  Everything torch derives
    float lr, beta1, beta2, eps, weight_decay;   // in Python doubles (1 - beta, 1 - lr wd, the bias corrections) arrives already
    float step_size;         // lr / (1 - beta1^t)            rounded from the double, so the kernel sees torch's constants
    float bc2_sqrt;          // sqrt(1 - beta2^t)
    float decay;             // 1 - lr * weight_decay
    float one_m_b1, one_m_b2;
    float grad_scale;        // gradients are multiplied by this first (1 / loss-scale when the caller unscales here; 1 otherwise)
    int decoupled;           // 1: AdamW (p *= 1 - lr wd); 0: Adam with L2 (g += wd p)
    int maximize;
    int pad[3];
};
static constexpr int OPT_CHUNK = 65536;

__global__ void __launch_bounds__(256)
adamw_multi_kernel(const CtsiOptTensor* __restrict__ tensors, const CtsiOptGroup* __restrict__ groups,
                   const int2* __restrict__ chunks /* {tensor, first element / 4} */) {
    const int2 ck = chunks[blockIdx.x];
    const CtsiOptTensor t = tensors[ck.x];
    const CtsiOptGroup h = groups[t.group];
    const long long e0 = (long long)ck.y * 4;
    long long e1 = e0 + OPT_CHUNK;
    if (e1 > t.numel) e1 = t.numel;
    // torch's kernels, operation by operation (each line = one torch op; the compiler may contract a * b + c into an fma
    // exactly where torch's pointwise functors get contracted):
    auto upd = [&](float& p, float g, float& m, float& v) {
        g *= h.grad_scale;
        if (h.maximize) g = -g;
        if (h.decoupled) p *= h.decay; else g = g + h.weight_decay * p;     // param.mul_(1 - lr wd) | grad.add(param, alpha=wd)
        m = m + h.one_m_b1 * (g - m);                        // exp_avg.lerp_(grad, 1 - beta1)
        const float vb = v * h.beta2;                        // exp_avg_sq.mul_(beta2)
        const float gg = g * g;
        v = vb + h.one_m_b2 * gg;                            //           .addcmul_(grad, grad, value=1 - beta2)
        const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;   // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
        const float r = m / denom;
        p = p - h.step_size * r;                             // param.addcdiv_(exp_avg, denom, value=-step_size)
    };
    const bool vec = ((((unsigned long long)t.p | (unsigned long long)t.g | (unsigned long long)t.m | (unsigned long long)t.v) & 15ull) == 0);
    if (vec) {
        const long long q0 = e0 >> 2, q1 = e1 >> 2;          // whole float4 groups (e0 is a multiple of 4)
        for (long long q = q0 + threadIdx.x; q < q1; q += 256) {
            float4 p = reinterpret_cast<float4*>(t.p)[q];
            const float4 g = reinterpret_cast<const float4*>(t.g)[q];
            float4 m = reinterpret_cast<float4*>(t.m)[q];
            float4 v = reinterpret_cast<float4*>(t.v)[q];
            upd(p.x, g.x, m.x, v.x);
            upd(p.y, g.y, m.y, v.y);
            upd(p.z, g.z, m.z, v.z);
            upd(p.w, g.w, m.w, v.w);
            reinterpret_cast<float4*>(t.p)[q] = p;
            reinterpret_cast<float4*>(t.m)[q] = m;
            reinterpret_cast<float4*>(t.v)[q] = v;
        }
        for (long long e = (q1 << 2) + threadIdx.x; e < e1; e += 256) upd(t.p[e], t.g[e], t.m[e], t.v[e]);
    } else {
        for (long long e = e0 + threadIdx.x; e < e1; e += 256) upd(t.p[e], t.g[e], t.m[e], t.v[e]);
    }
}

extern "C" int ctsi_adamw_chunk_elems(void) { return OPT_CHUNK; }

// tensors / groups / chunks: device tables as laid out above (the host builds them: optim.py); nchunks blocks.
extern "C" int ctsi_adamw_multi(const void* tensors, const void* groups, const void* chunks, int nchunks, void* stream) {
    CTSI_CHECK_ARG(tensors && groups && chunks && nchunks >= 0, "ctsi_adamw_multi: bad arguments");
    if (nchunks == 0) return CTSI_OK;
    hipLaunchKernelGGL(adamw_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                       (const CtsiOptTensor*)tensors, (const CtsiOptGroup*)groups, (const int2*)chunks);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// dst[i] = scale * src[i] for a table of fp32 segments {src, dst, n, scale}: every small fp32 operand of a program (biases,
// GroupNorm gamma / beta, the time-embedding matrices and their row-concatenations, scaled bias slices) refreshed from the
// parameters in ONE launch instead of one copy each.  One block per 4096-element piece: table2 = {segment, first element}.
struct CtsiCopySeg {
    const float* src;
    float* dst;
    long long n;
    float scale;
    int pad;
};
__global__ void __launch_bounds__(256)
copy_scale_multi_kernel(const CtsiCopySeg* __restrict__ segs, const int2* __restrict__ pieces) {
    const int2 pc = pieces[blockIdx.x];
    const CtsiCopySeg s = segs[pc.x];
    const long long e0 = (long long)pc.y * 4096;
    long long e1 = e0 + 4096;
    if (e1 > s.n) e1 = s.n;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) s.dst[e] = s.scale * s.src[e];
}
extern "C" int ctsi_copy_scale_multi(const void* segs, const void* pieces, int npieces, void* stream) {
    CTSI_CHECK_ARG(segs && pieces && npieces >= 0, "ctsi_copy_scale_multi: bad arguments");
    if (npieces == 0) return CTSI_OK;
    hipLaunchKernelGGL(copy_scale_multi_kernel, dim3((unsigned)npieces), dim3(256), 0, (hipStream_t)stream,
                       (const CtsiCopySeg*)segs, (const int2*)pieces);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// ---- the rest of the device-side optimizer step: EMA of the weights and global-norm clipping ---------
// Each of these is one more streaming pass over the parameter set, so each either is a launch of its own in the shape of the
// ones above (a tensor table + the same 64 Ki-element chunk table; block b owns chunk b; float4 where every pointer of the row
// is 16-byte aligned, scalars otherwise) or rides inside the update launch (adamw_ema_multi_kernel).

// ema = ema + w (p - ema), w = 1 - decay: torch's lerp_ for w < 0.5.  ONE spelling, shared by the stand-alone launch and the
// fused step, so the two produce the same bits.
__device__ __forceinline__ float ema_lerp(float ema, float p, float w) { return fmaf(w, p - ema, ema); }

struct CtsiEmaTensor {       // 32 bytes
    float* ema;
    const float* p;
    long long numel;
    int group;
    int pad;
};
__global__ void __launch_bounds__(256)
ema_multi_kernel(const CtsiEmaTensor* __restrict__ tensors, const float* __restrict__ weights /* w per group */,
                 const int2* __restrict__ chunks) {
    const int2 ck = chunks[blockIdx.x];
    const CtsiEmaTensor t = tensors[ck.x];
    const float w = weights[t.group];
    const long long e0 = (long long)ck.y * 4;
    long long e1 = e0 + OPT_CHUNK;
    if (e1 > t.numel) e1 = t.numel;
    long long es = e0;                                       // first element of the scalar part
    if ((((unsigned long long)t.ema | (unsigned long long)t.p) & 15ull) == 0) {
        const long long q0 = e0 >> 2, q1 = e1 >> 2;
        for (long long q = q0 + threadIdx.x; q < q1; q += 256) {
            float4 a = reinterpret_cast<float4*>(t.ema)[q];
            const float4 p = reinterpret_cast<const float4*>(t.p)[q];
            a.x = ema_lerp(a.x, p.x, w);
            a.y = ema_lerp(a.y, p.y, w);
            a.z = ema_lerp(a.z, p.z, w);
            a.w = ema_lerp(a.w, p.w, w);
            reinterpret_cast<float4*>(t.ema)[q] = a;
        }
        es = q1 << 2;
    }
    for (long long e = es + threadIdx.x; e < e1; e += 256) t.ema[e] = ema_lerp(t.ema[e], t.p[e], w);
}

// tensors[i] = { float* ema; const float* p; long long numel; int group; int pad }, weights[group] = (float)(1 - decay).
extern "C" int ctsi_ema_multi(const void* tensors, const void* weights, const void* chunks, int nchunks, void* stream) {
    CTSI_CHECK_ARG(tensors && weights && chunks && nchunks >= 0, "ctsi_ema_multi: bad arguments");
    if (nchunks == 0) return CTSI_OK;
    hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                       (const CtsiEmaTensor*)tensors, (const float*)weights, (const int2*)chunks);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// a <-> b, value for value (EMAWeights.applied(): the averaged weights go into the model and the raw ones into the shadows,
// and back; the addresses stay, so pointer tables and captured graphs stay valid).
struct CtsiSwapPair {        // 32 bytes
    float* a;
    float* b;
    long long numel;
    long long pad;
};
__global__ void __launch_bounds__(256)
swap_multi_kernel(const CtsiSwapPair* __restrict__ pairs, const int2* __restrict__ chunks) {
    const int2 ck = chunks[blockIdx.x];
    const CtsiSwapPair t = pairs[ck.x];
    const long long e0 = (long long)ck.y * 4;
    long long e1 = e0 + OPT_CHUNK;
    if (e1 > t.numel) e1 = t.numel;
    long long es = e0;
    if ((((unsigned long long)t.a | (unsigned long long)t.b) & 15ull) == 0) {
        const long long q0 = e0 >> 2, q1 = e1 >> 2;
        for (long long q = q0 + threadIdx.x; q < q1; q += 256) {
            const float4 a = reinterpret_cast<float4*>(t.a)[q];
            const float4 b = reinterpret_cast<float4*>(t.b)[q];
            reinterpret_cast<float4*>(t.a)[q] = b;
            reinterpret_cast<float4*>(t.b)[q] = a;
        }
        es = q1 << 2;
    }
    for (long long e = es + threadIdx.x; e < e1; e += 256) {
        const float a = t.a[e], b = t.b[e];
        t.a[e] = b;
        t.b[e] = a;
    }
}

// pairs[i] = { float* a; float* b; long long numel; long long pad }: the two tensors of a row must not overlap.
extern "C" int ctsi_swap_multi(const void* pairs, const void* chunks, int nchunks, void* stream) {
    CTSI_CHECK_ARG(pairs && chunks && nchunks >= 0, "ctsi_swap_multi: bad arguments");
    if (nchunks == 0) return CTSI_OK;
    hipLaunchKernelGGL(swap_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                       (const CtsiSwapPair*)pairs, (const int2*)chunks);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// Global L2 norm of a set of gradients, for torch.nn.utils.clip_grad_norm_'s coefficient.  Pass 1: block b squares and sums
// its chunk in fp64 (as the loss kernels and ctsi_slice_metrics accumulate) and writes partials[b]; pass 2: ONE block adds the
// partials in a fixed order.  No atomics anywhere, so the result is the same bits on every run.
struct CtsiNormTensor {      // 24 bytes
    float* g;                // (ctsi_grad_scale_multi writes through it; the norm pass only reads)
    long long numel;
    float scale;             // the gradient counts as scale * g (1 / loss-scale when the caller has not unscaled; 1 otherwise)
    int pad;
};
__device__ __forceinline__ double block_sum_f64(double s, double* red /* [4] in LDS */) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];                // (same order in every thread)
}
__global__ void __launch_bounds__(256)
grad_norm_partial_kernel(const CtsiNormTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                         double* __restrict__ partials) {
    __shared__ double red[4];
    const int2 ck = chunks[blockIdx.x];
    const CtsiNormTensor t = tensors[ck.x];
    const double sc = (double)t.scale;
    const long long e0 = (long long)ck.y * 4;
    long long e1 = e0 + OPT_CHUNK;
    if (e1 > t.numel) e1 = t.numel;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    long long es = e0;
    if (((unsigned long long)t.g & 15ull) == 0) {
        const long long q0 = e0 >> 2, q1 = e1 >> 2;
        for (long long q = q0 + threadIdx.x; q < q1; q += 256) {
            const float4 g = reinterpret_cast<const float4*>(t.g)[q];
            const double x = sc * (double)g.x, y = sc * (double)g.y, z = sc * (double)g.z, w = sc * (double)g.w;
            s0 += x * x;
            s1 += y * y;
            s2 += z * z;
            s3 += w * w;
        }
        es = q1 << 2;
    }
    for (long long e = es + threadIdx.x; e < e1; e += 256) {
        const double x = sc * (double)t.g[e];
        s0 += x * x;
    }
    const double s = block_sum_f64((s0 + s1) + (s2 + s3), red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
__global__ void __launch_bounds__(256)
grad_norm_finalize_kernel(const double* __restrict__ partials, int n, float max_norm, float* __restrict__ out) {
    __shared__ double part[256];
    // thread t adds its contiguous run of partials in index order, thread 0 then adds the 256 runs in index order
    const int per = (n + 255) / 256;
    const int i0 = threadIdx.x * per;
    const int i1 = i0 + per < n ? i0 + per : n;
    double s = 0.0;
    for (int i = i0; i < i1; ++i) s += partials[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < 256; ++i) tot += part[i];
        const float total_norm = (float)sqrt(tot);
        // torch: clip_coef = max_norm / (total_norm + 1e-6) in fp32, clamped at 1.0; a NaN stays a NaN (clamp keeps it)
        const float c = max_norm / (total_norm + 1e-6f);
        out[0] = total_norm;
        out[1] = c > 1.0f ? 1.0f : c;
    }
}

// tensors[i] = { float* grad; long long numel; float scale; int pad }; partials: nchunks doubles.
extern "C" int ctsi_grad_norm_multi(const void* tensors, const void* chunks, int nchunks, double* partials, void* stream) {
    CTSI_CHECK_ARG(tensors && chunks && partials && nchunks >= 0, "ctsi_grad_norm_multi: bad arguments");
    if (nchunks == 0) return CTSI_OK;
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                       (const CtsiNormTensor*)tensors, (const int2*)chunks, partials);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// out = { float total_norm; float clip_coef = min(1, max_norm / (total_norm + 1e-6)) } from the partials of the pass above.
extern "C" int ctsi_grad_norm_finalize(const double* partials, int nchunks, float max_norm, float* out, void* stream) {
    CTSI_CHECK_ARG(partials && out && nchunks >= 0, "ctsi_grad_norm_finalize: bad arguments");
    if (nchunks == 0) return CTSI_OK;
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nchunks, max_norm, out);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// g *= *dev_scale in place over the table of the norm pass: the rewrite of the gradients that the stand-alone
// clip_grad_norm_ owes its caller (the fused step never does it: it reads the coefficient instead).  A coefficient of exactly
// 1 (nothing to clip) leaves the memory alone.
__global__ void __launch_bounds__(256)
grad_scale_multi_kernel(const CtsiNormTensor* __restrict__ tensors, const int2* __restrict__ chunks,
                        const float* __restrict__ dev_scale) {
    const float c = *dev_scale;
    if (c == 1.0f) return;
    const int2 ck = chunks[blockIdx.x];
    const CtsiNormTensor t = tensors[ck.x];
    const long long e0 = (long long)ck.y * 4;
    long long e1 = e0 + OPT_CHUNK;
    if (e1 > t.numel) e1 = t.numel;
    long long es = e0;
    if (((unsigned long long)t.g & 15ull) == 0) {
        const long long q0 = e0 >> 2, q1 = e1 >> 2;
        for (long long q = q0 + threadIdx.x; q < q1; q += 256) {
            float4 g = reinterpret_cast<float4*>(t.g)[q];
            g.x *= c;
            g.y *= c;
            g.z *= c;
            g.w *= c;
            reinterpret_cast<float4*>(t.g)[q] = g;
        }
        es = q1 << 2;
    }
    for (long long e = es + threadIdx.x; e < e1; e += 256) t.g[e] *= c;
}
extern "C" int ctsi_grad_scale_multi(const void* tensors, const void* chunks, int nchunks, const float* dev_scale, void* stream) {
    CTSI_CHECK_ARG(tensors && chunks && dev_scale && nchunks >= 0, "ctsi_grad_scale_multi: bad arguments");
    if (nchunks == 0) return CTSI_OK;
    hipLaunchKernelGGL(grad_scale_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                       (const CtsiNormTensor*)tensors, (const int2*)chunks, dev_scale);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}

// adamw_multi_kernel's update (its `upd` is the specification: the lines below are a copy) plus, per launch, a gradient scale
// read from device memory (the clip coefficient of the norm pass: no host round trip, no rewrite of the gradients) and, per
// tensor, a shadow updated from the NEW parameter while it is still in registers (8 more bytes per element instead of a second
// 12-byte pass).  Its tensor row is wider than CtsiOptTensor; the old row and the old entry point stay as they are.
struct CtsiOptEmaTensor {    // 64 bytes
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema;              // NULL: this tensor has no shadow
    long long numel;
    int group;               // row of the CtsiOptGroup table
    int ema_group;           // index into the ema weight row
    long long pad;
};
__global__ void __launch_bounds__(256)
adamw_ema_multi_kernel(const CtsiOptEmaTensor* __restrict__ tensors, const CtsiOptGroup* __restrict__ groups,
                       const int2* __restrict__ chunks, const float* __restrict__ dev_grad_scale,
                       const float* __restrict__ ema_weights) {
    const int2 ck = chunks[blockIdx.x];
    const CtsiOptEmaTensor t = tensors[ck.x];
    CtsiOptGroup h = groups[t.group];
    if (dev_grad_scale) h.grad_scale *= *dev_grad_scale;     // once per block
    float* const ema = ema_weights ? t.ema : nullptr;
    const float w = ema ? ema_weights[t.ema_group] : 0.0f;
    const long long e0 = (long long)ck.y * 4;
    long long e1 = e0 + OPT_CHUNK;
    if (e1 > t.numel) e1 = t.numel;
    auto upd = [&](float& p, float g, float& m, float& v) {
        g *= h.grad_scale;
        if (h.maximize) g = -g;
        if (h.decoupled) p *= h.decay; else g = g + h.weight_decay * p;
        m = m + h.one_m_b1 * (g - m);
        const float vb = v * h.beta2;
        const float gg = g * g;
        v = vb + h.one_m_b2 * gg;
        const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
        const float r = m / denom;
        p = p - h.step_size * r;
    };
    const bool vec = ((((unsigned long long)t.p | (unsigned long long)t.g | (unsigned long long)t.m | (unsigned long long)t.v |
                        (unsigned long long)ema) & 15ull) == 0);
    // The loops that call upd are adamw_multi_kernel's, statement for statement: the compiler chooses where a * b + c becomes an
    // fma per loop body, and the bit-identity with that kernel rests on it choosing alike.  So the scalar loops stay free of the
    // shadow (it follows in a loop of its own: the same thread re-reads the few elements it has just written).
    long long es = e0;                                       // first element of the scalar part
    if (vec) {
        const long long q0 = e0 >> 2, q1 = e1 >> 2;          // whole float4 groups (e0 is a multiple of 4)
        for (long long q = q0 + threadIdx.x; q < q1; q += 256) {
            float4 p = reinterpret_cast<float4*>(t.p)[q];
            const float4 g = reinterpret_cast<const float4*>(t.g)[q];
            float4 m = reinterpret_cast<float4*>(t.m)[q];
            float4 v = reinterpret_cast<float4*>(t.v)[q];
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ema) a = reinterpret_cast<float4*>(ema)[q];
            upd(p.x, g.x, m.x, v.x);
            upd(p.y, g.y, m.y, v.y);
            upd(p.z, g.z, m.z, v.z);
            upd(p.w, g.w, m.w, v.w);
            reinterpret_cast<float4*>(t.p)[q] = p;
            reinterpret_cast<float4*>(t.m)[q] = m;
            reinterpret_cast<float4*>(t.v)[q] = v;
            if (ema) {
                a.x = ema_lerp(a.x, p.x, w);
                a.y = ema_lerp(a.y, p.y, w);
                a.z = ema_lerp(a.z, p.z, w);
                a.w = ema_lerp(a.w, p.w, w);
                reinterpret_cast<float4*>(ema)[q] = a;
            }
        }
        es = q1 << 2;
        for (long long e = es + threadIdx.x; e < e1; e += 256) upd(t.p[e], t.g[e], t.m[e], t.v[e]);
    } else {
        for (long long e = e0 + threadIdx.x; e < e1; e += 256) upd(t.p[e], t.g[e], t.m[e], t.v[e]);
    }
    if (ema)
        for (long long e = es + threadIdx.x; e < e1; e += 256) ema[e] = ema_lerp(ema[e], t.p[e], w);
}

// tensors[i] = { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; float* ema (or NULL); long long numel;
// int group; int ema_group; long long pad }; groups / chunks as for ctsi_adamw_multi.  dev_grad_scale (nullable): ONE device
// float multiplied into every group's grad_scale; ema_weights (nullable: then no shadow is touched): (float)(1 - decay) per
// ema group.  With both NULL the parameters and moments come out as ctsi_adamw_multi's, bit for bit.
extern "C" int ctsi_adamw_ema_multi(const void* tensors, const void* groups, const void* chunks, int nchunks,
                                    const float* dev_grad_scale, const float* ema_weights, void* stream) {
    CTSI_CHECK_ARG(tensors && groups && chunks && nchunks >= 0, "ctsi_adamw_ema_multi: bad arguments");
    if (nchunks == 0) return CTSI_OK;
    hipLaunchKernelGGL(adamw_ema_multi_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                       (const CtsiOptEmaTensor*)tensors, (const CtsiOptGroup*)groups, (const int2*)chunks, dev_grad_scale,
                       ema_weights);
    CTSI_LAUNCH_CHECK();
    return CTSI_OK;
}
