"""Float64 restatement of measurement guidance, independent of the package's code: which evaluations are
guided, kappa per sampler from alphas_cumprod, the three device passes of csrc/measure_guide.hip, and one guided evaluation
through the float64 oracle decoder.  Tensors are torch float64 on the CPU unless said otherwise."""
import math

import numpy as np
import torch

from oracle import ref_ops as R


def guided_evaluations(E, scale, start, every):
    if scale == 0:
        return ()
    first = math.ceil(start * (E - 1))
    out, e = [], E - 1
    while e >= first:
        out.append(e)
        e -= every
    return tuple(reversed(out))


def kappa(alphas_cumprod, kind, t_desc, betas=None):
    """The weight of the data prediction in the update, float64.  ddim: z' = sqrt(abar') z0 + sqrt(1 - abar') eps;
    ddpm: the posterior mean's beta_t sqrt(abar_{t-1}) / (1 - abar_t), on the schedule's own `betas` (a cosine schedule clips
    them, and 1 - abar_t / abar_{t-1} taken from fp32 values of abar cancels); dpmpp (2M, data prediction): with lambda = log(alpha /
    sigma), h = lambda' - lambda, z' = (sigma'/sigma) z - alpha' expm1(-h) D, D = (1 + 1/2r) x0 - (1/2r) x0_prev, r = h_prev/h
    (first order at step 0; the last step, to abar' = 1, returns x0)."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    t = [int(v) for v in t_desc]
    n = len(t)
    out = np.zeros(n)
    if kind == "ddim":
        for i in range(n):
            out[i] = math.sqrt(ac[t[i + 1]]) if i + 1 < n else 1.0
    elif kind == "ddpm":
        for i in range(n):
            prev = ac[t[i] - 1] if t[i] > 0 else 1.0
            out[i] = float(betas[t[i]]) * math.sqrt(prev) / (1.0 - ac[t[i]])
    elif kind == "dpmpp":
        lam = [0.5 * (math.log(ac[v]) - math.log1p(-ac[v])) for v in t]
        for i in range(n):
            if i == n - 1:
                out[i] = 1.0
                continue
            h = lam[i + 1] - lam[i]
            b = -math.sqrt(ac[t[i + 1]]) * math.expm1(-h)
            if i > 0:
                b *= 1.0 + 0.5 * h / (lam[i] - lam[i - 1])
            out[i] = b
    else:
        raise ValueError(kind)
    return out


def nan_to_num(v):
    return torch.nan_to_num(v, nan=0.0, posinf=1.0, neginf=-1.0)


def z0(z_t, eps, alpha, sigma, mode, clip):
    """ctsi_guide_z0 on NCDHW float64 tensors; alpha, sigma, clip: the fp32 row values as Python floats."""
    eps = nan_to_num(eps)
    x = (z_t - sigma * eps) / alpha if mode == 0 else alpha * z_t - sigma * eps
    x = nan_to_num(x)
    return x.clamp(-clip, clip) if clip > 0 else x


def residual(W, x, y):
    """r = y - W x along depth: W (d_in, d_out), x (n, c, d_out, h, w), y (n, c, d_in, h, w)."""
    return y - torch.einsum("kj,ncjhw->nckhw", W.to(x.dtype), x)


def residual_adj(W, x, y):
    """(g_x, sum r^2 per sample) of ctsi_depth_residual_adj in the dtype of x."""
    r = residual(W, x, y)
    return -torch.einsum("kj,nckhw->ncjhw", W.to(x.dtype), r), r.pow(2).sum(dim=(1, 2, 3, 4))


def sequential_sumsq(W32, x, y):
    """sum r^2 per sample in float64 from fp32 values, the depth sum taken ascending, one exact product at a time (the order
    of the kernel's fp64 residual; the order of the outer sum is the kernel's own and costs a few 1e-16 relative)."""
    W = torch.from_numpy(np.asarray(W32)).double()
    xd, acc = x.double().cpu(), torch.zeros(y.shape, dtype=torch.float64)
    for j in range(W.shape[1]):
        acc = acc + W[:, j].view(1, 1, -1, 1, 1) * xd[:, :, j:j + 1]
    return (y.double().cpu() - acc).pow(2).sum(dim=(1, 2, 3, 4))


def apply_factor(coef, sumsq_b, normalize):
    """The fp32 factor c of ctsi_guide_apply for one sample (None: the sample is left alone)."""
    if not normalize:
        return float(np.float32(coef))
    if not sumsq_b > 0.0:
        return None
    return float(np.float32(float(np.float32(coef)) * (1.0 / math.sqrt(sumsq_b))))


def decoder_gradient(sd, sf, W, z, y, autocast=False, prefix=""):
    """(g = grad_z 1/2 ||y - W D(z)||^2, ||r||_2 per sample) through the oracle decoder under torch autograd: float64 by
    default, bf16 autocast (fp32 tensors) for the yardstick's second term.  z (n, L, d, h, w), y (n, c, d_in, H, W)."""
    dt = torch.float32 if autocast else torch.float64
    sdd = {k: v.detach().to(dt) for k, v in sd.items() if k.startswith(prefix + "decoder.")}
    zz = z.detach().to(dt).clone().requires_grad_(True)
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            x = R.vae_decode(sdd, zz, sf, prefix)
        x = x.float()
    else:
        x = R.vae_decode(sdd, zz, sf, prefix)
    r = residual(W.to(dt), x, y.to(dt))
    (0.5 * r.pow(2).sum()).backward()
    return zz.grad.detach().double(), r.detach().double().pow(2).sum(dim=(1, 2, 3, 4)).sqrt()


def residual_norm(sd, sf, W, z, y, prefix=""):
    """||y - W D(z)||_2 per sample, float64 oracle decoder."""
    sdd = {k: v.detach().double() for k, v in sd.items() if k.startswith(prefix + "decoder.")}
    with torch.no_grad():
        x = R.vae_decode(sdd, z.detach().double(), sf, prefix)
    return residual(W.double(), x, y.double()).pow(2).sum(dim=(1, 2, 3, 4)).sqrt()


def delta_z0(g, rnorm, scale, normalize):
    """dz0 = -zeta g / ||r|| per sample ('residual'; 0 where ||r|| == 0) or -zeta g ('none')."""
    if normalize == "none":
        return -scale * g
    f = torch.where(rnorm > 0, 1.0 / rnorm.clamp_min(1e-300), torch.zeros_like(rnorm))
    return -scale * g * f.view(-1, 1, 1, 1, 1)
