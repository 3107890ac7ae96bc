"""Float64 restatement of the x0-form sampler updates and the zero-terminal-SNR schedule, the
specification the x0-form tests hold the engine to.  Plain torch / math in float64; no engine code.

    rescale (Lin et al. 2024, Algorithm 1):  s = sqrt(abar),  s <- (s - s_T) s_0 / (s_0 - s_T),  abar = s^2,
                                             alpha_t = abar_t / abar_{t-1},  beta = 1 - alpha
    kernel row {alpha, sigma, a, b, c, s, clip, 0}:
        X  = clamp(nan_to_num(alpha z - sigma v), -clip, clip)       (clip = 0: no clamp)
        z' = a z + b X + c hist + s noise,   hist <- X
    rows, with alpha, sigma at t and alpha', sigma' at the next timestep (1, 0 after the last):
        ddim   a = sigma'/sigma, b = alpha' - alpha a, s = eta sqrt((1 - abar')/(1 - abar) (1 - abar/abar')), clip 10
        ddpm   a = posterior_mean_coef2, b = posterior_mean_coef1, s = [t != 0] exp(logvar / 2), clip 1
        dpmpp  DPM-Solver++(2M) in data prediction: h = lambda' - lambda, a = sigma'/sigma, b = alpha' (1 - e^-h) (1 + 1/2r),
               c = -alpha' (1 - e^-h) / 2r, r = h_prev / h (first step / order 1: b = alpha' (1 - e^-h), c = 0; last: 0, 1, 0)
and a division-free form of the analytic Gaussian data model of tests/vpred_restatement.py (x_0 ~ N(MU + K c, SD^2)):
        x0* = (alpha SD^2 z + sigma^2 mean) / D,  eps* = sigma (z - alpha mean) / D,  D = alpha^2 SD^2 + sigma^2,
        v* = alpha eps* - sigma x0*."""
import math

import torch

from tests.vpred_restatement import K, MU, SD

F64 = torch.float64
BUFFERS = ("betas", "alphas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
           "sqrt_one_minus_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1",
           "posterior_mean_coef2")


# ---- the schedule ---------------------------------------------------------------------------------------------------------
def rescale(alphas_cumprod):
    """The ten buffers of the rescaled schedule from the fp32 `alphas_cumprod`, float64 (name -> tensor)."""
    s = alphas_cumprod.detach().to(F64).cpu().sqrt()
    s0, sT = s[0].clone(), s[-1].clone()
    s = (s - sT) * s0 / (s0 - sT)
    abar = s * s
    prev = torch.cat([torch.ones(1, dtype=F64), abar[:-1]])
    alpha = abar / prev
    beta = 1.0 - alpha
    var = beta * (1.0 - prev) / (1.0 - abar)
    return dict(betas=beta, alphas=alpha, alphas_cumprod=abar, alphas_cumprod_prev=prev, sqrt_alphas_cumprod=abar.sqrt(),
                sqrt_one_minus_alphas_cumprod=(1.0 - abar).sqrt(), posterior_variance=var,
                posterior_log_variance_clipped=var.clamp(min=1e-20).log(),
                posterior_mean_coef1=beta * prev.sqrt() / (1.0 - abar),
                posterior_mean_coef2=(1.0 - prev) * alpha.sqrt() / (1.0 - abar))


# ---- the row tables -------------------------------------------------------------------------------------------------------
def _abar(g, t_desc):
    return [float(g.alphas_cumprod.detach().to(F64).cpu()[int(t)]) for t in t_desc]


def rows(g, kind, t_desc, eta=0.0, order=2):
    """(E, 8) float64 rows of `kind` on the diffusion object `g` (its fp32 buffers widened)."""
    ab = _abar(g, t_desc)
    n = len(ab)
    out = torch.zeros(n, 8, dtype=F64)
    al = [math.sqrt(x) for x in ab]
    sg = [math.sqrt(1.0 - x) for x in ab]
    lam_prev_h = None
    for i in range(n):
        last = i == n - 1
        al_n, sg_n, ab_n = (1.0, 0.0, 1.0) if last else (al[i + 1], sg[i + 1], ab[i + 1])
        out[i, 0], out[i, 1] = al[i], sg[i]
        if kind == "ddim":
            a = sg_n / sg[i]
            out[i, 2], out[i, 3] = a, al_n - al[i] * a
            if eta > 0:
                out[i, 5] = eta * math.sqrt((1.0 - ab_n) / (1.0 - ab[i]) * (1.0 - ab[i] / ab_n))
            out[i, 6] = 10.0
        elif kind == "ddpm":
            t = int(t_desc[i])
            buf = lambda name: float(getattr(g, name).detach().to(F64).cpu()[t])
            out[i, 2], out[i, 3] = buf("posterior_mean_coef2"), buf("posterior_mean_coef1")
            out[i, 5] = 0.0 if t == 0 else math.exp(0.5 * buf("posterior_log_variance_clipped"))
            out[i, 6] = 1.0
        elif kind == "dpmpp":
            out[i, 6] = 10.0
            if last:
                out[i, 2:5] = torch.tensor([0.0, 1.0, 0.0], dtype=F64)
                continue
            lam = lambda a_, s_: (math.log(a_) if a_ > 0 else -math.inf) - math.log(s_)
            h = lam(al_n, sg_n) - lam(al[i], sg[i])                # +inf from abar = 0
            phi = 1.0 if math.isinf(h) else -math.expm1(-h)
            out[i, 2] = sg_n / sg[i]
            if order == 1 or lam_prev_h is None:
                out[i, 3] = al_n * phi
            else:
                half_inv_r = 0.0 if math.isinf(lam_prev_h) else 0.5 * h / lam_prev_h
                out[i, 3] = al_n * phi * (1.0 + half_inv_r)
                out[i, 4] = -al_n * phi * half_inv_r
            lam_prev_h = h
        else:
            raise ValueError(kind)
    return out


# ---- the kernel ------------------------------------------------------------------------------------------------------------
def nan_to_num(x):
    return torch.nan_to_num(x, nan=0.0, posinf=1.0, neginf=-1.0)


def kernel(z, v, row, hist=None, noise=None, dtype=F64):
    """One ctsi_x0_step on same-layout tensors: (X, z', |alpha z| + |sigma v|, |a z| + |b X| + |c h| + |s n|) in `dtype`
    (float64: the reference; float32: the same arithmetic in torch fp32, the yardstick of the chain tests).  v is sanitised
    first, as the kernel does; hist / noise enter only where the row's coefficient is not 0."""
    r = torch.as_tensor(row).to(dtype)
    z, v = z.to(dtype), nan_to_num(v.to(dtype))
    al, sg, a, b, c, s, clip = (r[k] for k in range(7))
    x = nan_to_num(al * z - sg * v)
    if float(clip) > 0:
        x = x.clamp(-float(clip), float(clip))
    mag_x = (al * z).abs() + (sg * v).abs()
    zn = a * z + b * x
    mag = (a * z).abs() + (b * x).abs()
    if hist is not None and float(c) != 0:
        zn = zn + c * hist.to(dtype)
        mag = mag + (c * hist.to(dtype)).abs()
    if noise is not None and float(s) != 0:
        zn = zn + s * noise.to(dtype)
        mag = mag + (s * noise.to(dtype)).abs()
    return x, zn, mag_x, mag


def chain(table, z0, model, t_desc, noises=None, dtype=F64, trajectory=None):
    """The sampling loop on a row table: z <- kernel(z, model(z, t), row_i) with hist = the previous X and noise_i = noises[i]
    where the row has s != 0.  `model(z, t)` returns v in any dtype."""
    z = z0.to(dtype)
    hist = torch.zeros_like(z)
    for i, t in enumerate(t_desc):
        v = model(z, int(t))
        nz = noises[i] if (noises is not None and float(table[i, 5]) != 0) else None
        hist, z, _, _ = kernel(z, v, table[i], hist, nz, dtype)
        if trajectory is not None:
            trajectory.append(z.clone())
    return z


# ---- the analytic model, without a division by alpha ------------------------------------------------------------------------
def analytic(alpha, sigma, z, c):
    """(eps*, x0*, v*) at VP coefficients (alpha, sigma), alpha^2 + sigma^2 = 1, float64; finite at alpha = 0."""
    z, mean = z.to(F64), MU + K * c.to(F64)
    den = alpha * alpha * SD * SD + sigma * sigma
    x0 = (alpha * SD * SD * z + sigma * sigma * mean) / den
    eps = sigma * (z - alpha * mean) / den
    return eps, x0, alpha * eps - sigma * x0


def v_model(alphas_cumprod, cond):
    """model(z, t) -> v* in float64 for the restated chains (`cond` on the host)."""
    ac = alphas_cumprod.detach().to(F64).cpu()

    def model(z, t):
        return analytic(ac[t].sqrt(), (1 - ac[t]).sqrt(), z, cond)[2]
    return model


def analytic_callables(alphas_cumprod, device):
    """model(z, t, c) callables on integer timesteps: (eps*, v*), float64 inside, fp32 out (for the generic-callable loop)."""
    ac = alphas_cumprod.detach().to(F64).to(device)

    def parts(z, t, c):
        ab = ac[t].view(-1, 1, 1, 1, 1)
        return analytic(ab.sqrt(), (1 - ab).sqrt(), z, c)

    return (lambda z, t, c: parts(z, t, c)[0].float()), (lambda z, t, c: parts(z, t, c)[2].float())
