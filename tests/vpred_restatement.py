"""Float64 restatement of v-prediction, the specification the v-prediction tests hold the engine to:

    v     = sqrt(abar) eps - sqrt(1 - abar) z_0                 (the training target)
    eps   = sqrt(abar) v + sqrt(1 - abar) z_t                   (the conversion; z_t the network's input)
    z_0   = sqrt(abar) z_t - sqrt(1 - abar) v
    w     = min(snr, 5) / (snr + 1),  snr = abar / (1 - abar + 1e-8)          (Min-SNR-5 on a v target)

and the analytic Gaussian data model of tests/test_gpu_cfg.py, x_0 ~ N(MU + K c, SD^2) per element, with its exact eps*,
x_0* and v* = sqrt(abar) eps* - sqrt(1 - abar) x_0*.  Plain torch / numpy in float64 on whatever device the inputs live; no
engine code."""
import math

import numpy as np
import torch

MU, SD, K = 0.5, 1.0, 0.3
U24 = 2.0 ** -24


def _b(x, like):
    """A per-sample (n,) coefficient broadcast over `like`."""
    x = torch.as_tensor(x, dtype=torch.float64, device=like.device)
    return x.reshape(-1, *([1] * (like.dim() - 1))) if x.dim() else x


def convert(out, z, rows, hist=None):
    """a out + b0 z + b1 hist, float64; rows: (n, >= 3) per-sample {a, b0, b1} or one row for all."""
    rows = torch.as_tensor(rows, dtype=torch.float64)
    rows = rows.reshape(1, -1) if rows.dim() == 1 else rows
    o, zz = out.double(), z.double()
    e = _b(rows[:, 0], o) * o + _b(rows[:, 1], o) * zz
    if hist is not None:
        e = e + _b(rows[:, 2], o) * hist.double()
    return e


def convert_magnitude(out, z, rows, hist=None):
    """|a out| + |b0 z| + |b1 hist|: what the fp32 roundings of the conversion are relative to."""
    rows = torch.as_tensor(rows, dtype=torch.float64)
    rows = rows.reshape(1, -1) if rows.dim() == 1 else rows
    o = out.double()
    m = (_b(rows[:, 0], o) * o).abs() + (_b(rows[:, 1], o) * z.double()).abs()
    if hist is not None:
        m = m + (_b(rows[:, 2], o) * hist.double()).abs()
    return m


def vp_rows(alphas_cumprod, t_desc):
    """{sqrt(abar_t), sqrt(1 - abar_t), 0} per integer timestep, float64."""
    ab = alphas_cumprod.detach().double().cpu()[torch.as_tensor([int(t) for t in t_desc])]
    return torch.stack([ab.sqrt(), (1 - ab).sqrt(), torch.zeros_like(ab)], dim=1)


def heun_rows(sigmas, order, gammas):
    """The conversion rows of an EDM run from its schedule alone (sigmas ending in 0, per-step churn gammas), float64:
    {alpha, beta, 0} at sigma_hat for predictor / Euler / final rows, {alpha', beta' c4, beta' c5} at sigma_{i+1} for
    corrector rows, c4 = a(sigma_hat) sigma_{i+1} / (sigma_hat a(sigma_{i+1})), c5 = (1 - sigma_{i+1} / sigma_hat) /
    a(sigma_{i+1}), a(s) = sqrt(1 + s^2), alpha = 1 / a(s), beta = s alpha."""
    a = lambda s: math.sqrt(1.0 + s * s)
    rows = []
    for i in range(len(sigmas) - 1):
        sh, s1 = float(sigmas[i]) * (1.0 + float(gammas[i])), float(sigmas[i + 1])
        rows.append([1.0 / a(sh), sh / a(sh), 0.0])
        if order == 2 and s1 > 0.0:
            c4, c5 = a(sh) * s1 / sh / a(s1), (1.0 - s1 / sh) / a(s1)
            rows.append([1.0 / a(s1), s1 / a(s1) * c4, s1 / a(s1) * c5])
    return torch.tensor(rows, dtype=torch.float64)


def v_target(sqrt_ab, sqrt_1mab, z0, noise):
    """sqrt(abar) noise - sqrt(1 - abar) z_0 with per-sample coefficients, float64."""
    return _b(sqrt_ab, z0) * noise.double() - _b(sqrt_1mab, z0) * z0.double()


def min_snr_weight_v(alphas_cumprod, t):
    ab = alphas_cumprod.detach().double().cpu()[t.cpu()]
    snr = ab / (1 - ab + 1e-8)
    return torch.clamp(snr, max=5.0) / (snr + 1.0)


# ---- the analytic model -------------------------------------------------------------------------------------------------
def analytic(alpha, sigma, z, c):
    """(eps*, x0*, v*) of the data model at VP coefficients (alpha, sigma), alpha^2 + sigma^2 = 1, float64."""
    z, mean = z.double(), MU + K * c.double()
    eps = sigma * (z - alpha * mean) / (alpha * alpha * SD * SD + sigma * sigma)
    x0 = (z - sigma * eps) / alpha
    return eps, x0, alpha * eps - sigma * x0


def analytic_callables(alphas_cumprod, device):
    """model(z, t, c) callables on integer timesteps: (eps*, v*), float64 inside, fp32 out."""
    ac = alphas_cumprod.double().to(device)

    def parts(z, t, c):
        ab = ac[t].view(-1, 1, 1, 1, 1)
        return analytic(ab.sqrt(), (1 - ab).sqrt(), z, c)

    return (lambda z, t, c: parts(z, t, c)[0].float()), (lambda z, t, c: parts(z, t, c)[2].float())


def analytic_callables_edm(log_sigma_table, device):
    """The same on the (fractional) timesteps of the EDM sampler: sigma(t) log-linear in the table, alpha = 1 / sqrt(1 +
    sigma^2)."""
    ls = torch.as_tensor(np.asarray(log_sigma_table), dtype=torch.float64).to(device)

    def parts(z, t, c):
        t = t.double().clamp(0, len(ls) - 1)
        k = t.floor().long().clamp(max=len(ls) - 2)
        s = torch.exp(ls[k] + (t - k) * (ls[k + 1] - ls[k])).view(-1, 1, 1, 1, 1)
        al = 1.0 / (1 + s * s).sqrt()
        return analytic(al, s * al, z, c)

    return (lambda z, t, c: parts(z, t, c)[0].float()), (lambda z, t, c: parts(z, t, c)[2].float())
