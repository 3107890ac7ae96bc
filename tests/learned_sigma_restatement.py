"""Float64 restatement of the learned reverse variance and the strided ancestral sampler: what
csrc/learned_sigma.hip and learned_sigma.py compute, written from the formulas of Nichol & Dhariwal 2021 ("Improved DDPM") in
torch float64, independent of the engine's code.  Tensors are NCDHW unless said otherwise.
"""
import math

import numpy as np
import torch

F64 = torch.float64
LN2 = math.log(2.0)


# ---- the respaced chain ---------------------------------------------------------------------------------------------
def respaced(alphas_cumprod, t_desc):
    """The chain on the descending timestep subset `t_desc`, per loop position j: abar, abar of the next position (1 behind
    the last), beta' = 1 - abar / abar_next, the posterior coefficients and variance of that chain, all float64."""
    ac = np.asarray(alphas_cumprod.detach().double().cpu())
    a = ac[[int(t) for t in t_desc]]
    ap = np.append(a[1:], 1.0)
    beta = 1.0 - a / ap
    post = beta * (1.0 - ap) / (1.0 - a)
    lpost = np.log(np.where(post > 0, post, 1.0))
    lpost[-1] = lpost[-2] if len(a) > 1 else math.log(1e-20)          # the last step's variance is 0: its neighbour's value
    return dict(abar=a, abar_next=ap, beta=beta, coef1=beta * np.sqrt(ap) / (1.0 - a),
                coef2=(1.0 - ap) * np.sqrt(1.0 - beta) / (1.0 - a), log_beta=np.log(beta), log_post=lpost, post=post)


def rows64(alphas_cumprod, t_desc, clip):
    """The (N, 8) rows of ctsi_ddpm_lv_step in float64; entry 6 is the fixed-small noise scale [not last] sqrt(beta~')."""
    c = respaced(alphas_cumprod, t_desc)
    n = len(t_desc)
    rows = np.zeros((n, 8))
    rows[:, 0], rows[:, 1] = np.sqrt(1.0 - c["abar"]), np.sqrt(c["abar"])
    rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5] = c["coef1"], c["coef2"], c["log_beta"], c["log_post"]
    rows[:-1, 6] = np.sqrt(c["post"][:-1])
    rows[:, 7] = 1.0 if clip else 0.0
    return torch.from_numpy(rows)


# ---- one step (any layout: elementwise) ------------------------------------------------------------------------------------
def step(z, eps, vraw, noise, row):
    """(new z, log-variance, elementwise error bound of an fp32 evaluation) of one ancestral step on the row (8 float64).

    The bound counts roundings of relative size u = 2^-24, each applied to the magnitude it acts on:
      z0   = (z - c0 eps) / c1 : product, difference and quotient -- 3 u (|z| + |c0 eps|) / c1  (the clamp adds none)
      mean = c2 z0 + c3 z      : two products and a sum, plus the inherited error of z0 -- 3 u (|c2 z0| + |c3 z|) + c2 err(z0)
      scale = c6 exp((lv - c5) / 2) = c6 exp(f (c4 - c5) / 2), f = (v + 1) / 2, with c6 = [not last] exp(c5 / 2) from the row: the
             exp argument is a sum, a difference and two products, absolute error 4 u |f (c4 - c5) / 2|, and an absolute error
             delta in the argument costs a relative delta in the scale; the device exp itself is allowed 2 ulp, the products
             c6 * exp and scale * noise and the fused sum 3 more
      out  = mean + scale noise: u |out| for the last sum
    vraw None: the scale is c6 exactly.  The log-variance returned is lv = f c4 + (1 - f) c5."""
    u = 2.0 ** -24
    c0, c1, c2, c3, c4, c5, c6, clip = (float(v) for v in row)
    z, eps = z.double(), eps.double()
    z0 = (z - c0 * eps) / c1
    e_z0 = 3 * u * (z.abs() + (c0 * eps).abs()) / c1
    if clip > 0:
        z0 = z0.clamp(-clip, clip)
    mean = c2 * z0 + c3 * z
    bound = 3 * u * ((c2 * z0).abs() + (c3 * z).abs()) + abs(c2) * e_z0
    if vraw is None:
        lv = torch.full_like(z, c5)
        e_arg = torch.zeros_like(z)
    else:
        f = (vraw.double() + 1.0) / 2.0
        lv = f * c4 + (1.0 - f) * c5
        e_arg = 4 * u * (0.5 * f * (c4 - c5)).abs()
    out = mean
    if noise is not None:
        term = c6 * torch.exp(0.5 * (lv - c5)) * noise.double()
        out = mean + term
        bound = bound + term.abs() * (e_arg + 5 * u)
    return out, lv, bound + u * out.abs()


# ---- the variational bound ---------------------------------------------------------------------------------------------
def kl_normal(mean1, logvar1, mean2, logvar2):
    """KL(N(mean1, exp(logvar1)) || N(mean2, exp(logvar2))), nats, elementwise (Improved DDPM's normal_kl)."""
    return 0.5 * (-1.0 + logvar2 - logvar1 + torch.exp(logvar1 - logvar2) + (mean1 - mean2) ** 2 * torch.exp(-logvar2))


def nll_normal(x, mean, logvar):
    """-log N(x; mean, exp(logvar)), nats, elementwise: the continuous Gaussian negative log-likelihood (the t = 0 term; the
    project's targets are continuous latents, so there is no 1/255 bin to integrate over)."""
    return 0.5 * (math.log(2.0 * math.pi) + logvar + (x - mean) ** 2 * torch.exp(-logvar))


def schedule64(g):
    """Per-timestep float64 columns from the module's registered buffers (what the engine's loss table holds)."""
    b = lambda name: getattr(g, name).detach().cpu().double()
    plv = b("posterior_log_variance_clipped").clone()
    plv[0] = plv[1]
    return dict(a=b("sqrt_alphas_cumprod"), s=b("sqrt_one_minus_alphas_cumprod"), c1=b("posterior_mean_coef1"),
                c2=b("posterior_mean_coef2"), log_beta=torch.log(b("betas")), log_post=plv)


def hybrid_terms(pred2, z0, noise, t, sched, v_pred):
    """(mse element term, bound element term in nats) of a (B, 2L, ...) prediction; autograd-friendly float64.  The bound's mean
    is detached: its gradient reaches the variance channels only."""
    B, L = z0.shape[0], z0.shape[1]
    col = lambda k: sched[k][t].view(B, 1, 1, 1, 1)
    a, s, c1, c2, lb, lp = (col(k) for k in ("a", "s", "c1", "c2", "log_beta", "log_post"))
    z0, noise = z0.double(), noise.double()
    p, v = pred2[:, :L], pred2[:, L:]
    zt = a * z0 + s * noise
    if v_pred:
        target, x0p = a * noise - s * z0, a * zt - s * p
    else:
        target, x0p = noise, (zt - s * p) / a
    mse = (p - target) ** 2
    f = (v + 1.0) / 2.0
    lv = f * lb + (1.0 - f) * lp
    mu_true = c1 * z0 + c2 * zt
    mu_model = (c1 * x0p + c2 * zt).detach()
    kl = kl_normal(mu_true, lp.expand_as(lv), mu_model, lv)
    nll = nll_normal(z0, mu_model, lv)
    t0 = (t == 0).view(B, 1, 1, 1, 1)
    return mse, torch.where(t0, nll, kl)


def hybrid_error_terms(pred2, z0, noise, t, sched, v_pred):
    """(mse term, bound term) per-element error magnitudes of an fp32 evaluation of `hybrid_terms`, float64: the roundings
    u = 2^-24 listed in tests/test_gpu_learned_sigma.py::test_hybrid_loss_forward_against_float64, each on the magnitude it acts
    on, every inherited error carried through, doubled (fused and unfused multiply-adds round differently).  `sched`: the
    columns of `schedule64`."""
    u = 2.0 ** -24
    n, Lc = z0.shape[0], z0.shape[1]
    col = lambda k: sched[k][t].view(n, 1, 1, 1, 1)
    a, s_, c1, c2, lb, lp = (col(k) for k in ("a", "s", "c1", "c2", "log_beta", "log_post"))
    z0, nz, p, vch = z0.double(), noise.double(), pred2[:, :Lc].double(), pred2[:, Lc:].double()
    zt = a * z0 + s_ * nz
    if v_pred:
        target, x0p = a * nz - s_ * z0, a * zt - s_ * p
        e_t, e_x0 = 3 * u * ((a * nz).abs() + (s_ * z0).abs()), 4 * u * ((a * zt).abs() + (s_ * p).abs())
    else:
        target, x0p = nz, (zt - s_ * p) / a
        e_t, e_x0 = torch.zeros_like(nz), 4 * u * (zt.abs() + (s_ * p).abs()) / a
    dp = p - target
    e_dp = e_t + u * dp.abs()
    mag_mse = 2 * (2 * dp.abs() * e_dp + e_dp ** 2 + u * dp ** 2)
    f = (vch + 1) / 2
    lv = f * lb + (1 - f) * lp
    e_lv = 4 * u * ((f * lb).abs() + ((1 - f) * lp).abs()) + u * lv.abs()
    inv = torch.exp(-lv)
    t0 = (t == 0).view(n, 1, 1, 1, 1)
    q = torch.where(t0, z0 - c1 * x0p - c2 * zt, c1 * (z0 - x0p))
    e_q = c1 * e_x0 + 4 * u * (z0.abs() + (c1 * x0p).abs() + (c2 * zt).abs())
    e_quad = inv * (2 * q.abs() * e_q + e_q ** 2) + q ** 2 * inv * (e_lv + 5 * u)
    ratio = torch.exp(lp - lv)
    e_kl = e_lv + u * (lv - lp).abs() + ratio * (e_lv + u * (lp - lv).abs() + 3 * u) + u * (ratio - 1).abs()
    e_nll = e_lv + u * (math.log(2 * math.pi) + lv.abs())
    parts = torch.where(t0, math.log(2 * math.pi) + lv.abs(), (lv - lp).abs() + (ratio - 1).abs()) + q ** 2 * inv
    mag_vb = 2 * (0.5 * (e_quad + torch.where(t0, e_nll, e_kl)) + 3 * u * 0.5 * parts)
    return mag_mse, mag_vb


def hybrid_sum_bounds(S, V, S_mag, V_mag, norm, norm_vb, mse=None, vb=None):
    """The bounds of the five outputs of ctsi_hybrid_loss_fwd from the per-sample float64 sums S, V and the summed error
    magnitudes S_mag, V_mag (each (B,)): dict(S_b, V_b, mse, vb, total).  u for each fp32 norm factor and the final fp32 store;
    the scalars are formed from the device's double accumulators, not from the rounded per-sample sums.  `mse`, `vb`: the float64 values of the two terms where the caller has them (else formed here)."""
    u = 2.0 ** -24
    mse = (norm * S).sum() if mse is None else mse
    vb = (norm_vb * V).sum() if vb is None else vb
    return dict(S_b=S_mag + u * S.abs(), V_b=V_mag + u * V.abs(), mse=(norm * S_mag).sum() + 2 * u * mse.abs(),
                vb=(norm_vb * V_mag).sum() + 2 * u * vb.abs(),
                total=(norm * S_mag).sum() + (norm_vb * V_mag).sum() + 2 * u * (mse + vb).abs())


def count_norm(mask, shape):
    """The batch / element normalisation of both loss terms, (B,) float64: 1 / (B L d h w) without a mask; with a (B, 1 or L, d)
    mask 1 / (total valid elements) when every sample has the same number of them, else 1 / (B valid_b) per sample.
    Returns (norm, the mask expanded to `shape`, pooled) -- pooled: the equal-count case, whose L_simple weight is the batch mean."""
    B, L, d, h, w = shape
    if mask is None:
        return torch.full((B,), 1.0 / (B * L * d * h * w), dtype=F64), torch.ones(shape, dtype=F64), False
    me = mask.double().expand(B, L, d)
    nv = me.reshape(B, -1).sum(1) * (h * w)
    full = me[:, :, :, None, None].expand(shape)
    if bool((nv == nv[0]).all()):
        return (1.0 / nv.sum()).expand(B).clone(), full, True
    return torch.where(nv > 0, 1.0 / (nv.clamp(min=1) * B), torch.zeros_like(nv)), full, False


def hybrid_loss(pred2, z0, noise, t, g, weight, mask=None, v_pred=False):
    """{'total', 'mse', 'vb'} float64 scalars: mse = sum_b weight_b cn_b sum(mask mse), vb = lambda / ln 2 sum_b cn_b sum(mask
    bound), lambda = timesteps / 1000.  `weight`: (B,) the loss weight of L_simple (with an equal-count mask: its mean)."""
    shape = tuple(z0.shape)
    cn, me, pooled = count_norm(mask, shape)
    mse, vb = hybrid_terms(pred2, z0, noise, t, schedule64(g), v_pred)
    B = shape[0]
    w = weight.double().mean().expand(B) if pooled else weight.double()
    lam = float(g.timesteps) / 1000.0
    l_mse = (w * cn * (me * mse).reshape(B, -1).sum(1)).sum()
    l_vb = (lam / LN2) * (cn * (me * vb).reshape(B, -1).sum(1)).sum()
    return dict(total=l_mse + l_vb, mse=l_mse, vb=l_vb)


# ---- the analytic model: i.i.d. N(m, s^2) data ----------------------------------------------------------------------------
def analytic_eps_coefs(abar, m, s):
    """E[eps | z_t] = k (z_t - sqrt(abar) m) with k = sqrt(1 - abar) / (abar s^2 + 1 - abar): returns (k, sqrt(abar) m)."""
    return math.sqrt(1.0 - abar) / (abar * s * s + 1.0 - abar), math.sqrt(abar) * m


def analytic_optimal_v(chain, m, s):
    """The variance channel value whose log-variance is the exact reverse variance of the respaced chain on N(m, s^2) data:
    Var(z_next | z_t) = beta' V_next / V_t with V = abar s^2 + 1 - abar; solved for v in lv = f log beta' + (1 - f) log beta~'.
    (The last position draws no noise: its v is 0.)"""
    V = chain["abar"] * s * s + 1.0 - chain["abar"]
    Vn = chain["abar_next"] * s * s + 1.0 - chain["abar_next"]
    var = chain["beta"] * Vn / V
    v = np.zeros_like(var)
    for j in range(len(var) - 1):
        f = (math.log(var[j]) - chain["log_post"][j]) / (chain["log_beta"][j] - chain["log_post"][j])
        v[j] = 2.0 * f - 1.0
    return v, var


def analytic_sample_std(chain, m, s, v=None):
    """(mean, std) of one element after the whole strided ancestral chain started from N(0, 1), without clipping, by the
    linear-Gaussian recursion: each step is z <- A z + B + sigma xi.  `v` None: the fixed-small variance beta~'."""
    mean, var = 0.0, 1.0
    n = len(chain["abar"])
    for j in range(n):
        abar = chain["abar"][j]
        k, shift = analytic_eps_coefs(abar, m, s)
        sa, sig = math.sqrt(abar), math.sqrt(1.0 - abar)
        # z0_hat = (z - sig k (z - shift)) / sa;  mean = c1 z0_hat + c2 z
        A = chain["coef1"][j] * (1.0 - sig * k) / sa + chain["coef2"][j]
        Bc = chain["coef1"][j] * sig * k * shift / sa
        if j == n - 1:
            noise_var = 0.0
        elif v is None:
            noise_var = chain["post"][j]
        else:
            f = (v[j] + 1.0) / 2.0
            noise_var = math.exp(f * chain["log_beta"][j] + (1.0 - f) * chain["log_post"][j])
        mean, var = A * mean + Bc, A * A * var + noise_var
    return mean, math.sqrt(var)
