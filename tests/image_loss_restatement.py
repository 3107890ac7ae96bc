"""float64 restatements of the image-loss joints (csrc/image_loss.hip), written from the formulas and from
nothing in the engine: test infrastructure, like tests/x0_restatement.py.

  z0_pred_f64      the clean latent a training step's prediction stands for
  loss_bwd_z0_f64  the loss-head gradient with the gradient of that latent added
  rows_f64         the SNR gate of the rows that take part
All tensors are taken as they are given (fp32 values are exact in float64); nothing is rounded here."""
import torch

F64 = torch.float64


def _rows(v, ndim):
    return v.to(F64).reshape(-1, *((1,) * (ndim - 1)))


def z0_pred_f64(z0, noise, pred_ncdhw, sqrt_ac, sqrt_1mac, t, active, v_prediction):
    """z_t = a z0 + s noise;  epsilon: (z_t - s pred) / a;  v: a z_t - s pred;  inactive rows: z0.  a = sqrt_ac[t], s =
    sqrt_1mac[t] (the fp32 table values, exact in float64).  All of (n, c, d, h, w)."""
    a, s = _rows(sqrt_ac[t], z0.dim()), _rows(sqrt_1mac[t], z0.dim())
    x, ns, p = z0.to(F64), noise.to(F64), pred_ncdhw.to(F64)
    zt = a * x + s * ns
    # (an inactive row may sit at a = 0: it is never divided)
    out = a * zt - s * p if v_prediction else (zt - s * p) / torch.where(a == 0, torch.ones_like(a), a)
    return torch.where(active.reshape(-1, 1, 1, 1, 1).bool(), out, x)


def z0_coef_f64(sqrt_ac, sqrt_1mac, t, active, v_prediction):
    """d z0^ / d pred per row: -s / a (epsilon) or -s (v); 0 on inactive rows."""
    a, s = sqrt_ac[t].to(F64), sqrt_1mac[t].to(F64)
    coef = -s if v_prediction else -s / torch.where(active.bool(), a, torch.ones_like(a))
    return torch.where(active.bool(), coef, torch.zeros_like(coef))


def loss_bwd_z0_f64(pred_ncdhw, target, mask, norm, gscale, g_z0, active, coef):
    """gscale 2 norm[b] mask (pred - target) + active[b] coef[b] g_z0, (n, c, d, h, w); mask (n, c, d) or None."""
    nd = pred_ncdhw.dim()
    first = 2.0 * _rows(norm, nd) * (pred_ncdhw.to(F64) - target.to(F64)) * float(gscale)
    if mask is not None:
        first = first * mask.to(F64)[:, :, :, None, None]
    second = _rows(torch.where(active.bool(), coef.to(F64), torch.zeros_like(coef, dtype=F64)), nd) * g_z0.to(F64)
    second = torch.where(active.reshape(-1, 1, 1, 1, 1).bool(), second, torch.zeros_like(second))
    return first + second


def rows_f64(alphas_cumprod, t, min_snr):
    """abar_t / (1 - abar_t) >= min_snr, in float64 (abar_t < 1 on every schedule of the project)."""
    ab = alphas_cumprod.to(F64)[t]
    return ab / (1.0 - ab) >= float(min_snr)
