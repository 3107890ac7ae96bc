"""Torch restatement of the ResBlock3D options (UNet3D(use_scale_shift_norm=, dropout=)) and of the U-Net / training forward
that use them.

The oracle's own functions are used unedited: `resblock_options()` swaps `oracle.ref_ops.unet_resblock` for the duration of a
call (as tests/attn_restatement.py swaps `temporal_attention`), so `R.unet_forward`, `R.ddim_sample`, `R.training_loss`, ...
evaluate the block below.  The block reads its mode from the state dict: a `time_mlp.1.weight` of 2C rows is the scale-shift
form silu(gn(h) * (1 + s) + b) with s, b = e.chunk(2, dim=1) (scale first), C rows the additive form silu(gn(h)) + e.

`masks`: optional dict of per-layer keep masks for dropout on conv2's input, ResBlock module name -> a (B, C, D, H, W) tensor of
0 / 1 or a callable(shape) returning one; a layer without an entry is not dropped.  A name matches with or without the prefix
the oracle walks the state dict with ('down_blocks.0.0.0' matches 'unet.down_blocks.0.0.0').  Kept values are multiplied by `inv`.

`form` selects deliberately WRONG evaluations of a 2C-wide block, for the tests' "a kernel that ignored the modulation cannot
pass" assertions: 'additive' (the first C values used as a bias after the activation), 'noscale' (s = 0), 'swapped' (the halves
exchanged).

`pass_fwd64` / `pass_bwd64` are the middle pass alone and its backward in float64 on NDHWC operands, written from the formulas
of DESIGN section 21.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle import ref_ops as R

F64 = torch.float64
FORMS = ("right", "additive", "noscale", "swapped")


def _lookup(masks, p):
    if not masks:
        return None
    for key, m in masks.items():
        if p == key or p.endswith("." + key):
            return m
    return None


def _b(v):
    return v[:, :, None, None, None]


def make_resblock(masks=None, inv: float = 1.0, form: str = "right"):
    assert form in FORMS

    def unet_resblock(sd, p: str, x, temb):
        cout = sd[p + ".conv1.conv.weight"].shape[0]
        res = R.conv3d(sd, p + ".residual_conv", x) if (p + ".residual_conv.weight") in sd else x
        h = R.conv3d(sd, p + ".conv1.conv", x, padding=1)
        h = R.gn(sd, p + ".conv1.norm", h, R.conv_block_groups(cout))
        e = F.linear(F.silu(temb), sd[p + ".time_mlp.1.weight"], sd[p + ".time_mlp.1.bias"])
        if e.shape[1] == 2 * cout:
            s, b = e.chunk(2, dim=1)
            if form == "right":
                y = F.silu(h * (1 + _b(s)) + _b(b))
            elif form == "additive":
                y = F.silu(h) + _b(s)
            elif form == "noscale":
                y = F.silu(h + _b(b))
            else:
                y = F.silu(h * (1 + _b(b)) + _b(s))
        else:
            assert e.shape[1] == cout
            y = F.silu(h) + _b(e)
        m = _lookup(masks, p)
        if m is not None:
            if callable(m):
                m = m(tuple(y.shape))
            y = y * m.to(device=y.device, dtype=y.dtype) * inv
        h = R.conv3d(sd, p + ".conv2.0", y, padding=1)
        h = R.gn(sd, p + ".conv2.1", h, R.group_count(cout))
        return F.silu(h + res)

    return unet_resblock


@contextlib.contextmanager
def resblock_options(masks=None, inv: float = 1.0, form: str = "right"):
    saved = R.unet_resblock
    R.unet_resblock = make_resblock(masks, inv, form)
    try:
        yield
    finally:
        R.unet_resblock = saved


def unet_forward(sd, cfg, x, t, c, prefix: str = "", masks=None, inv: float = 1.0, form: str = "right"):
    with resblock_options(masks, inv, form):
        return R.unet_forward(sd, cfg, x, t, c, prefix)


def training_loss(sd, cfg, z0, cond, t, noise, mask=None, prefix: str = "unet.", masks=None, inv: float = 1.0):
    with resblock_options(masks, inv):
        return R.training_loss(sd, cfg, z0, cond, t, noise, mask, prefix)


# ---- the middle pass alone, float64, NDHWC ------------------------------------------------------------------------------
def _silu(z):
    return z * torch.sigmoid(z)


def _silu_grad(z):
    sg = torch.sigmoid(z)
    return sg * (1 + z * (1 - sg))


def _stats(x, sums, groups, eps):
    """xhat and rstd (per channel, broadcastable) from the fp64 (sum, sumsq) slot the kernels read."""
    n, d, h, w, c = x.shape
    cpg = c // groups
    cnt = float(cpg * d * h * w)
    sm = sums.to(F64).reshape(n, groups, 2)
    m = sm[..., 0] / cnt
    var = (sm[..., 1] / cnt - m * m).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    mc = m.repeat_interleave(cpg, 1)[:, None, None, None, :]
    rc = rstd.repeat_interleave(cpg, 1)[:, None, None, None, :]
    return (x.to(F64) - mc) * rc, rc


def group_sums(x, groups):
    """(n, groups, 2) float64 (sum, sumsq) of an NDHWC tensor: what ctsi_gn_finalize hands the pass."""
    n, d, h, w, c = x.shape
    xg = x.to(F64).reshape(n, d * h * w, groups, c // groups)
    return torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], dim=-1)


def pass_fwd64(x, sums, gamma, beta, row, groups, eps, film, keep=None, inv=1.0, form="right"):
    """x: (n, d, h, w, c); row: (n, 2c) = (s | b) when film else (n, c) = e; keep: (n, d, h, w, c) of 0 / 1 or None."""
    c = x.shape[-1]
    xh, _ = _stats(x, sums, groups, eps)
    hh = xh * gamma.to(F64) + beta.to(F64)
    r = row.to(F64)[:, None, None, None, :]
    if film:
        s, b = r[..., :c], r[..., c:2 * c]
        if form == "right":
            y = _silu(hh * (1 + s) + b)
        elif form == "additive":
            y = _silu(hh) + s
        elif form == "noscale":
            y = _silu(hh + b)
        else:
            y = _silu(hh * (1 + b) + s)
    else:
        y = _silu(hh) + r[..., :c]
    if keep is not None:
        y = y * keep.to(F64) * inv
    return y


def pass_bwd64(x, dy, sums, gamma, beta, row, groups, eps, film, keep=None, inv=1.0):
    """The backward of pass_fwd64 from the formulas: dict(dx, dgamma, dbeta, dxsum, drow) with drow = (d_s | d_b) or d_e."""
    n, d, h, w, c = x.shape
    cpg = c // groups
    cnt = float(cpg * d * h * w)
    gam, bet = gamma.to(F64), beta.to(F64)
    xh, rc = _stats(x, sums, groups, eps)
    hh = xh * gam + bet
    r = row.to(F64)[:, None, None, None, :]
    ga = dy.to(F64)
    if keep is not None:
        ga = ga * keep.to(F64) * inv
    if film:
        s1, b = 1 + r[..., :c], r[..., c:2 * c]
        gu = ga * _silu_grad(hh * s1 + b)
    else:
        s1 = torch.ones_like(r[..., :c])
        gu = ga * _silu_grad(hh)
    G = gam * s1                                                       # (n, 1, 1, 1, c): the per-sample effective weight
    sg = gu.sum((1, 2, 3))                                             # (n, c)  sum_vox gu
    sgx = (gu * xh).sum((1, 2, 3))                                     # (n, c)  sum_vox gu * xhat
    S1 = (G * gu).reshape(n, -1, groups, cpg).sum((1, 3)) / cnt
    S2 = (G * gu * xh).reshape(n, -1, groups, cpg).sum((1, 3)) / cnt
    e1 = S1.repeat_interleave(cpg, 1)[:, None, None, None, :]
    e2 = S2.repeat_interleave(cpg, 1)[:, None, None, None, :]
    dx = rc * (G * gu - e1 - xh * e2)
    s1n = s1.reshape(n, c)
    out = dict(dx=dx, dgamma=(s1n * sgx).sum(0), dbeta=(s1n * sg).sum(0), dxsum=dx.sum((0, 1, 2, 3)))
    out["drow"] = torch.cat([gam * sgx + bet * sg, sg], dim=1) if film else ga.sum((1, 2, 3))
    return out
