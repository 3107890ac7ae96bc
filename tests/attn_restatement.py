"""Torch restatement of the CORRECTED TemporalAttention -- softmax(Q K^T / sqrt(hd)) V over depth, i.e. the reference's second
einsum with its intended indices ('bhqk,bhkc->bhqc') -- and of the U-Net / training forward that use it.

The oracle's own functions are used unedited: `softmax_attention()` swaps `oracle.ref_ops.temporal_attention` for the
duration of a call, so `R.unet_forward`, `R.ddim_sample`, `R.training_loss`, ... evaluate the corrected block.

Float64 functions for the core alone (`core_fwd64`, `core_bwd64`) work on (..., D, hd) tensors; `split_heads` /
`merge_heads` move between them and the engine's NDHWC tensors.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle import ref_ops as R

F64 = torch.float64


def temporal_attention_softmax(sd, p: str, x, heads: int):
    """oracle.ref_ops.temporal_attention with the keys contracted against the values."""
    b, c, t, hh, ww = x.shape
    hd = c // heads
    xn = R.gn(sd, p + ".norm", x, R.group_count(c))
    qkv = R.conv3d(sd, p + ".qkv", xn)
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]

    def tokens(u):  # 'b (head c) t h w -> (b h w) head t c'
        return u.reshape(b, heads, hd, t, hh, ww).permute(0, 4, 5, 1, 3, 2).reshape(b * hh * ww, heads, t, hd)

    q, k, v = tokens(q), tokens(k), tokens(v)
    attn = torch.einsum('bhqc,bhkc->bhqk', q, k) * (hd ** -0.5)
    attn = F.softmax(attn, dim=-1)
    out = torch.einsum('bhqk,bhkc->bhqc', attn, v)
    out = out.reshape(b, hh, ww, heads, t, hd).permute(0, 3, 5, 4, 1, 2).reshape(b, c, t, hh, ww)
    return R.conv3d(sd, p + ".proj_out", out) + x


@contextlib.contextmanager
def softmax_attention():
    saved = R.temporal_attention
    R.temporal_attention = temporal_attention_softmax
    try:
        yield
    finally:
        R.temporal_attention = saved


def unet_forward(sd, cfg, x, t, c, prefix: str = ""):
    with softmax_attention():
        return R.unet_forward(sd, cfg, x, t, c, prefix)


def training_loss(sd, cfg, z0, cond, t, noise, mask=None, prefix: str = "unet."):
    with softmax_attention():
        return R.training_loss(sd, cfg, z0, cond, t, noise, mask, prefix)


# ---- the core in float64 -------------------------------------------------------------------------------------------------
def core_fwd64(q, k, v):
    """(..., D, hd) -> (A, P): P = softmax(q k^T / sqrt(hd)), A = P v."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    s = q @ k.transpose(-1, -2) * (q.shape[-1] ** -0.5)
    p = torch.softmax(s, dim=-1)
    return p @ v, p


def core_uniform64(v):
    """What a kernel that ignored the scores would return: the mean of v over the keys, for every query."""
    v = v.to(F64)
    return v.mean(dim=-2, keepdim=True).expand_as(v)


def core_bwd64(q, k, v, da):
    """The backward formulas of the issue, written out: returns dict(dq, dk, dv, p, ds)."""
    q, k, v, da = q.to(F64), k.to(F64), v.to(F64), da.to(F64)
    sc = q.shape[-1] ** -0.5
    a, p = core_fwd64(q, k, v)
    dv = p.transpose(-1, -2) @ da
    dp = da @ v.transpose(-1, -2)
    ds = p * (dp - (da * a).sum(-1, keepdim=True))
    return dict(dq=ds @ k * sc, dk=ds.transpose(-1, -2) @ q * sc, dv=dv, p=p, ds=ds)


def split_heads(t, heads: int):
    """NDHWC (n, d, h, w, c) -> (n, h, w, heads, d, hd)."""
    n, d, h, w, c = t.shape
    return t.reshape(n, d, h, w, heads, c // heads).permute(0, 2, 3, 4, 1, 5)


def merge_heads(t):
    """(n, h, w, heads, d, hd) -> NDHWC (n, d, h, w, c)."""
    n, h, w, heads, d, hd = t.shape
    return t.permute(0, 4, 1, 2, 3, 5).reshape(n, d, h, w, heads * hd)


def split_qkv(qkv, heads: int):
    """NDHWC (n, d, h, w, 3c) -> q, k, v each (n, h, w, heads, d, hd)."""
    c = qkv.shape[-1] // 3
    return tuple(split_heads(qkv[..., i * c:(i + 1) * c], heads) for i in range(3))
