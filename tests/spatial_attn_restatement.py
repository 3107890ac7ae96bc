"""Torch restatement of SpatialAttention -- y = x + proj_out(softmax(q k^T / sqrt(hd)) v) over the h * w positions of each
(sample, depth slice, head) -- and of the U-Net / training forward with such blocks.

The oracle's walk of the stages has no slot for the new modules, so `unet_forward` here walks the stages itself, built from
`oracle.ref_ops`'s own functions (looked up at call time: `tests.attn_restatement.softmax_attention()` still swaps the temporal
block).  `cfg` is the oracle's dict plus `spatial_attention_levels`.

For the core alone the float64 functions of tests/attn_restatement.py (`core_fwd64`, `core_bwd64`) are reused on tensors whose
sequence axis is the plane: `split_plane` / `split_qkv_plane` move between them and the engine's NDHWC tensors.
`spatial_unet()` lets the oracle's own training / sampling functions run on the walk here.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle import ref_ops as R


def spatial_attention(sd, p: str, x, heads: int):
    b, c, t, hh, ww = x.shape
    hd = c // heads
    xn = R.gn(sd, p + ".norm", x, R.group_count(c))
    qkv = R.conv3d(sd, p + ".qkv", xn)
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]

    def tokens(u):  # 'b (head c) t h w -> b t head (h w) c'
        return u.reshape(b, heads, hd, t, hh * ww).permute(0, 3, 1, 4, 2)

    q, k, v = tokens(q), tokens(k), tokens(v)
    attn = F.softmax(torch.einsum('bthqc,bthkc->bthqk', q, k) * (hd ** -0.5), dim=-1)
    out = torch.einsum('bthqk,bthkc->bthqc', attn, v)
    out = out.permute(0, 2, 4, 1, 3).reshape(b, c, t, hh, ww)
    return R.conv3d(sd, p + ".proj_out", out) + x


def unet_forward(sd, cfg: dict, x, t, c, prefix: str = ""):
    """oracle.ref_ops.unet_forward with a SpatialAttention appended to every stage whose level is listed (after the ResBlock3D
    and the TemporalAttention) and `mid_attn_spatial` after `mid_attn` when the deepest level is."""
    P = prefix
    mc, nrb = cfg["model_channels"], cfg["num_res_blocks"]
    mult, att, heads = list(cfg["channel_mult"]), list(cfg["attention_levels"]), cfg["num_heads"]
    sp = list(cfg.get("spatial_attention_levels", ()))
    levels = len(mult)

    def stage(p, h, lvl, temb):
        h = R.unet_resblock(sd, p + ".0", h, temb)
        k = 1
        if lvl in att:
            h = R.temporal_attention(sd, f"{p}.{k}", h, heads)
            k += 1
        if lvl in sp:
            h = spatial_attention(sd, f"{p}.{k}", h, heads)
        return h

    temb = R.time_embedding(sd, P + "time_embed", t, mc)
    h = R.conv3d(sd, P + "conv_in", torch.cat([x, c], dim=1), padding=1)
    skips = []
    for lvl in range(levels):
        for b in range(nrb):
            h = stage(f"{P}down_blocks.{lvl}.{b}", h, lvl, temb)
        skips.append(h)
        if lvl < levels - 1:
            h = R.conv3d(sd, f"{P}down_samples.{lvl}.conv", h, stride=(1, 2, 2), padding=(1, 1, 1))
    h = R.unet_resblock(sd, P + "mid_block1", h, temb)
    h = R.temporal_attention(sd, P + "mid_attn", h, heads)
    if levels - 1 in sp:
        h = spatial_attention(sd, P + "mid_attn_spatial", h, heads)
    h = R.unet_resblock(sd, P + "mid_block2", h, temb)
    for lvl in range(levels):
        src = levels - 1 - lvl
        for b in range(nrb + 1):
            if b == 0:
                h = torch.cat([h, skips.pop()], dim=1)
            h = stage(f"{P}up_blocks.{lvl}.{b}", h, src, temb)
        if lvl < levels - 1:
            h = R.conv_transpose_122(h, sd[f"{P}up_samples.{lvl}.conv.weight"], sd[f"{P}up_samples.{lvl}.conv.bias"])
    h = F.silu(R.gn(sd, P + "conv_out.0", h, R.group_count(h.shape[1])))
    return R.conv3d(sd, P + "conv_out.2", h, padding=1)


def training_loss(sd, cfg, z0, cond, t, noise, prefix: str = "unet."):
    """oracle.ref_ops.training_loss (no mask) on the walk above."""
    bufs = {k[len("diffusion."):]: v for k, v in sd.items() if k.startswith("diffusion.")}
    B = z0.shape[0]
    pred = unet_forward(sd, cfg, R.q_sample(bufs, z0, t, noise), t, cond, prefix)
    ac = bufs["alphas_cumprod"][t]
    snr = ac / (1 - ac + 1e-8)
    w = torch.clamp(snr, max=5.0) / (snr + 1e-8)
    per = F.mse_loss(pred, noise, reduction="none").reshape(B, -1).mean(dim=1)
    return (per * w).mean()


# ---- the engine's NDHWC tensors <-> (n, d, heads, N, hd) -------------------------------------------------------------------
def split_plane(t, heads: int):
    """NDHWC (n, d, h, w, c) -> (n, d, heads, h * w, hd)."""
    n, d, h, w, c = t.shape
    return t.reshape(n, d, h * w, heads, c // heads).permute(0, 1, 3, 2, 4)


def split_qkv_plane(qkv, heads: int):
    c = qkv.shape[-1] // 3
    return tuple(split_plane(qkv[..., i * c:(i + 1) * c], heads) for i in range(3))


@contextlib.contextmanager
def spatial_unet():
    """Swap `oracle.ref_ops.unet_forward` for the walk above for the duration of a call, so that the oracle's own
    `training_loss`, `model_training_forward`, ... evaluate a U-Net with spatial blocks (the levels travel in `cfg`)."""
    saved = R.unet_forward
    R.unet_forward = unet_forward
    try:
        yield
    finally:
        R.unet_forward = saved
