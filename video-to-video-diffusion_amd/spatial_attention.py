"""How SpatialAttention is evaluated: in-plane attention over the h * w positions of every depth slice,
    y = x + proj_out(softmax(q k^T / sqrt(hd)) v),  [q | k | v] = qkv(gn(x)),
on the flash-attention kernels of csrc/attention_plane.hip.  This module holds its launches -- the inference / training-forward
block and the training backward -- as attention.py does for the softmax mode of TemporalAttention; the engines only dispatch on
the layer's type.  The block does not depend on `UNet3D.attention_mode`, which is about the depth axis."""
from __future__ import annotations

import torch

from .lib import CtsiError

HEAD_DIMS = (8, 16, 32, 64, 128)


def spatial_attention_modules(unet):
    return [m for m in unet.modules() if type(m).__name__ == "SpatialAttention"]


def check_spatial_attention_supported(unet, precision: str = "bf16", sharded: bool = False):
    """CtsiError -- with the numbers -- for what the spatial blocks of `unet` do not run on: the fp32 / bf16x3 inference modes
    (there is no fp32 core, as for attention_mode='softmax'), depth sharding (it would be local per slice; out of scope) and a
    head dimension the kernel has no instantiation for.  A U-Net without spatial blocks passes."""
    mods = spatial_attention_modules(unet)
    if not mods:
        return
    levels = tuple(getattr(unet, "spatial_attention_levels", ()))
    if precision != "bf16":
        raise CtsiError(f"spatial_attention_levels={levels} ({len(mods)} SpatialAttention blocks) needs the bf16 engine: "
                        f"inference_precision={precision!r} has no in-plane attention core (csrc/attention_plane.hip is bf16 "
                        "only, DESIGN section 26)")
    if sharded:
        raise CtsiError(f"spatial_attention_levels={levels} ({len(mods)} SpatialAttention blocks) does not support depth "
                        "sharding (unet.depth_shard_comm): drop the communicator or build the model without spatial blocks")
    for m in mods:
        hd = m.channels // m.num_heads
        if hd not in HEAD_DIMS:
            raise CtsiError(f"SpatialAttention: head dimension {hd} (channels={m.channels} / num_heads={m.num_heads}) is not "
                            f"supported: the in-plane attention core takes {HEAD_DIMS}")


def emit_spatial_attention(prog, m, x, save: bool = False):
    """Append the block to `prog` (an engine.Program): seven launches --
        gn.colsum, gn.finalize     GroupNorm statistics of x
        gn.apply                   xn = gn(x), no SiLU
        sattn.qkv                  one 1x1x1 conv C -> 3C
        sattn.core                 A = softmax(q k^T / sqrt(hd)) v over the plane (ctsi_attn_plane)
        sattn.proj                 the proj_out 1x1x1 conv
        sattn.residual_add         y += x in place (ctsi_add_bf16)
    Returns (y, saved); `save` keeps what the backward reads (xn, qkv, A, lse) instead of handing the buffers back to the pool,
    and makes the core write lse (inference passes NULL)."""
    lib, sptr = prog.lib, prog.ctx.sptr
    n, c, d, h, w = x.n, x.c, x.d, x.h, x.w
    heads = m.num_heads
    if getattr(prog, "precision", "bf16") != "bf16":
        raise CtsiError(f"SpatialAttention needs the bf16 engine: the {prog.precision} inference mode has no in-plane attention "
                        "core (DESIGN section 26)")
    if prog.shard is not None:
        raise CtsiError("SpatialAttention does not support depth sharding (out of scope, DESIGN section 26)")
    if c % heads or c // heads not in HEAD_DIMS:
        raise CtsiError(f"SpatialAttention: head dimension {c / heads:g} (channels={c} / num_heads={heads}) is not supported: "
                        f"the in-plane attention core takes {HEAD_DIMS}")
    slot = prog.gn_finalize(x, m.norm.num_groups, prog.gn_colsum(x))
    xn = prog.gn_apply(x, slot, m.norm, silu_pre=False)
    qkv, _ = prog.conv("sattn.qkv", lambda: m.qkv.weight, lambda: m.qkv.bias, xn, None, k=(1, 1, 1), p=(0, 0, 0),
                       cout=3 * c)
    a = prog.act(n, c, d, h, w, halo=0)
    lse = prog.pool.get(n * d * heads * h * w, torch.float32) if save else None
    qp, ap = qkv.ip, a.ip
    lp = None if lse is None else lse.data_ptr()

    def run_core():
        lib.attn_plane(qp, ap, lp, n, c, d, h, w, heads, sptr)

    nq = h * w
    fl = 4.0 * n * d * nq * nq * c             # q k^T and p v: 2 N^2 hd each per (slice, head)
    prog.flops += fl
    prog._emit(run_core, "sattn.core", fl, "attn_plane_mfma", nbytes=8.0 * n * c * d * h * w,
               audit=dict(kind="attn_plane", qkv=qkv, heads=heads, out=a, lse=lse))
    y, _ = prog.conv("sattn.proj", lambda: m.proj_out.weight, lambda: m.proj_out.bias, a, None, k=(1, 1, 1),
                     p=(0, 0, 0), cout=c)
    yp, xp, cnt = y.ip, x.ip, n * d * h * w * c

    def run_add():
        lib.add_bf16(yp, xp, cnt, sptr)

    prog._emit(run_add, "sattn.residual_add", nbytes=6.0 * cnt, audit=dict(kind="add", dst=y, src=x))
    y.dirty = False
    saved = dict(slot=slot, xn=xn, qkv=qkv, a=a, lse=lse)
    if not save:
        for t in (xn, qkv, a):
            prog.release(t)
    return y, saved


def emit_spatial_attention_train(prog, m, x):
    """The block on a training program (train_engine.UNetTrainProgram): the inference launches with xn = gn(x), qkv, the core's
    output A and lse kept, and on the tape its backward -- proj_out (dW, db, dA), the core's backward (dqkv from qkv, A, lse and
    dA: one entry point, two grids), the whole qkv layer (dW, db over all three thirds, d xn), then the GroupNorm backward, whose
    `add` operand brings in the identity path's gradient in the same launch."""
    lib, sptr = prog.lib, prog.ctx.sptr
    n, c, d, h, w = x.n, x.c, x.d, x.h, x.w
    heads = m.num_heads
    out, sv = emit_spatial_attention(prog, m, x, save=True)
    slot, xn, qkv, a, lse = sv["slot"], sv["xn"], sv["qkv"], sv["a"], sv["lse"]
    gamma = prog.dev_f32(lambda: m.norm.weight)
    beta = prog.dev_f32(lambda: m.norm.bias)

    def bwd():
        gy = out.grad
        if gy is None:
            raise CtsiError("internal: no gradient reached a spatial attention output")
        prog._conv_bwd("sattn.proj", m.proj_out.weight, m.proj_out.bias, a, None, gy, False, (1, 1, 1), (1, 1),
                       (0, 0, 0), c, True)
        da = a.grad
        dqkv = prog.act(n, 3 * c, d, h, w, halo=0)
        qp, ap, dap, dqp, lp = qkv.ip, a.ip, da.ip, dqkv.ip, lse.data_ptr()

        def run_core_bwd():
            lib.attn_plane_bwd(qp, ap, dap, lp, dqp, n, c, d, h, w, heads, sptr)

        nq = h * w
        fl = 14.0 * n * d * nq * nq * c        # s^T, dp^T, dq (query-block pass) and s, dp, dv, dk (key-block pass): 2 N^2 hd each
        prog.flops += fl
        prog._emit(run_core_bwd, "sattn.core.bwd", fl, "attn_plane_bwd_mfma",
                   audit=dict(kind="attn_plane_bwd", qkv=qkv, a=a, da=da, lse=lse, heads=heads, out=dqkv))
        prog._conv_bwd("sattn.qkv", m.qkv.weight, m.qkv.bias, xn, None, dqkv, False, (1, 1, 1), (1, 1), (0, 0, 0),
                       3 * c, True)
        dxn = xn.grad
        prog._gn_bwd(x, dxn, False, slot, m.norm, gamma, beta, False, None, None, False, gy)
        for t in (da, dqkv, dxn, gy):
            prog.release(t)
        a.grad = xn.grad = out.grad = None

    prog.tape.append(bwd)
    return out
