"""How TemporalAttention is evaluated (DESIGN sections 3.2 and 19).

'fast' / 'exact'  the reference's einsum 'bhqk,bhvc->bhqc' as written: every query receives the depth SUM of V, the q and k
                  thirds of `qkv` have no effect (engine.Program.attention, csrc/attention.hip).
'softmax'         true attention over depth, y = x + proj_out(softmax(q k^T / sqrt(hd)) v) per (b, h, w) location
                  (csrc/attention_core.hip).  This module holds its launches: the inference / training-forward block and the
                  training backward.

The mode is `UNet3D.attention_mode`; the modules and the state dict are the same in all three."""
from __future__ import annotations

from .lib import CtsiError

ATTENTION_MODES = ("fast", "exact", "softmax")


def check_attention_mode(mode) -> str:
    """Validate an attention_mode value; anything unknown is a ValueError, not the fast path."""
    if not isinstance(mode, str) or mode not in ATTENTION_MODES:
        raise ValueError(f"attention_mode must be one of {ATTENTION_MODES}, got {mode!r}")
    return mode


def emit_softmax_attention(prog, m, x, save: bool = False):
    """Append the softmax-mode block to `prog` (an engine.Program): seven launches --
        gn.colsum, gn.finalize     GroupNorm statistics of x
        gn.apply                   xn = gn(x), no SiLU
        attn.qkv                   one 1x1x1 conv C -> 3C
        attn.core                  A = softmax(q k^T / sqrt(hd)) v over depth (ctsi_attn_core)
        attn.proj                  the proj_out 1x1x1 conv
        attn.residual_add          y += x in place (ctsi_add_bf16: no bf16 conv epilogue adds a plain tensor -- the fused
                                   tail adds a GroupNorm)
    Returns (y, saved); `save` keeps what the backward reads (xn, qkv, A) instead of handing the buffers back to the pool."""
    lib, sptr = prog.lib, prog.ctx.sptr
    n, c, d, h, w = x.n, x.c, x.d, x.h, x.w
    heads = m.num_heads
    if prog.shard is not None:
        raise CtsiError("softmax-mode attention needs every key on one rank; use the fast mode when sharding")
    slot = prog.gn_finalize(x, m.norm.num_groups, prog.gn_colsum(x))
    xn = prog.gn_apply(x, slot, m.norm, silu_pre=False)
    qkv, _ = prog.conv("attn.qkv", lambda: m.qkv.weight, lambda: m.qkv.bias, xn, None, k=(1, 1, 1), p=(0, 0, 0),
                       cout=3 * c)
    a = prog.act(n, c, d, h, w, halo=0)
    qp, ap = qkv.ip, a.ip

    def run_core():
        lib.attn_core(qp, ap, n, c, d, h, w, heads, sptr)

    fl = 4.0 * n * h * w * d * d * c          # q k^T and p v: 2 d^2 hd each per (position, head)
    prog.flops += fl
    prog._emit(run_core, "attn.core", fl, "attn_core_mfma", nbytes=8.0 * n * c * d * h * w,
               audit=dict(kind="attn_core", qkv=qkv, heads=heads, out=a))
    y, _ = prog.conv("attn.proj", lambda: m.proj_out.weight, lambda: m.proj_out.bias, a, None, k=(1, 1, 1),
                     p=(0, 0, 0), cout=c)
    yp, xp, cnt = y.ip, x.ip, n * d * h * w * c

    def run_add():
        lib.add_bf16(yp, xp, cnt, sptr)

    prog._emit(run_add, "attn.residual_add", nbytes=6.0 * cnt, audit=dict(kind="add", dst=y, src=x))
    y.dirty = False
    saved = dict(slot=slot, xn=xn, qkv=qkv, a=a)
    if not save:
        for t in (xn, qkv, a):
            prog.release(t)
    return y, saved


def emit_softmax_attention_train(prog, m, x):
    """The block on a training program (train_engine.UNetTrainProgram): the inference launches with xn = gn(x), qkv and the
    core's output A kept, and on the tape its backward -- proj_out (dW, db, dA), the core's backward (dqkv from qkv and dA, one
    launch), the whole qkv layer (dW, db over all three thirds, d xn), then the GroupNorm backward, whose `add` operand brings
    in the identity path's gradient in the same launch."""
    lib, sptr = prog.lib, prog.ctx.sptr
    n, c, d, h, w = x.n, x.c, x.d, x.h, x.w
    heads = m.num_heads
    out, sv = emit_softmax_attention(prog, m, x, save=True)
    slot, xn, qkv, a = sv["slot"], sv["xn"], sv["qkv"], sv["a"]
    gamma = prog.dev_f32(lambda: m.norm.weight)
    beta = prog.dev_f32(lambda: m.norm.bias)

    def bwd():
        gy = out.grad
        if gy is None:
            raise CtsiError("internal: no gradient reached an attention output")
        prog._conv_bwd("attn.proj", m.proj_out.weight, m.proj_out.bias, a, None, gy, False, (1, 1, 1), (1, 1),
                       (0, 0, 0), c, True)
        da = a.grad
        dqkv = prog.act(n, 3 * c, d, h, w, halo=0)
        qp, dap, dqp = qkv.ip, da.ip, dqkv.ip

        def run_core_bwd():
            lib.attn_core_bwd(qp, dap, dqp, n, c, d, h, w, heads, sptr)

        fl = 14.0 * n * h * w * d * d * c      # s^T, dp^T, dq (per query tile) and s, dp, dv, dk (per key tile): 2 d^2 hd each
        prog.flops += fl
        prog._emit(run_core_bwd, "attn.core.bwd", fl, "attn_core_bwd_mfma",
                   audit=dict(kind="attn_core_bwd", qkv=qkv, da=da, heads=heads, out=dqkv))
        prog._conv_bwd("attn.qkv", m.qkv.weight, m.qkv.bias, xn, None, dqkv, False, (1, 1, 1), (1, 1), (0, 0, 0),
                       3 * c, True)
        dxn = xn.grad
        prog._gn_bwd(x, dxn, False, slot, m.norm, gamma, beta, False, None, None, False, gy)
        for t in (da, dqkv, dxn, gy):
            prog.release(t)
        a.grad = xn.grad = out.grad = None

    prog.tape.append(bwd)
    return out
