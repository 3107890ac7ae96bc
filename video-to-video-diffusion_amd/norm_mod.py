"""The ResBlock3D options of UNet3D(use_scale_shift_norm=, dropout=) on the engine (csrc/norm_act.hip, csrc/norm_bwd.hip): the
launches that replace the default middle pass of a ResBlock -- the GroupNorm pass that produces conv2's input -- when a block
asks for them, and the dropout state they read.  The default pass (ctsi_gn_apply / ctsi_gn_apply_f32 / ctsi_gn_bwd) is emitted
by the engines themselves, as ever; `Program.gn_apply` and `TrainProgram.t_gn` come here only with `film` or `drop` set.

  additive      y = drop( silu(gn(x)) + e )               e: the block's C columns of the time rows
  scale-shift   y = drop( silu(gn(x) * (1 + s) + b) )     (s | b): its 2C columns, scale first

drop(v) = v * keep * inv.  keep is a pure function of (seed, layer, element): one Philox4x32-10 call per 8 channels of a voxel,
so the backward regenerates the mask instead of storing it.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .lib import CtsiError


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def check_dropout(p) -> float:
    """Validate a dropout probability: a real number in [0, 1); raises ValueError otherwise."""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not (0.0 <= float(p) < 1.0):
        raise ValueError(f"dropout must be a number in [0, 1), got {p!r}")
    return float(p)


def dropout_threshold(p) -> int:
    """The 16-bit keep threshold of a dropout probability: floor(p * 65536); an element is dropped iff its Philox lane is below
    it, so the probability actually applied is thr / 65536 and 0 means no dropout (the default kernels)."""
    return int(check_dropout(p) * 65536.0)


def dropout_active(model) -> bool:
    """Whether a training forward of `model` drops: its `dropout` attribute (validated here, read at every forward) has a
    threshold > 0 AND the module is in training mode.  False selects the default launches (ctsi_gn_apply / ctsi_gn_bwd in
    additive mode) and draws no seed."""
    return dropout_threshold(getattr(model, "dropout", 0.0)) > 0 and bool(getattr(model, "training", False))


class DropoutState:
    """What the dropout launches of one train program read at launch time: the 16-bit keep threshold thr = floor(p * 65536)
    (an element is kept iff its Philox lane >= thr), the scale inv = 65536 / (65536 - thr) as one fp32 constant, and the
    device buffer holding the 64-bit seed of the current forward -- it stays in place until that forward's backward has run
    (the rule 'backward before the next forward of the same shape' guarantees it)."""

    def __init__(self, seed_buf: torch.Tensor):
        self.seed = seed_buf          # int64 (1,), persistent
        self.thr, self.inv = 0, 1.0
        self.seed_value = 0

    def set(self, p: float, seed: int):
        self.thr = dropout_threshold(p)
        self.inv = 65536.0 / (65536.0 - self.thr)
        self.seed_value = int(seed) & 0xFFFFFFFFFFFFFFFF

    def upload(self):
        """The seed of the next forward into the device buffer (on the current stream)."""
        sv = self.seed_value
        self.seed.copy_(torch.tensor([sv - (1 << 64) if sv >= (1 << 63) else sv], dtype=torch.int64))

    def launch_args(self):
        return self.thr, self.inv, _ptr(self.seed)


def _drop_args(drop):
    """(state, layer_id) or None -> (callable returning (thr, inv, seed pointer) at launch time, state, layer_id)."""
    if drop is None:
        return (lambda: (0, 1.0, None)), None, 0
    state, layer_id = drop
    return state.launch_args, state, int(layer_id)


def emit_gn_apply_mod(prog, *, xp, yp, slot, gp, bp, n, c, d, h, w, d_stat, groups, eps, tbp, tbias_stride, stp, film, drop,
                      record: dict):
    """bf16: ctsi_gn_apply_mod in place of ctsi_gn_apply.  `record`: the fields of the default pass's audit record."""
    lib, sptr = prog.lib, prog.ctx.sptr
    args, state, layer_id = _drop_args(drop)

    def run():
        thr, inv, seedp = args()
        lib.gn_apply_mod(xp, yp, C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), gp, bp, n, c, d, h, w, d_stat, groups, eps, 1,
                         tbp, tbias_stride, stp, None, 0, int(film), thr, inv, seedp, layer_id, sptr)

    prog._emit(run, "gn.apply_mod", nbytes=2 * 2.0 * n * c * d * h * w,
               audit=dict(record, kind="gn_apply_mod", film=bool(film), drop=state, layer_id=layer_id))


def emit_gn_apply_mod_f32(prog, *, xp, yp, slot, gp, bp, n, c, d, h, w, groups, eps, tbp, tbias_stride, stp, record: dict):
    """fp32 activations: ctsi_gn_apply_mod_f32 (scale-shift only: inference never drops)."""
    lib, sptr = prog.lib, prog.ctx.sptr

    def run():
        lib.gn_apply_mod_f32(xp, yp, C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), gp, bp, n, c, d, h, w, d, groups, eps, 1,
                             tbp, tbias_stride, stp, None, 0, 1, sptr)

    prog._emit(run, "gn.apply_mod", nbytes=2 * 4.0 * n * c * d * h * w,
               audit=dict(record, kind="gn_apply_mod", f32=True, film=True, drop=None, layer_id=0))


def emit_gn_bwd_mod(prog, x, gy, slot: int, gn, gamma, beta, tb_off: int, film: bool, drop, dxsum: Optional[torch.Tensor]):
    """Backward of the pass (ctsi_gn_bwd_mod) for a train program: dx, dgamma, dbeta, the conv-bias hand-off, and (d_s | d_b) --
    d_e in additive mode -- into the block's columns of d_tbias, so the stacked linear_bwd of the time embedding needs no change."""
    lib, sptr = prog.lib, prog.ctx.sptr
    n, c, d, h, w = x.n, x.c, x.d, x.h, x.w
    groups, eps = gn.num_groups, float(gn.eps)
    prog._need["gn"] = max(prog._need["gn"], 4 * lib.gn_bwd_mod_workspace_floats(n, c, d, h, w, groups))
    if x.grad is not None:
        raise CtsiError("internal: a normalised tensor has a second consumer")
    x.grad = prog.act_like(x)
    dgam, dbet = prog.grad_buf(gn.weight), prog.grad_buf(gn.bias)
    xp, gyp, gp, bp, dxp, dgp, dbp = x.ip, gy.ip, _ptr(gamma), _ptr(beta), x.grad.ip, _ptr(dgam), _ptr(dbet)
    tbp = C.c_void_p(prog.tbias.data_ptr() + 4 * tb_off)
    dtp = C.c_void_p(prog.d_tbias.data_ptr() + 4 * tb_off)
    tstride = prog.total_out
    dxsp = _ptr(dxsum)
    args, state, layer_id = _drop_args(drop)

    def run():
        thr, inv, seedp = args()
        lib.gn_bwd_mod(xp, gyp, C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), gp, bp, n, c, d, h, w, groups, eps, tbp, tstride,
                       int(film), thr, inv, seedp, layer_id, dxp, prog._ws_ptr("gn"), dgp, dbp, dtp, tstride, dxsp, sptr)

    nsum = n * groups * 2
    width = 2 * c if film else c
    prog._emit(run, "gn.bwd_mod", audit=dict(
        kind="gn_bwd_mod", x=x, dy=gy, sums=lambda: prog._gn_sums[slot:slot + nsum], gamma=gamma, beta=beta, groups=groups,
        eps=eps, film=bool(film), drop=state, layer_id=layer_id, tbias=prog.tbias[:, tb_off:tb_off + width], dx=x.grad,
        dgamma=dgam, dbeta=dbet, dxsum=dxsum, dtbias=prog.d_tbias[:, tb_off:tb_off + width]))
