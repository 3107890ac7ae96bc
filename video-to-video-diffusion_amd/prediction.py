"""What the U-Net's output means: 'epsilon' (the reference) or 'v_prediction', v = sqrt(abar) eps -
sqrt(1 - abar) z_0 (Salimans & Ho 2022).  The type lives on GaussianDiffusion.prediction_type; this module holds its
validation and the one launch a v-prediction step program adds, ctsi_pred_to_eps (csrc/prediction.hip)."""
from __future__ import annotations

import ctypes as C

import torch

PREDICTION_TYPES = ("epsilon", "v_prediction")


def check_prediction_type(p) -> str:
    """Validate a prediction_type value ('epsilon' | 'v_prediction'); raises ValueError otherwise."""
    if not isinstance(p, str) or p not in PREDICTION_TYPES:
        raise ValueError(f"unknown prediction_type {p!r}: expected one of {PREDICTION_TYPES}")
    return p


def add_pred_to_eps(prog):
    """Append ctsi_pred_to_eps to the step program `prog` (engine.UNetProgram.add_sampler_step, right behind the network):
    over every network row -- 2n when guided, reading the n rows of z twice -- `eps` holds v before the launch and eps
    after it, so whatever follows is the epsilon program's.  One row {a, b0, b1, 0} per evaluation in `prog.pred_rows`
    (identity rows until set_schedule writes the schedule's), selected by the device-side step counter."""
    lib, sptr = prog.lib, prog.ctx.sptr
    n, nb = prog.n, prog.nb
    per = prog.L * prog.d * prog.h * prog.w
    prog.pred_rows = prog.persistent((max(prog.max_rows // nb, 1), 4), torch.float32, zero=True)
    prog.pred_rows[:, 0] = 1.0
    ep, zp, rp, sp = (C.c_void_p(t.data_ptr()) for t in (prog.eps, prog.z, prog.pred_rows, prog.step_ptr))
    hp = C.c_void_p(0 if prog.hist is None else prog.hist.data_ptr())
    prog._emit(lambda: lib.pred_to_eps(ep, zp, hp, rp, sp, 1, nb, n, per, sptr), "pred.to_eps",
               nbytes=(12.0 if prog.hist is None else 16.0) * nb * per,
               audit=dict(kind="pred_to_eps", out=prog.eps, z=prog.z, hist=prog.hist, rows=prog.pred_rows,
                          step_ptr=prog.step_ptr, rows_per_step=1, n=nb, z_rows=n, per_sample=per))
