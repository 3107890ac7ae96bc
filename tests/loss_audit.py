"""Eager audit of the perceptual-loss and decode-gradient programs, launch by launch (used by tests/test_gpu_loss_program_audit.py,
shown on the CPU by tests/test_host_loss_audit.py).

vgg_loss_engine.VGGLossProgram (the VGG-19 feature loss and LPIPS) and vae_train_engine.VAEDecodeGradProgram are built on
engine.PhasedProgram like the training programs; every launch of theirs carries an audit record.  `audit_forward` /
`audit_backward` run ops[:n_fwd] / ops[n_fwd:] one at a time, copy what a launch is about to read, run it and recompute its result
in float64 from exactly those operands, as tests/fwd_audit.py and tests/train_audit.py do.  Kinds those two modules know go to
their tables unchanged (fwd_audit.REFS, train_audit.check); the kinds below have their references here.  The comparisons, the
bound constants and the table format are the two modules' own.

An Act of the loss program holds 2 n_img images along its depth axis: the pred half first, the target half behind it.

Record kinds and what they compute:
  maxpool2_fwd        out = 2 x 2 / stride 2 max pooling (floor) of all 2 n_img images                     selection: bit for bit
  relu                x <- max(x, 0) in place, sign-bit rule (-0 -> +0)                                    selection: bit for bit
  maxpool2_bwd        gx = g at the FIRST maximum of each window in (h, w) row-major order, +0 elsewhere (an odd last row /
                      column included), over the pred half                                                selection: bit for bit
  seam.grad_z         out (fp32 NCDHW) = g (bf16 NDHWC)                                                    copy: bit for bit
  feat_loss           slab[0 .. blocks) of layer l <- fp64 partial sums of |p - t| or (p - t)^2 over `half` elements
  lpips_dist          slab[image][0 .. blocks) of tap l <- fp64 partial sums of sum_c w_c (u_c - v_c)^2 over the positions
  feat_loss_finalize  out[1 + l] = sum(slab l) / counts[l], out[0] = their average
  lpips_finalize      out[i] = sum_l sum(slab l, image i) / counts[l], out[n_img + l] = the mean over the images of that quotient
  feat_grad_relu      out = (g_in + coef gl[0] f(y - t)) [y > 0]: f = sign (loss_kind 1), 2 (.) (2), no term (0); relu 0: no mask
  lpips_grad_relu     out = (g_in + gl[image] / pos (r / (a + eps) - u (u . r) / a)) [y > 0], r = 2 w (u - v)
  dgrad               train_audit's data-gradient conv; here also where the output Act is wider than the weights' input channels
                      (the 3-channel stem's gradient in its 8-channel image): the channels past them must be zero

Bounds (each from the arithmetic of the launch, none from a measurement):
  selections, copies  bit for bit.
  partial sums        the slab's float64 sum against the float64 sum of the operands.  feat_loss: SUM_REL = 2^-21 relative, what
                      tests/test_gpu_vgg_ops.py::test_feature_distance_against_float64 holds the finalized means to (fp32 per 8
                      elements: 4 roundings of 2^-24; fp64 from there on).  lpips_dist: FWD_TOL = 1e-5 relative per image, as
                      tests/test_gpu_lpips_ops.py derives it, valid while 2 DELTA kappa + 6e-7 <= FWD_TOL with kappa^2 =
                      sum w (|u| + |v|)^2 / sum w d^2 of the launch's own operands: the row fails if they leave that range.
                      Every other element of `partials` must keep its bits.
  finalizes           from the partials the launch read, in float64: SUM_REL per output (fp64 sums, one rounding to fp32 =
                      2^-24).  `counts` must equal, bit for bit, the row computed from the tapped Acts' shapes.
  bf16 elementwise    train_audit.cmp_bf16: one bf16 ulp of float64 + BF16_FLOOR rms(ref).  Both gradient passes evaluate their
                      expression in fp32 and round once (half an ulp); the fp32 chain leaves `need` = 2 k 2^-24 sum|terms| (k
                      counted beside each use), far below the floor unless a term is much larger than the result's rms.  The
                      reference computes `need` per element from its own float64 intermediates: where need <= BF16_FLOOR rms(ref)
                      everywhere the plain bound holds (what tests/test_gpu_lpips_ops.py's header argues for its operand
                      ranges); otherwise the launch's operands are outside those ranges and `need` is added as the per-element
                      `extra` (the row's `extra` says which).
  convs               fwd_audit's conv_fwd (ReLU epilogue act = 2 included) and train_audit's dgrad, unchanged.
"""
from __future__ import annotations

import math
from typing import Iterable, Optional

import torch

from tests import fwd_audit as FA
from tests import train_audit as TA
from tests.fwd_audit import SKIP, cmp_elem, cmp_same, snapshot as fwd_snapshot
from tests.train_audit import (BF16_FLOOR, BF16_REL_L2, BF16_ULPS, F32_MAX_REL, F32_REL_L2, F64, act_ndhwc, bf16_ulp, cmp_bf16,
                               cmp_exact, cmp_f32, format_table, snapshot as train_snapshot, _row)

__all__ = ["audit_forward", "audit_backward", "format_table", "REFS", "SUM_REL", "FWD_TOL", "DELTA", "LPIPS_EPS",
           "ref_maxpool2_fwd", "ref_maxpool2_bwd", "ref_relu", "ref_feat_sum", "ref_lpips_sums", "ref_feat_grad", "ref_lpips_grad",
           "ref_feat_finalize", "ref_lpips_finalize", "tie_fraction", "cmp_rel", "cmp_same", "cmp_bf16", "cmp_exact", "cmp_f32",
           "cmp_elem", "SKIP"]

EPS32 = FA.EPS32
SUM_REL = 2.0 ** -21            # tests/test_gpu_vgg_ops.py::test_feature_distance_against_float64
FWD_TOL = 1e-5                  # tests/test_gpu_lpips_ops.py
DELTA = 8.5 * 2.0 ** -24        # tests/test_gpu_lpips_ops.py: the relative error of u and v
LPIPS_EPS = 1e-10


# ---- comparisons -----------------------------------------------------------------------------------------------------------
def cmp_rel(out: torch.Tensor, ref: torch.Tensor, tol: float) -> dict:
    """every element within `tol` of its own reference value, relatively (sums of non-negative terms: no cancellation)"""
    o, r = out.detach().to(F64).reshape(-1), ref.to(F64).reshape(-1)
    err = (o - r).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    rel = torch.where(r != 0, err / r.abs().clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    worst = float(rel.max()) if r.numel() else 0.0
    rn = float(r.norm())
    return dict(cls="rel", rel_l2=float(err.norm()) / rn if rn > 0 else worst, max_rel=worst, ulps=worst / tol, ok=worst <= tol)


# ---- float64 references (plain tensors, any device) ------------------------------------------------------------------------------
def _corners(x: torch.Tensor):
    """x (n, h, w, c) -> the four corners of every 2 x 2 window in (h, w) row-major order, each (n, h // 2, w // 2, c)"""
    ho, wo = x.shape[1] // 2, x.shape[2] // 2
    return (x[:, 0:2 * ho:2, 0:2 * wo:2], x[:, 0:2 * ho:2, 1:2 * wo:2], x[:, 1:2 * ho:2, 0:2 * wo:2], x[:, 1:2 * ho:2, 1:2 * wo:2])


def _first_max(x: torch.Tensor):
    """(the window maximum with the bits of the FIRST element that holds it, that element's index 0 .. 3)"""
    a, b, c, d = _corners(x)
    m, k = a, torch.zeros(a.shape, dtype=torch.int64, device=x.device)
    for q, v in ((1, b), (2, c), (3, d)):
        later = v > m                      # strictly greater: an equal later element does not take over (nor does a NaN)
        m, k = torch.where(later, v, m), torch.where(later, torch.full_like(k, q), k)
    return m, k


def ref_maxpool2_fwd(x: torch.Tensor) -> torch.Tensor:
    return _first_max(x)[0].contiguous()


def ref_maxpool2_bwd(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """x (n, h, w, c), g (n, h // 2, w // 2, c) -> gx (n, h, w, c) in g's dtype: g at the first maximum, +0 everywhere else"""
    ho, wo = x.shape[1] // 2, x.shape[2] // 2
    k = _first_max(x)[1]
    gx = torch.zeros(x.shape, dtype=g.dtype, device=g.device)
    zero = torch.zeros_like(g)
    for q, (r0, c0) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        gx[:, r0:2 * ho:2, c0:2 * wo:2] = torch.where(k == q, g, zero)
    return gx


def tie_fraction(x: torch.Tensor) -> float:
    """the share of windows whose maximum is non-zero and held by more than one element"""
    a, b, c, d = _corners(x.to(F64))
    win = torch.stack([a, b, c, d], -1)
    mx = win.amax(-1, keepdim=True)
    tied = ((win == mx).sum(-1) > 1) & (mx[..., 0] != 0)
    return float(tied.to(F64).mean()) if tied.numel() else 0.0


def ref_relu(x: torch.Tensor) -> torch.Tensor:
    """the kernel's rule: an element with the sign bit set becomes +0 (so -0 does too), every other keeps its bits"""
    return torch.where(torch.signbit(x), torch.zeros_like(x), x)


def ref_feat_sum(p: torch.Tensor, t: torch.Tensor, sq: int) -> torch.Tensor:
    df = p.to(F64) - t.to(F64)
    return (df * df).sum() if sq else df.abs().sum()


def _unit(y: torch.Tensor):
    a = y.pow(2).sum(-1, keepdim=True).sqrt()
    return a, y / (a + LPIPS_EPS)


def ref_lpips_sums(y: torch.Tensor, t: torch.Tensor, w: torch.Tensor):
    """y, t (n, pos, c), w (c,) -> (per-image sums over positions of sum_c w (u - v)^2, per-image kappa)"""
    y, t, w = y.to(F64), t.to(F64), w.to(F64).reshape(1, 1, -1)
    u, v = _unit(y)[1], _unit(t)[1]
    s = (w * (u - v) ** 2).sum((1, 2))
    kappa = ((w.abs() * (u.abs() + v.abs()) ** 2).sum((1, 2)) / s.abs().clamp_min(1e-300)).sqrt()
    return s, kappa


def ref_feat_grad(g: Optional[torch.Tensor], y: torch.Tensor, t: torch.Tensor, coef: float, gl: float, loss_kind: int, relu: int):
    """(reference, need) of ctsi_feat_grad_relu_bwd.  need = 2 k EPS32 (|g| + |term|), k = 4: coef -> fp32, coef gl, the product
    with y - t (exact itself: two bf16 values; 2 (.) is exact), the add."""
    y, t = y.to(F64), t.to(F64)
    g = torch.zeros_like(y) if g is None else g.to(F64)
    df = y - t
    scale = float(coef) * float(gl)
    term = {0: torch.zeros_like(y), 1: scale * torch.sign(df), 2: 2.0 * scale * df}[int(loss_kind)]
    v, need = g + term, 2.0 * 4 * EPS32 * (g.abs() + term.abs())
    if relu:
        keep = y > 0
        v, need = torch.where(keep, v, torch.zeros_like(v)), torch.where(keep, need, torch.zeros_like(need))
    return v, need


def ref_lpips_grad(g: Optional[torch.Tensor], y: torch.Tensor, t: torch.Tensor, w: torch.Tensor, gl: torch.Tensor, pos: int):
    """(reference, need) of ctsi_lpips_grad_relu_bwd; y, t, g (n, pos, c), w (c,), gl (n,).  The closed form of the kernel's
    header (checked against autograd in tests/test_host_loss_audit.py).  need, from lpips_grad_kernel with d = DELTA / EPS32 =
    8.5 roundings on ia, ib, u, v (tests/test_gpu_lpips_ops.py):
      r = w2 (u - v)           e_r  = |w2| (DELTA (|u| + |v|) + EPS32 |u - v|) + EPS32 |r|
      t1 = r ia                e_t1 = e_r ia + 9.5 EPS32 |t1|
      ur = sum u r             e_ur = sum (|u| e_r + DELTA |u r|) + 14 EPS32 sum |u r|        (8 fmas, <= 6 butterfly levels)
      proj = ur / a            e_pr = e_ur / a + 8 EPS32 |proj|                               (a: 7 roundings, the division)
      t2 = u proj              e_t2 = |u| e_pr + 9.5 EPS32 |t2|
      dy = t1 - t2             e_dy = e_t1 + e_t2 + EPS32 |dy|
      o = g + s dy             e_o  = |s| e_dy + 3 EPS32 |s dy| + EPS32 |o|                   (1 / pos, gl / pos, s dy; the add)
    doubled, as every fp32-elementwise bound of the audits."""
    y, t = y.to(F64), t.to(F64)
    n = y.shape[0]
    w2 = 2.0 * w.to(F64).reshape(1, 1, -1)
    g = torch.zeros_like(y) if g is None else g.to(F64)
    s = (gl.to(F64).reshape(n, 1, 1) / float(pos))
    a, u = _unit(y)
    v = _unit(t)[1]
    ia = 1.0 / (a + LPIPS_EPS)
    r = w2 * (u - v)
    ur = (u * r).sum(-1, keepdim=True)
    safe = a.clamp_min(1e-300)
    proj = torch.where(a > 0, ur / safe, torch.zeros_like(ur))
    t1, t2 = r * ia, u * proj
    dy = t1 - t2
    o = g + s * dy
    e_r = w2.abs() * (DELTA * (u.abs() + v.abs()) + EPS32 * (u - v).abs()) + EPS32 * r.abs()
    e_t1 = e_r * ia + 9.5 * EPS32 * t1.abs()
    e_ur = (u.abs() * e_r + DELTA * (u * r).abs()).sum(-1, keepdim=True) + 14 * EPS32 * (u * r).abs().sum(-1, keepdim=True)
    e_pr = torch.where(a > 0, e_ur / safe, torch.zeros_like(ur)) + 8 * EPS32 * proj.abs()
    e_t2 = u.abs() * e_pr + 9.5 * EPS32 * t2.abs()
    e_dy = e_t1 + e_t2 + EPS32 * dy.abs()
    need = 2.0 * (s.abs() * e_dy + 3 * EPS32 * (s * dy).abs() + EPS32 * o.abs())
    keep = y > 0
    return torch.where(keep, o, torch.zeros_like(o)), torch.where(keep, need, torch.zeros_like(need))


def ref_feat_finalize(partials: torch.Tensor, counts: torch.Tensor, blocks: int) -> torch.Tensor:
    nl = counts.numel()
    means = partials.to(F64)[:nl * blocks].view(nl, blocks).sum(1) / counts.to(F64)
    return torch.cat([means.mean().view(1), means])


def ref_lpips_finalize(partials: torch.Tensor, counts: torch.Tensor, n_img: int, blocks: int) -> torch.Tensor:
    nl = counts.numel()
    d = partials.to(F64)[:nl * n_img * blocks].view(nl, n_img, blocks).sum(2) / counts.to(F64).view(nl, 1)
    return torch.cat([d.sum(0), d.mean(1)])


# ---- checks, one function per kind ---------------------------------------------------------------------------------------------
def _images(a) -> torch.Tensor:
    """an Act of the loss program -> (images, h, w, c)"""
    return act_ndhwc(a)[0]


def _halves(x: torch.Tensor, n_img: int):
    assert x.shape[0] == 2 * n_img, (tuple(x.shape), n_img)
    return x[:n_img], x[n_img:]


def _bf16_elem(out: torch.Tensor, ref: torch.Tensor, need: torch.Tensor) -> dict:
    rms = float(ref.pow(2).mean().sqrt()) if ref.numel() else 0.0
    inside = bool((need <= BF16_FLOOR * rms).all())
    plain = cmp_bf16(out, ref)
    res = plain if inside else cmp_bf16(out, ref, extra=need)
    res["extra"] = "-" if inside else "fp32 chain"
    res["plain_ulps"] = plain["ulps"]            # the worst element against one ulp + the floor alone, for the log
    return res


def _slab_rows(rec, sn, R, lo: int, hi: int, what: str, res: dict):
    """the row of a partial-sum launch + the two that pin where it wrote: the record's slab view is partials[lo:hi], and
    everything outside it kept its bits"""
    parts, slab = rec["partials"], rec["slab"]
    placed = slab.data_ptr() == parts.data_ptr() + 8 * lo and slab.numel() == hi - lo
    keep = torch.ones(parts.numel(), dtype=torch.bool, device=parts.device)
    keep[lo:hi] = False
    where = dict(cls="exact", rel_l2=0.0 if placed else math.inf, max_rel=0.0 if placed else math.inf, ulps=float("nan"), ok=placed)
    return [R(what, parts[lo:hi], res), R("slab@", slab, where), R("others", parts[keep], cmp_same(parts[keep], sn["partials"][keep]))]


def _chk_maxpool2_fwd(rec, sn, R, ctx):
    out = _images(rec["out"])
    return [R("y", out, cmp_same(out, ref_maxpool2_fwd(sn["x"][0])))]


def _chk_relu(rec, sn, R, ctx):
    out = _images(rec["out"])
    return [R("y", out, cmp_same(out, ref_relu(sn["x"][0])))]


def _chk_maxpool2_bwd(rec, sn, R, ctx):
    out = _images(rec["out"])
    x = sn["x"][0][:rec["n_img"]]
    res = cmp_same(out, ref_maxpool2_bwd(x, sn["g"][0]))
    res["ties"] = tie_fraction(x)
    return [R("gx", out, res)]


def _chk_seam_grad_z(rec, sn, R, ctx):
    out = rec["out"]
    return [R("g_z", out, cmp_same(out, sn["g"].permute(0, 4, 1, 2, 3).to(torch.float32).contiguous()))]


def _chk_feat_loss(rec, sn, R, ctx):
    p, t = _halves(sn["x"][0], rec["n_img"])
    assert p.numel() == rec["half"], (p.numel(), rec["half"])
    b, l = rec["blocks"], rec["l"]
    got = rec["partials"][l * b:(l + 1) * b].sum()
    return _slab_rows(rec, sn, R, l * b, (l + 1) * b, "sum", cmp_rel(got, ref_feat_sum(p, t, rec["sq"]), SUM_REL))


def _chk_lpips_dist(rec, sn, R, ctx):
    n = rec["n_img"]
    p, t = _halves(sn["x"][0], n)
    c = p.shape[-1]
    assert p.numel() == rec["half"] and p.shape[1] * p.shape[2] == rec["pos"], (tuple(p.shape), rec["half"], rec["pos"])
    want, kappa = ref_lpips_sums(p.reshape(n, -1, c), t.reshape(n, -1, c), sn["head"])
    nb, l = n * rec["blocks"], rec["l"]
    got = rec["partials"][l * nb:(l + 1) * nb].view(n, rec["blocks"]).sum(1)
    res = cmp_rel(got, want, FWD_TOL)
    res["kappa"] = float(kappa.max())
    res["ok"] = res["ok"] and 2 * DELTA * res["kappa"] + 6e-7 <= FWD_TOL       # the operand range the bound is derived for
    return _slab_rows(rec, sn, R, l * nb, (l + 1) * nb, "sums", res)


def _counts(rec, per_image: bool) -> torch.Tensor:
    n = rec["n_img"]
    rows = [(a.h * a.w if per_image else n * a.h * a.w * a.c) for a in rec["taps"]]
    return torch.tensor(rows, dtype=torch.int64, device=rec["counts"].device)


def _chk_feat_loss_finalize(rec, sn, R, ctx):
    cnt = _counts(rec, False)
    return [R("counts", rec["counts"], cmp_same(rec["counts"], cnt)),
            R("out", rec["out"], cmp_rel(rec["out"], ref_feat_finalize(sn["partials"], cnt, rec["blocks"]), SUM_REL))]


def _chk_lpips_finalize(rec, sn, R, ctx):
    cnt = _counts(rec, True)
    return [R("counts", rec["counts"], cmp_same(rec["counts"], cnt)),
            R("out", rec["out"], cmp_rel(rec["out"], ref_lpips_finalize(sn["partials"], cnt, rec["n_img"], rec["blocks"]), SUM_REL))]


def _g_in(rec, sn):
    assert rec["no_g_in"] == (sn["g_in"] is None)
    return None if sn["g_in"] is None else sn["g_in"][0]


def _chk_feat_grad_relu(rec, sn, R, ctx):
    out = _images(rec["out"])
    y, t = _halves(sn["y"][0], rec["n_img"])
    # the coefficient from what the loss means, not from the record: each tap on this node adds 1 / (layers x elements)
    coef = len(rec["l"]) / (rec["nl"] * float(y.numel()))
    kind = 0 if not rec["l"] else (2 if rec["sq"] else 1)
    ref, need = ref_feat_grad(_g_in(rec, sn), y, t, coef, float(sn["gl"][0]), kind, rec["relu"])
    said = dict(cls="exact", rel_l2=0.0, max_rel=0.0, ulps=float("nan"),
                ok=kind == rec["loss_kind"] and y.numel() == rec["half"] and abs(coef - rec["coef"]) <= 1e-15 * coef)
    return [R("g", out, _bf16_elem(out, ref, need)), R("scalars", out[:0], said)]


def _chk_lpips_grad_relu(rec, sn, R, ctx):
    out = _images(rec["out"])
    n = rec["n_img"]
    y, t = _halves(sn["y"][0], n)
    c = y.shape[-1]
    assert y.numel() == rec["half"] and y.shape[1] * y.shape[2] == rec["pos"]
    g = _g_in(rec, sn)
    ref, need = ref_lpips_grad(None if g is None else g.reshape(n, -1, c), y.reshape(n, -1, c), t.reshape(n, -1, c), sn["head"],
                               sn["gl"], y.shape[1] * y.shape[2])
    return [R("g", out, _bf16_elem(out, ref.view(out.shape), need.view(out.shape)))]


def _chk_dgrad_padded(rec, sn, R, ctx):
    out = act_ndhwc(rec["out"])
    ref = TA.ref_dgrad(rec, sn)
    c = ref.shape[-1]
    pad = out[..., c:]
    return [R("dx", out[..., :c], cmp_bf16(out[..., :c], ref)), R("dx.pad", pad, cmp_same(pad, torch.zeros_like(pad)))]


REFS = {
    "maxpool2_fwd": _chk_maxpool2_fwd,
    "relu": _chk_relu,
    "feat_loss": _chk_feat_loss,
    "lpips_dist": _chk_lpips_dist,
    "feat_loss_finalize": _chk_feat_loss_finalize,
    "lpips_finalize": _chk_lpips_finalize,
    "feat_grad_relu": _chk_feat_grad_relu,
    "lpips_grad_relu": _chk_lpips_grad_relu,
    "maxpool2_bwd": _chk_maxpool2_bwd,
    "seam.grad_z": _chk_seam_grad_z,
}

# what is copied before the launch: everything it reads, and every buffer of which it may only write a part
_INPUTS = {
    "maxpool2_fwd": ("x",),
    "relu": ("x",),
    "feat_loss": ("x", "partials"),
    "lpips_dist": ("x", "head", "partials"),
    "feat_loss_finalize": ("partials",),
    "lpips_finalize": ("partials",),
    "feat_grad_relu": ("g_in", "y", "gl"),
    "lpips_grad_relu": ("g_in", "y", "head", "gl"),
    "maxpool2_bwd": ("x", "g"),
    "seam.grad_z": ("g",),
}


def _snapshot(rec: dict) -> dict:
    return {k: FA._clone(rec.get(k)) for k in _INPUTS[rec["kind"]]}


def _wide_dgrad(rec: dict) -> bool:
    """a data-gradient conv whose output Act has more channels than its weights give it"""
    if rec.get("kind") != "dgrad" or rec.get("op") != "convT" or rec.get("w_ci") is not None:
        return False
    return rec["out"].c > FA._val(rec["weight"]).shape[1]


def _run(prog, idx: Iterable[int], fwd: bool, ctx: dict):
    rows, missing = [], []
    for i in idx:
        rec = prog.op_audit[i]
        name, _, kern = prog.op_meta[i]
        kind = None if rec is None else rec.get("kind")
        R = lambda what, out, res: _row(i, name, kern, what, tuple(out.shape), res)
        if kind in REFS:
            sn = _snapshot(rec)
            prog.ops[i]()
            rows.extend(REFS[kind](rec, sn, R, ctx))
        elif fwd and kind in FA.REFS:
            sn = fwd_snapshot(rec)
            prog.ops[i]()
            rows.extend(FA.check(rec, sn, i, name, kern, ctx))
        elif not fwd and rec is not None and _wide_dgrad(rec):
            sn = train_snapshot(rec)
            prog.ops[i]()
            rows.extend(_chk_dgrad_padded(rec, sn, R, ctx))
        elif not fwd and rec is not None:
            sn = train_snapshot(rec)
            prog.ops[i]()
            rows.extend(TA.check(rec, sn, i, name, kern))
        else:
            if name not in (SKIP if fwd else TA.SKIP):
                missing.append(name)
            prog.ops[i]()
            continue
        del sn
    return rows, missing


def audit_forward(prog, only: Optional[Iterable[int]] = None, budget: Optional[int] = None, conv_cache: Optional[dict] = None):
    """Run ops[:n_fwd] one at a time (the inputs loaded by the caller), checking every op that has a record.  Returns (rows,
    unaccounted).  `only`: run and check just these op indices; `conv_cache`: as fwd_audit.audit_forward."""
    idx = range(prog.n_fwd) if only is None else sorted(only)
    with prog.ctx.scope(), torch.backends.cudnn.flags(enabled=False), torch.no_grad():
        ctx = dict(budget=FA.slab_budget(prog.ctx.device) if budget is None else budget, keep_tol=False, conv_cache=conv_cache)
        rows, missing = _run(prog, idx, True, ctx)
        prog.check_errors()
        torch.cuda.synchronize()
    return rows, missing


def audit_backward(prog, only: Optional[Iterable[int]] = None):
    """Run ops[n_fwd:] one at a time (after a forward, the upstream gradient set by the caller).  Returns (rows, unaccounted)."""
    idx = range(prog.n_fwd, len(prog.ops)) if only is None else sorted(only)
    with prog.ctx.scope(), torch.backends.cudnn.flags(enabled=False), torch.no_grad():
        rows, missing = _run(prog, idx, False, {})
        prog.check_errors()
        torch.cuda.synchronize()
    return rows, missing
