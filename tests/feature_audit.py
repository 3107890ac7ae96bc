"""Eager audit of the forward launches the optional U-Net features add, launch by launch (used by
tests/test_gpu_feature_program_audit.py, shown on the CPU by tests/test_host_feature_audit.py).

Scale-shift conditioning and dropout (norm_mod.py), true depth attention (attention.py), spatial attention
(spatial_attention.py), v-prediction (prediction.py), the x0 update form (x0_form.py), the learned variance (learned_sigma.py)
and latent window fusion (window_fuse.py) add launches to the U-Net step and training programs.  Every one of them carries an
audit record; `audit_forward` runs the forward ops one at a time, copies what a launch is about to read, runs it and recomputes
its result in float64 from exactly those operands, as tests/fwd_audit.py, tests/train_audit.py and tests/loss_audit.py do.  Kinds
those modules know go to their tables unchanged (fwd_audit.REFS; train_audit's `add`); the kinds below have their references
here, built from the restatements the op tests use (tests/*_restatement.py, keep_mask_np).  The comparisons, the bound constants
and the table format are fwd_audit's and train_audit's.

Record kinds and what they compute:
  gn_apply_mod         the ResBlock's middle pass: y = drop(silu(gn(x) (1 + s) + b)) (film) or drop(silu(gn(x)) + e), (s | b) or e
                       the block's columns of the time row of sample i at evaluation *step_ptr; bf16, or fp32 (`f32`: film only)
  attn_core            A = softmax(q k^T / sqrt(hd)) v over depth per (sample, h, w, head), [q | k | v] the thirds of `qkv`
  attn_plane           the same over the h * w positions of every (sample, slice, head); `lse` = ln sum_j exp(s_ij) where kept
  add (forward)        dst = bf16(fp32(dst) + fp32(src))                                          train_audit's reference
  pred_to_eps          out[b] <- a out[b] + b0 z[b mod z_rows] + b1 hist[b mod z_rows], {a, b0, b1} = rows[*step_ptr]
  x0_step              X = clip(alpha z - sigma v), z' = a z + b X + c hist + s noise; z, the z half of the network input, the
                       history (X), the non-finite counters
  sigma_split          eps = channels [0, L) of all n rows of out2, vraw = channels [L, 2L) of rows [0, n_keep)
  sampler_step ddpm_lv the ancestral step on a respaced row with the learned (vraw) or the fixed-small variance
  window_gather        the z half of every window row of the network input <- its box of the full-shape input, both halves
  window_blend         eps[g n + b] = sum_k wd wh ww win[(g nw + k) n + b] over the windows k covering the voxel
  hybrid_loss.fwd      {total, mse, vb, S_b, V_b}: L_simple + lambda L_vb of a 2L-channel prediction

Bounds (each from the arithmetic of the launch and the same as the kernel's op test holds it to; none from a measurement):
  gn_apply_mod bf16    train_audit.cmp_bf16: one bf16 ulp of float64 + BF16_FLOOR rms(ref) (tests/test_gpu_resblock_options.py's
                       header: fp32 from the load to the one rounding at the store).  Inside a program x may sit close to its
                       group mean, where the terms of the fp32 chain are much larger than the result: the reference computes
                       need = 2 k 2^-24 sum|terms| per element from its own float64 intermediates (k counted from
                       csrc/norm_act.hip beside its use, carried through the SiLU as fwd_audit does) and adds it as `extra` only
                       where it exceeds the rms floor somewhere (loss_audit's rule for its gradient passes; the row's `extra`
                       says which).
  gn_apply_mod drop    the dropped set equals keep_mask_np(seed, layer_id, element) exactly and every dropped element is +0
                       (bit for bit); kept elements within the bound above of inv x the undropped value; the layer_ids of one
                       program's records are pairwise distinct.
  gn_apply_mod f32     fwd_audit's fp32 elementwise class: 2 k 2^-24 sum|terms|, k counted from csrc/f32_ops.hip.
  attn_core, _plane    cmp_bf16 with extra = 2^-8 sum_k P |V|: P is rounded to bf16 for the P V MFMA
                       (tests/test_gpu_attn_softmax.py, tests/test_gpu_spatial_attention.py).  lse: the per-row bound written
                       out in the header of tests/test_gpu_spatial_attention.py.  Each row reports how far the float64 result is
                       from uniform attention (`uniform`).
  pred_to_eps          4 * 2^-24 * VR.convert_magnitude(...) (tests/test_gpu_vpred.py); z, hist and the row table bit for bit.
  x0_step              |X - X64| <= 4 * 2^-24 (|alpha z| + |sigma v|), |z' - z'64| <= 4 * 2^-24 (|a z| + |b X| + |c h| + |s n|)
                       + |b| (bound on X) (tests/test_gpu_x0_form.py::_kernel_bounds); the bf16 z half against bf16(z), the fp32
                       one and the counters exactly.
  sigma_split, window_gather   copies: bit for bit.
  ddpm_lv              the elementwise bound of learned_sigma_restatement.step (tests/test_gpu_learned_sigma.py::
                       test_lv_step_against_float64).
  window_blend         (K + 8) 2^-24 max_k |out_k| per voxel (tests/test_gpu_window_fuse_ops.py).
  hybrid_loss.fwd      the five bounds of tests/test_gpu_learned_sigma.py::test_hybrid_loss_forward_against_float64, from the
                       helpers that test calls (learned_sigma_restatement.hybrid_error_terms / hybrid_sum_bounds).

What the engine chooses and a record alone cannot show (the record and the launch are built from the same variables) is taken
from the MODEL where `audit_forward(model=)` is given: the columns of the stacked time row a block reads are those of the
ResBlock3D whose GroupNorm the launch applies (`time_row_plan`: the enumeration of unet.modules()), and the head count is the
module tree's.  `sigma_split` keeps as many rows as `vraw` has, which are the conditional ones.
"""
from __future__ import annotations

import math
from typing import Iterable, List, Optional

import numpy as np
import torch

from tests import attn_restatement as AR
from tests import fwd_audit as FA
from tests import learned_sigma_restatement as LR
from tests import resblock_restatement as RR
from tests import spatial_attn_restatement as SR
from tests import train_audit as TA
from tests import vpred_restatement as VR
from tests import x0_restatement as XR
from tests.fwd_audit import EPS32, SILU_SLOPE, SKIP, cmp_elem, cmp_same
from tests.test_host_resblock_options import keep_mask_np
from tests.train_audit import BF16_FLOOR, F64, act_ndhwc, cmp_bf16, cmp_exact, format_table, _row

__all__ = ["audit_forward", "format_table", "REFS", "_INPUTS", "DEFERRED_BACKWARD", "time_row_plan", "model_heads",
           "ref_gn_apply_mod", "ref_attn_core", "ref_attn_plane", "ref_pred_to_eps", "ref_x0_step", "ref_sigma_split",
           "ref_lv_step", "ref_window_gather", "ref_window_blend", "ref_hybrid_loss", "lse_bound",
           "cmp_within", "cmp_bf16", "cmp_same", "cmp_elem", "REL_HALF_ULP", "K_MOD_FILM", "K_MOD_ADD", "K_MOD_F32"]

REL_HALF_ULP = 2.0 ** -8        # half a bf16 ulp of x is at most this much of |x| (the attention core tests)
U24 = EPS32
# the backward launches of the same features: every one has its op test; their program audit is not part of this module
DEFERRED_BACKWARD = ("gn_bwd_mod", "attn_core_bwd", "attn_plane_bwd", "hybrid_loss_bwd")
# fp32 roundings of the affine part of ctsi_gn_apply_mod (csrc/norm_act.hip, gn_apply_kernel's prologue and `one`):
#   film      rstd -> fp32, gamma rstd, mean -> fp32, mean sc, beta - .., 1 + s, sc s1, sh s1, + b, x scale, + shift       = 11
#   additive  fwd_audit._affine's 7 (the FILM branch is not taken: the coefficients are ctsi_gn_apply's)
# and of ctsi_gn_apply_mod_f32 (csrc/f32_ops.hip): scale and shift are formed in double and rounded once each, x scale, + shift = 4
K_MOD_FILM, K_MOD_ADD, K_MOD_F32 = 11, 7, 4
K_DROP = 2                      # the dropout scale: inv -> fp32, the product


# ---- comparisons -----------------------------------------------------------------------------------------------------------
def cmp_within(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> dict:
    """|out - ref| <= bound elementwise (the op tests' criterion for fp32 launches): fwd_audit.cmp_elem with the bound as the
    tolerance; an element whose reference is not finite must hold the same bits."""
    r = ref.to(F64)
    fin = torch.isfinite(r)
    if bool(fin.all()):
        return cmp_elem(out, r, bound)
    res = cmp_elem(out.to(F64)[fin], r[fin], bound.to(F64).expand_as(r)[fin])
    o32, r32 = out.detach().to(torch.float32)[~fin], r.to(torch.float32)[~fin]
    res["ok"] = res["ok"] and cmp_same(o32, r32)["ok"]
    return res


def _exact(ok: bool, bad: int = 0) -> dict:
    return dict(cls="exact", rel_l2=0.0 if ok else math.inf, max_rel=0.0 if ok else math.inf, ulps=float("nan"), ok=bool(ok),
                mismatches=int(bad))


def _bf16_elem(out: torch.Tensor, ref: torch.Tensor, need: torch.Tensor) -> dict:
    """loss_audit's rule: one ulp + the floor where the fp32 chain stays under the floor everywhere, else + `need`."""
    rms = float(ref.pow(2).mean().sqrt()) if ref.numel() else 0.0
    inside = bool((need <= BF16_FLOOR * rms).all())
    plain = cmp_bf16(out, ref)
    res = plain if inside else cmp_bf16(out, ref, extra=need)
    res["extra"] = "-" if inside else "fp32 chain"
    res["plain_ulps"] = plain["ulps"]
    return res


def _rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.to(F64) - b.to(F64)).norm() / (b.to(F64).norm() + 1e-30))


# ---- what the model says about a launch -------------------------------------------------------------------------------------
def time_row_plan(unet) -> List[dict]:
    """Per ResBlock3D in unet.modules() order: the GroupNorm weight of its conv1 and its columns [off, off + width) of the
    stacked time projection (width = C, or 2C in scale-shift mode).  A launch is matched to its block by that weight, so the
    weights of same-shaped blocks must be pairwise different (formula weights are; freshly initialised all-ones weights are
    not): anything else is refused here, not matched loosely."""
    plan, off = [], 0
    for m in unet.modules():
        if type(m).__name__ == "ResBlock3D":
            width = m.time_mlp[1].out_features
            plan.append(dict(gamma=m.conv1.norm.weight.detach().to(torch.float32).cpu(), off=off, width=width))
            off += width
    for j, p in enumerate(plan):
        for q in plan[:j]:
            if q["gamma"].shape == p["gamma"].shape and torch.equal(q["gamma"], p["gamma"]):
                raise AssertionError(f"time_row_plan: the blocks at columns {q['off']} and {p['off']} have the same GroupNorm "
                                     "weight: a launch could not be told from its neighbour's")
    return plan


def model_heads(unet) -> Optional[int]:
    heads = {m.num_heads for m in unet.modules() if type(m).__name__ in ("TemporalAttention", "SpatialAttention")}
    assert len(heads) <= 1, heads
    return heads.pop() if heads else None


def _tb_columns(rec, sn, ctx) -> int:
    """The first column of the block's time row: with a model, the columns of THE ResBlock3D whose GroupNorm weight the launch
    applies (a record that points elsewhere then fails its row unless the two rows happen to be equal); else the record's."""
    plan = ctx.get("time_rows")
    if not plan:
        return int(rec["tbias_off"])
    gam = sn["gamma"].detach().to(torch.float32).cpu()
    mine = [p for p in plan if p["gamma"].shape == gam.shape and torch.equal(p["gamma"], gam)]
    if len(mine) != 1:
        raise AssertionError(f"gn_apply_mod: {len(mine)} ResBlock3D of the model have this launch's GroupNorm weight")
    return mine[0]["off"]


# ---- float64 references (plain tensors, any device) ------------------------------------------------------------------------------
def ref_gn_apply_mod(x, sums, gamma, beta, row, groups, eps, film, keep=None, inv=1.0, f32=False):
    """(reference, need) of the middle pass on NDHWC operands: the value is resblock_restatement.pass_fwd64's; `need` is the
    fp32 chain's 2 k EPS32 sum|terms| carried through the SiLU (fwd_audit._silu_err, SILU_SLOPE), the additive time row and
    the dropout scale."""
    n, c = x.shape[0], x.shape[-1]
    x = x.to(F64)
    ref = RR.pass_fwd64(x, sums, gamma, beta, row, groups, eps, film, keep=keep, inv=inv)
    count = float((c // groups) * x.shape[1] * x.shape[2] * x.shape[3])
    m, rstd = FA._gn_stats(sums.reshape(-1), 0, n, groups, c, count, eps)
    shape = (n, 1, 1, 1, c)
    sc, msc = (gamma.to(F64) * rstd).view(shape), (m * gamma.to(F64) * rstd).view(shape)
    b0 = beta.to(F64).view(1, 1, 1, 1, c)
    r = row.to(F64).view(n, 1, 1, 1, -1)
    if film:
        s1, b = 1.0 + r[..., :c], r[..., c:2 * c]
        u = x * sc * s1 + (b0 - msc) * s1 + b
        terms = (x * sc * s1).abs() + (msc * s1).abs() + (b0 * s1).abs() + b.abs()
        need = 2.0 * (K_MOD_F32 if f32 else K_MOD_FILM) * EPS32 * terms
        need = SILU_SLOPE * need + FA._silu_err(u)
        y = FA._silu(u)
    else:
        assert not f32, "the fp32 engine emits the scale-shift form only"
        u = x * sc + (b0 - msc)
        need = 2.0 * K_MOD_ADD * EPS32 * ((x * sc).abs() + msc.abs() + b0.abs())
        need = SILU_SLOPE * need + FA._silu_err(u)
        y = FA._silu(u) + r[..., :c]
        need = need + 2.0 * EPS32 * y.abs()                      # one add
    if keep is not None:
        need = (inv * need + 2.0 * K_DROP * EPS32 * (inv * y).abs()) * keep.to(F64)
    return ref, need


def ref_attn_core(qkv, heads: int):
    """qkv NDHWC (n, d, h, w, 3c) -> (A, extra, uniform), each (n, h, w, heads, d, hd)."""
    q, k, v = (t.to(F64) for t in AR.split_qkv(qkv, heads))
    a, p = AR.core_fwd64(q, k, v)
    return a, REL_HALF_ULP * (p @ v.abs()), AR.core_uniform64(v)


def lse_bound(q, k, s, lse):
    """The per-row bound of the header of tests/test_gpu_spatial_attention.py; q, k (..., N, hd), s = q k^T / sqrt(hd)."""
    nq, hd = q.shape[-2], q.shape[-1]
    sabs = (q.abs() @ k.abs().transpose(-1, -2) * hd ** -0.5).amax(-1)
    return U24 * ((hd + 1) * sabs + 10 * s.abs().amax(-1) + nq + 3 * ((nq + 63) // 64) + 2 + 6 * lse.abs())


def ref_attn_plane(qkv, heads: int):
    """qkv NDHWC -> dict(a, extra, uniform: (n, d, heads, N, hd); lse, lse_tol: (n, d, heads, N))."""
    q, k, v = (t.to(F64) for t in SR.split_qkv_plane(qkv, heads))
    a, p = AR.core_fwd64(q, k, v)
    s = q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5
    lse = torch.logsumexp(s, dim=-1)
    return dict(a=a, extra=REL_HALF_ULP * (p @ v.abs()), uniform=AR.core_uniform64(v), lse=lse, lse_tol=lse_bound(q, k, s, lse))


def ref_pred_to_eps(out, z, hist, row, z_rows: int):
    """out (rows, ...), z / hist (z_rows, ...), row {a, b0, b1, .} -> (eps, bound)."""
    idx = [b % z_rows for b in range(out.shape[0])]
    zz = z[idx]
    hh = None if hist is None else hist[idx]
    r = row.to(F64).cpu()
    return VR.convert(out, zz, r, hh), 4.0 * U24 * VR.convert_magnitude(out, zz, r, hh)


def ref_x0_step(z, v, row, hist=None, noise=None):
    """One ctsi_x0_step on NDHWC tensors: dict(x, bx, z, bz, counts) -- X and z' of x0_restatement.kernel with the bounds of
    tests/test_gpu_x0_form.py::_kernel_bounds, z' sanitised as the kernel stores it, and the six non-finite counters."""
    r = row.to(F64).cpu()
    x64, z64, mag_x, mag = XR.kernel(z, v, r, hist, noise)
    bx = 4.0 * U24 * mag_x
    bz = 4.0 * U24 * mag + abs(float(r[3])) * bx
    vv = v.to(F64)
    raw_x = float(r[0]) * z.to(F64) - float(r[1]) * XR.nan_to_num(vv)        # X before it is sanitised: what is counted
    counts = FA._count(vv) + FA._count(raw_x) + FA._count(z64)
    return dict(x=x64, bx=bx, z=XR.nan_to_num(z64), bz=bz, counts=counts)


def ref_sigma_split(out2, L: int, n_keep: int):
    return out2[..., :L].contiguous(), out2[:n_keep, ..., L:].contiguous()


def ref_lv_step(z, eps, vraw, noise, row):
    """(z', bound) of learned_sigma_restatement.step on NDHWC tensors."""
    out, _, bound = LR.step(z, eps, vraw, noise, row.to(F64).cpu())
    return out, bound


def _boxes(starts, n: int, halves: int):
    nw = len(starts)
    for g in range(halves):
        for k, st in enumerate(starts):
            for b in range(n):
                yield (g * nw + k) * n + b, g, k, b, tuple(int(v) for v in st)


def ref_window_gather(src, zin_before, starts, n, halves, L, win):
    """torch slicing: the z half of row (g nw + k) n + b is the box of window k in row b of `src`; the rest keeps its bits."""
    want = zin_before.clone()
    td, lh, lw = win
    for r, g, k, b, (sd, sh, sw) in _boxes(starts, n, halves):
        want[r, ..., :L] = src[b, sd:sd + td, sh:sh + lh, sw:sw + lw, :L]
    return want


def table_starts(tables, nwin) -> list:
    """Per axis the start of window k: the position its table covers at offset 0."""
    axes = []
    for t, k in zip(tables, nwin):
        st = [None] * k
        for p in range(t.count.shape[0]):
            for j in range(int(t.count[p])):
                if t.offset[p, j] == 0:
                    st[t.index[p, j]] = p
        axes.append(st)
    return axes


def ref_window_blend(win_t, tables, n, halves, nwin, full, win):
    """float64 (sum_k wd wh ww out_k, bound = (K + 8) 2^-24 max_k |out_k|, starts), of the full shape (halves n, D, H, W, L),
    from the host tables: the restatement and the bound of tests/test_gpu_window_fuse_ops.py (`_restate`, `_check`)."""
    from tests.test_gpu_window_fuse_ops import _restate, _starts
    axes = table_starts(tables, nwin)
    ref, K, amax = _restate(win_t, tables, n, halves, tuple(full), tuple(win), axes)
    dev = win_t.device
    return ref.to(dev), ((K[None, ..., None] + 8) * U24 * amax).to(dev), _starts(axes)


def _sched_columns(rows):
    """The per-timestep columns ctsi_hybrid_loss_fwd reads, float64: it takes log beta~ (c5) and log beta - log beta~ (d45) and
    never log beta itself, so log beta = c5 + d45."""
    r = rows.to(F64)
    return dict(a=r[:, 0], s=r[:, 1], c1=r[:, 2], c2=r[:, 3], log_beta=r[:, 5] + r[:, 6], log_post=r[:, 5])


def ref_hybrid_loss(pred2, z0, noise, t, rows, v_pred, mask, norm, norm_vb):
    """NCDHW operands, `rows` the (T, 8) table the launch read, mask (n, L, d) or None -> (reference, bound), each the
    3 + 2n values {total, mse, vb, S_b, V_b}.  Element terms, their error magnitudes and the five bounds are
    learned_sigma_restatement's (`hybrid_terms`, `hybrid_error_terms`, `hybrid_sum_bounds`), the ones
    tests/test_gpu_learned_sigma.py::test_hybrid_loss_forward_against_float64 holds the kernel to."""
    n = z0.shape[0]
    sched = _sched_columns(rows)
    t = t.long()
    mse_e, vb_e = LR.hybrid_terms(pred2.to(F64), z0, noise, t, sched, bool(v_pred))
    mag_mse, mag_vb = LR.hybrid_error_terms(pred2, z0, noise, t, sched, bool(v_pred))
    me = 1.0 if mask is None else mask.to(F64).reshape(n, z0.shape[1], z0.shape[2])[:, :, :, None, None]
    S, V = (me * mse_e).reshape(n, -1).sum(1), (me * vb_e).reshape(n, -1).sum(1)
    S_mag, V_mag = (me * mag_mse).reshape(n, -1).sum(1), (me * mag_vb).reshape(n, -1).sum(1)
    nm, nv = norm.to(F64), norm_vb.to(F64)
    bd = LR.hybrid_sum_bounds(S, V, S_mag, V_mag, nm, nv)
    mse, vb = (nm * S).sum(), (nv * V).sum()
    ref = torch.cat([torch.stack([mse + vb, mse, vb]), S, V])
    bound = torch.cat([torch.stack([bd["total"], bd["mse"], bd["vb"]]), bd["S_b"], bd["V_b"]])
    return ref, bound


# ---- checks, one function per kind ---------------------------------------------------------------------------------------------
def _time_rows(rec, sn, ctx, n: int, width: int) -> torch.Tensor:
    step = int(sn["step_ptr"][0]) if sn["step_ptr"] is not None else 0
    tb, stride = sn["tbias"].reshape(-1), rec["tbias_stride"]
    r0 = _tb_columns(rec, sn, ctx) + step * n * stride
    return torch.stack([tb[r0 + i * stride:r0 + i * stride + width] for i in range(n)])


def _chk_gn_apply_mod(rec, sn, R, ctx):
    out = act_ndhwc(rec["out"])
    x = sn["x"]
    n, c = x.shape[0], x.shape[-1]
    film, f32, groups = bool(rec["film"]), bool(rec.get("f32")), rec["groups"]
    assert rec["d_stat"] == x.shape[1] and rec["silu_pre"], "the middle pass of an unsharded program"
    row = _time_rows(rec, sn, ctx, n, 2 * c if film else c)
    sums = sn["sums"][rec["slot"]:rec["slot"] + n * groups * 2]
    st = rec["drop"]
    if st is None:
        ref, need = ref_gn_apply_mod(x, sums, sn["gamma"], sn["beta"], row, groups, rec["eps"], film, f32=f32)
        if f32:
            return [R("y", out, cmp_elem(out, ref, need))]
        return [R("y", out, _bf16_elem(out, ref, need))]
    seed = int(sn["seed"][0]) & 0xFFFFFFFFFFFFFFFF
    keep = torch.from_numpy(keep_mask_np(seed, int(rec["layer_id"]), int(st.thr), x.numel()).astype(np.bool_)).to(x.device)
    keep = keep.view(x.shape)
    ref, need = ref_gn_apply_mod(x, sums, sn["gamma"], sn["beta"], row, groups, rec["eps"], film, keep=keep, inv=float(st.inv))
    dropped = out[~keep]
    res_d = cmp_same(dropped, torch.zeros_like(dropped))            # exactly +0, every one of them
    tol = FA.bf16_tol(ref, need)
    lost = int(((out == 0) & keep & (ref.abs() > tol)).sum())       # kept by the rule, zero in the output
    res_d["mismatches"] = res_d.get("mismatches", 0) + lost
    res_d["ok"] = res_d["ok"] and lost == 0
    res_d["kept"] = float(keep.to(F64).mean())
    seen = ctx.setdefault("layer_ids", {})
    first = seen.setdefault(int(rec["layer_id"]), id(rec))
    return [R("y", out[keep], _bf16_elem(out[keep], ref[keep], need[keep])), R("dropped", dropped, res_d),
            R("layer_id", out[:0], _exact(first == id(rec), 0 if first == id(rec) else 1))]


def _heads(rec, ctx) -> int:
    return int(ctx.get("heads") or rec["heads"])


def _chk_attn_core(rec, sn, R, ctx):
    heads = _heads(rec, ctx)
    out = AR.split_heads(act_ndhwc(rec["out"]), heads)
    a, extra, uni = ref_attn_core(sn["qkv"], heads)
    res = cmp_bf16(out, a, extra)
    res["uniform"] = _rel_l2(uni, a)
    return [R("A", out, res)]


def _chk_attn_plane(rec, sn, R, ctx):
    heads = _heads(rec, ctx)
    out = SR.split_plane(act_ndhwc(rec["out"]), heads)
    ref = ref_attn_plane(sn["qkv"], heads)
    res = cmp_bf16(out, ref["a"], ref["extra"])
    res["uniform"] = _rel_l2(ref["uniform"], ref["a"])
    rows = [R("A", out, res)]
    if rec["lse"] is not None:
        lse = rec["lse"][:ref["lse"].numel()].view(ref["lse"].shape)
        rows.append(R("lse", lse, cmp_elem(lse, ref["lse"], ref["lse_tol"])))
    return rows


def _chk_pred_to_eps(rec, sn, R, ctx):
    assert rec["rows_per_step"] == 1, "the step programs hold one conversion row per evaluation"
    step = int(sn["step_ptr"][0])
    out = rec["out"]
    assert out.shape[0] == rec["n"] and sn["z"].shape[0] == rec["z_rows"]
    ref, bound = ref_pred_to_eps(sn["out"], sn["z"], sn["hist"], sn["rows"][step], rec["z_rows"])
    rows = [R("eps", out, cmp_within(out, ref, bound)), R("z", rec["z"], cmp_same(rec["z"], sn["z"])),
            R("rows", rec["rows"], cmp_same(rec["rows"], sn["rows"]))]
    if rec["hist"] is not None:
        rows.append(R("hist", rec["hist"], cmp_same(rec["hist"], sn["hist"])))
    return rows


def _zin_rows(rec, sn, R, zout, n, L):
    """The z half of the network input (bf16 against bf16(z), fp32 exact) and everything else of that tensor."""
    zin = act_ndhwc(rec["zin"])
    half = zin[:n, ..., :L]
    if zin.dtype == torch.bfloat16:
        rows = [R("zin", half, cmp_exact(half.contiguous(), zout.to(torch.bfloat16)))]
    else:
        rows = [R("zin", half, cmp_same(half, zout))]
    rest = sn["zin"].clone()
    rest[:n, ..., :L] = half
    return rows + [R("zin.rest", zin, cmp_same(zin, rest))]


def _noise_ndhwc(sn):
    return None if sn["noise"] is None else sn["noise"].permute(0, 2, 3, 4, 1)


def _chk_x0_step(rec, sn, R, ctx):
    n, L = rec["n"], rec["L"]
    step = int(sn["step_ptr"][0])
    ref = ref_x0_step(sn["z"], sn["v"][:n], sn["coef"][step], sn["hist"], _noise_ndhwc(sn))
    zout = rec["z"]
    rows = [R("z", zout, cmp_within(zout, ref["z"], ref["bz"]))] + _zin_rows(rec, sn, R, zout, n, L)
    if rec["hist"] is not None:
        rows.append(R("hist", rec["hist"], cmp_within(rec["hist"], ref["x"], ref["bx"])))
    if rec["nonfinite"] is not None:
        want = sn["nonfinite"].clone()
        want[step] += torch.tensor(ref["counts"], dtype=want.dtype, device=want.device)
        rows.append(R("nonfinite", rec["nonfinite"], cmp_same(rec["nonfinite"], want)))
    return rows


def _chk_sigma_split(rec, sn, R, ctx):
    L, vraw = rec["L"], FA._val(rec["vraw"])
    out2 = sn["out2"]
    assert out2.shape[0] == rec["n"] and out2.shape[-1] == 2 * L
    rows = [R("out2", rec["out2"], cmp_same(rec["out2"], out2))]
    if vraw is None:
        eps, _ = ref_sigma_split(out2, L, 0)
        return rows + [R("eps", rec["eps"], cmp_same(rec["eps"], eps))]
    n_keep = vraw.shape[0]                                  # the rows the update reads: the conditional ones
    eps, var = ref_sigma_split(out2, L, n_keep)
    said = rec["n_keep"] == n_keep and n_keep <= rec["n"]
    return rows + [R("eps", rec["eps"], cmp_same(rec["eps"], eps)), R("vraw", vraw, cmp_same(vraw, var)),
                   R("n_keep", vraw[:0], _exact(said, 0 if said else 1))]


def _chk_lv_step(rec, sn, R, ctx):
    n, L = rec["n"], rec["L"]
    step = int(sn["step_ptr"][0])
    ref, bound = ref_lv_step(sn["z"], sn["eps"][:n], sn["vraw"], _noise_ndhwc(sn), sn["coef"][step])
    zout = rec["z"]
    res = cmp_within(zout, ref, bound)
    res["vraw"] = sn["vraw"] is not None
    return [R("z", zout, res)] + _zin_rows(rec, sn, R, zout, n, L)


def _chk_window_gather(rec, sn, R, ctx):
    zin = act_ndhwc(rec["zin"])
    L = rec["L"]
    starts = [tuple(int(v) for v in s) for s in sn["starts"].cpu().tolist()]
    assert len(starts) == rec["nw"] and zin.shape[0] == rec["halves"] * rec["nw"] * rec["n"]
    want = ref_window_gather(sn["src"], sn["zin"], starts, rec["n"], rec["halves"], L, rec["win"])
    rows = [R("zin", zin[..., :L], cmp_same(zin[..., :L], want[..., :L]))]
    if zin.shape[-1] > L:
        rows.append(R("cond", zin[..., L:], cmp_same(zin[..., L:], sn["zin"][..., L:])))
    return rows


def _chk_window_blend(rec, sn, R, ctx):
    from importlib import import_module
    WF = import_module("video-to-video-diffusion_amd.window_fuse")
    out = rec["out"]
    ref, bound, _ = ref_window_blend(sn["win"], rec["tables"], rec["n"], rec["halves"], rec["nwin"], rec["full"], rec["win_dims"])
    ti, tw = WF.pack_tables(rec["tables"])
    tabs = cmp_same(rec["tab_i"], ti.to(out.device))["ok"] and cmp_same(rec["tab_w"], tw.to(out.device))["ok"]
    return [R("eps", out, cmp_within(out, ref, bound)), R("tables", rec["tab_w"], _exact(tabs, 0 if tabs else 1))]


def _chk_hybrid_loss_fwd(rec, sn, R, ctx):
    out = rec["out"]
    pred2 = sn["pred2"].permute(0, 4, 1, 2, 3)                       # NDHWC -> NCDHW
    n = pred2.shape[0]
    ref, bound = ref_hybrid_loss(pred2, sn["z0"], sn["noise"], sn["t_rows"], sn["sched"], rec["v_pred"], sn["mask"], sn["norm"],
                                 sn["norm_vb"])
    got = out[:3 + 2 * n]
    res = cmp_within(got, ref, bound)
    res["mask"] = sn["mask"] is not None
    return [R("loss", got, res)]


REFS = {
    "gn_apply_mod": _chk_gn_apply_mod,
    "attn_core": _chk_attn_core,
    "attn_plane": _chk_attn_plane,
    "pred_to_eps": _chk_pred_to_eps,
    "x0_step": _chk_x0_step,
    "sigma_split": _chk_sigma_split,
    "sampler_step.ddpm_lv": _chk_lv_step,
    "window_gather": _chk_window_gather,
    "window_blend": _chk_window_blend,
    "hybrid_loss.fwd": _chk_hybrid_loss_fwd,
}

# what is copied before the launch: everything it reads, and every buffer of which it may only write a part
_INPUTS = {
    "gn_apply_mod": ("x", "sums", "gamma", "beta", "tbias", "step_ptr"),
    "attn_core": ("qkv",),
    "attn_plane": ("qkv",),
    "pred_to_eps": ("out", "z", "hist", "rows", "step_ptr"),
    "x0_step": ("z", "v", "hist", "noise", "zin", "coef", "step_ptr", "nonfinite"),
    "sigma_split": ("out2",),
    "sampler_step.ddpm_lv": ("z", "eps", "vraw", "noise", "zin", "coef", "step_ptr"),
    "window_gather": ("src", "zin", "starts"),
    "window_blend": ("win",),
    "hybrid_loss.fwd": ("pred2", "z0", "noise", "t_rows", "sched", "mask", "norm", "norm_vb"),
}


def kind_of(rec: Optional[dict]) -> Optional[str]:
    """The key of a record in REFS / _INPUTS: its kind; the learned-variance update is told from the other sampler steps."""
    if rec is None:
        return None
    if rec.get("kind") == "sampler_step" and rec.get("sampler") == "ddpm_lv":
        return "sampler_step.ddpm_lv"
    return rec.get("kind")


def _snapshot(rec: dict, kind: str) -> dict:
    sn = {k: FA._clone(rec.get(k)) for k in _INPUTS[kind]}
    if kind == "gn_apply_mod" and rec["drop"] is not None:
        sn["seed"] = rec["drop"].seed.detach().clone()
    return sn


def references(kind: Optional[str]) -> Optional[str]:
    """Which table answers for a forward record kind: 'feature', 'train' (train_audit's add), 'fwd' or None."""
    if kind in REFS:
        return "feature"
    if kind == "add":
        return "train"
    if kind in FA.REFS:
        return "fwd"
    return None


def audit_forward(prog, stop: Optional[int] = None, only: Optional[Iterable[int]] = None, model=None,
                  budget: Optional[int] = None):
    """Run ops[:stop] one at a time (the inputs loaded by the caller), checking every op that has a record.  `only`: run and
    check just these op indices.  `model`: the U-Net the program was built from -- its time-row plan and head count then
    replace the record's own.  Returns (rows, unaccounted): one result row per checked output, and the names of the ops run
    that have neither a reference nor an entry in fwd_audit.SKIP."""
    stop = len(prog.ops) if stop is None else stop
    idx = range(stop) if only is None else sorted(only)
    rows, missing = [], []
    with prog.ctx.scope(), torch.backends.cudnn.flags(enabled=False), torch.no_grad():
        ctx = dict(budget=FA.slab_budget(prog.ctx.device) if budget is None else budget, keep_tol=False, conv_cache=None)
        if model is not None:
            ctx["time_rows"], ctx["heads"] = time_row_plan(model), model_heads(model)
        for i in idx:
            rec = prog.op_audit[i]
            name, _, kern = prog.op_meta[i]
            kind = kind_of(rec)
            table = references(kind)
            if table == "feature":
                R = lambda what, out, res: _row(i, name, kern, what, tuple(out.shape), res)
                sn = _snapshot(rec, kind)
                prog.ops[i]()
                rows.extend(REFS[kind](rec, sn, R, ctx))
            elif table == "train":
                sn = TA.snapshot(rec)
                prog.ops[i]()
                rows.extend(TA.check(rec, sn, i, name, kern))
            elif table == "fwd":
                sn = FA.snapshot(rec)
                prog.ops[i]()
                rows.extend(FA.check(rec, sn, i, name, kern, ctx))
            else:
                if name not in SKIP:
                    missing.append(name)
                prog.ops[i]()
                continue
            del sn
        prog.check_errors()
        torch.cuda.synchronize()
    return rows, missing


# ---- the feature model of the program tests, and its restatement with taps -------------------------------------------------------
# Formula weights leave every attention nearly uniform (scores of a few 1e-2): a core that averaged V would pass.  The q and k
# thirds of every qkv conv (weight and bias) are scaled by QK_GAIN, the precedent being PROJ_GAIN of
# tests/test_gpu_spatial_attention.py: the smallest power of two at which the float32 restatement of program A's network
# (`restated_taps`, on the CPU alone) puts at least one attn_core and one attn_plane launch more than 0.5 rel-L2 from uniform
# attention.  Model seed 8, inputs program_inputs(SHAPE_A, 100), t = 999 (program A's first evaluation); the largest distance
# over the launches of each kind:   gain 1: attn_core 0.245, attn_plane 0.386   gain 2: attn_core 0.606, attn_plane 0.887
# (at 2 every one of the 11 launches is more than 0.56 away).  tests/test_host_feature_audit.py recomputes both lines.
QK_GAIN = 2.0
MODEL_SEED, INPUT_SEED = 8, 100
FEATURE_LEVELS = [0, 1]
SHAPE_A = (1, 8, 5, 12, 8)       # depth not a multiple of four; N = 96 at level 0, 24 at level 1 and the mid block


def feature_kw(**extra) -> dict:
    from tests.helpers import TINY_UNET
    return dict(TINY_UNET, use_scale_shift_norm=True, spatial_attention_levels=list(FEATURE_LEVELS), **extra)


def feature_unet(pkg, seed: int, gain: Optional[float] = None, spatial: bool = True, **extra):
    """TINY_UNET with scale-shift ResBlocks, softmax depth attention and spatial blocks on both levels, formula weights: every
    key of the model without spatial blocks keeps the weights that model has at this seed, only the new keys are drawn for
    this one (tests/test_gpu_spatial_attention.py::_spatial_model); then the q and k thirds of every qkv conv times `gain`."""
    from tests.helpers import formula_sd
    kw = feature_kw(**extra)
    base_kw = {k: v for k, v in kw.items() if k != "spatial_attention_levels"}
    un = pkg.UNet3D(**(kw if spatial else base_kw))
    sd = formula_sd(un, seed)
    if spatial:
        sd.update(formula_sd(pkg.UNet3D(**base_kw), seed))
    gain = QK_GAIN if gain is None else gain
    for k in list(sd):
        if k.endswith(".qkv.weight") or k.endswith(".qkv.bias"):
            c2 = 2 * (sd[k].shape[0] // 3)
            v = sd[k].clone()
            v[:c2] = v[:c2] * gain
            sd[k] = v
    un.load_state_dict(sd, strict=True)
    un.eval()
    un.attention_mode = "softmax"
    return un, sd


def feature_cfg(spatial: bool = True) -> dict:
    from tests.helpers import TINY_UNET, unet_cfg
    return dict(unet_cfg(TINY_UNET), spatial_attention_levels=list(FEATURE_LEVELS) if spatial else [])


def program_inputs(shape, seed: int):
    """(z, cond) of a program test, fp32 NCDHW on the CPU."""
    g = lambda s: torch.randn(shape, generator=torch.Generator().manual_seed(s))
    return g(seed + 1), g(seed + 2)


def restated_taps(sd, cfg, x, t, c, masks=None, inv: float = 1.0, edit=None):
    """The restatement of the feature network (scale-shift ResBlocks of resblock_restatement, the softmax depth attention of
    attn_restatement, the walk of spatial_attn_restatement) in x's dtype, with a tap on every block: returns (output, taps),
    taps[name] = dict(kind, x: the block's input, temb for a ResBlock).  `edit(kind, name, args)` may change the arguments a
    block is called with (the planted defects of tests/test_host_feature_audit.py)."""
    from oracle import ref_ops as R
    taps = {}
    res_fn, tmp_fn, sp_fn = RR.make_resblock(masks, inv), AR.temporal_attention_softmax, SR.spatial_attention

    def resblock(sd_, p, x_, temb):
        taps[p] = dict(kind="resblock", x=x_, temb=temb)
        a = dict(sd=sd_, p=p, x=x_, temb=temb)
        if edit:
            edit("resblock", p, a)
        return res_fn(a["sd"], a["p"], a["x"], a["temb"])

    def temporal(sd_, p, x_, heads):
        taps[p] = dict(kind="attn_core", x=x_)
        a = dict(sd=sd_, p=p, x=x_, heads=heads)
        if edit:
            edit("attn_core", p, a)
        return tmp_fn(a["sd"], a["p"], a["x"], a["heads"])

    def spatial(sd_, p, x_, heads):
        taps[p] = dict(kind="attn_plane", x=x_)
        a = dict(sd=sd_, p=p, x=x_, heads=heads)
        if edit:
            edit("attn_plane", p, a)
        return sp_fn(a["sd"], a["p"], a["x"], a["heads"])

    saved = (R.unet_resblock, R.temporal_attention, SR.spatial_attention)
    R.unet_resblock, R.temporal_attention, SR.spatial_attention = resblock, temporal, spatial
    try:
        out = SR.unet_forward(sd, cfg, x, t, c)
    finally:
        R.unet_resblock, R.temporal_attention, SR.spatial_attention = saved
    return out, taps


def tap_qkv(sd, p: str, x):
    """The qkv tensor of the attention block `p` on its input x (NCDHW), NDHWC: oracle.ref_ops' own GroupNorm and conv."""
    from oracle import ref_ops as R
    qkv = R.conv3d(sd, p + ".qkv", R.gn(sd, p + ".norm", x, R.group_count(x.shape[1])))
    return qkv.permute(0, 2, 3, 4, 1).contiguous()


def uniform_distances(sd, cfg, x, t, c, heads: int) -> dict:
    """name -> (kind, rel-L2 of the float64 core result of the tapped qkv from uniform attention)."""
    _, taps = restated_taps(sd, cfg, x, t, c)
    out = {}
    for p, tp in taps.items():
        if tp["kind"] == "attn_core":
            a, _, uni = ref_attn_core(tap_qkv(sd, p, tp["x"]), heads)
        elif tp["kind"] == "attn_plane":
            r = ref_attn_plane(tap_qkv(sd, p, tp["x"]), heads)
            a, uni = r["a"], r["uniform"]
        else:
            continue
        out[p] = (tp["kind"], _rel_l2(uni, a))
    return out
