"""Eager audit of a program's forward pass, launch by launch (used by tests/test_gpu_fwd_audit.py and test_host_fwd_audit.py, and
by the conv op tests through tests/gpu_utils.run_conv(audit=True) / audit_program: test_gpu_ops.py, test_gpu_vgg_ops.py,
test_gpu_train_ops.py, shown on the CPU by test_host_conv_op_audit.py; tests/loss_audit.py sends the forward ops of the
perceptual-loss and decode-gradient programs through `snapshot` / `check` and keeps the references of their own kinds).

Every forward op of engine.Program / UNetProgram / VAEEncodeProgram / VAEDecodeProgram, of the fp32 engine and of the forward
halves of the training programs carries an audit record (`Program.op_audit`, parallel to `ops` / `op_meta`).  `audit_forward`
runs the ops one at a time; for each op with a record it copies the operands the op is about to read -- including a destination
that is also an input (the in-place gn_apply, the fused GroupNorm tail that normalises its own output buffer) and the buffers
whose untouched part must stay as it was -- runs the op, and recomputes its result from exactly those operands in float64 torch
on the device (cudnn / MIOpen off).  Each number therefore describes one launch: errors of earlier launches do not compound.
`_colsum` is reused by every conv, so the GroupNorm column sums are checked at the launch that writes them.

Depth-sharded programs are out of scope: their Acts carry depth halos, which `act_ndhwc` refuses.

Record kinds and what they compute (Acts are NDHWC, bf16 in the bf16 engine and fp32 in the fp32 engine, `f32=True`):
  conv_fwd             out = act(conv(cat(x1, x2)[:, :cin_w], W) + bias [+ residual]), W = bf16(weight()) (fp32 engine: weight()),
                       act = none / tanh / ReLU;
                       output a bf16 / fp32 Act or a strided fp32 tensor; `stats`: column-sum slab [2][class * n * tps][cpad] of
                       the UNROUNDED result; `fuse_gn`: out = silu?(gn(h) + conv result), h possibly the output buffer itself
  gn_colsum            colsum[2][n * tps][c]: per 512-voxel tile sums of x and x^2
  gn_finalize          sums[slot + (i * groups + g) * 2 ..] = fp64 (sum, sumsq) of the slab(s), later parts accumulating
  gn_apply             out = [silu](x sc + sh) [+ tbias row (*step_ptr) n + i] [+ residual] [silu], sc = gamma rstd, sh = beta - mean sc
  attn_depthsum        depthsum = sum_d x (fp32) and the column sums of x per tile of `tile_pos` positions
  attn_normsum         out = gamma rstd (S - D mean) + D beta
  attn_pv              out = bias + W bf16(that), W bf16 [c][c]
  attn_softmax_rowsum  out[n, d, h, w, head] = sum_k softmax_k(q . k hd^-0.5)
  attn_broadcast_add   out = x + p [rowsum] broadcast over depth
  cfg_stats / cfg_stats_finalize / cfg_combine / cfg_mirror   csrc/guidance.hip
  sampler_step         every SAMPLER_STEPS kind: z, the z half of the network input, the history, the non-finite counters
  sampler_advance      *step_ptr += 1
  train.inputs         q_sample into the z half, the conditioning into the other half, the time-bias table
  loss.fwd             loss_out[0] = sum_b norm[b] S_b, loss_out[1 + b] = S_b = sum mask (pred - noise)^2
  seam.z_to_bf16       out = bf16(z) in NDHWC

Bounds (each from the arithmetic of the launch, none from a measurement):
  bf16 outputs       every element within BF16_ULPS = 1 bf16 ulp of the float64 reference + BF16_FLOOR rms(ref), rel-L2 <=
                     BF16_REL_L2 against bf16(ref) (train_audit's constants).  Products of bf16 operands are exact in fp32 and
                     accumulating K <= 27 x 768 of them in fp32 leaves ~sqrt(K) 2^-24 of the operand scale: far below the half
                     ulp the final rounding takes, the other half is slack.  Where the SOURCE shows more than that one rounding,
                     a per-element term computed from the reference's own intermediates is added (`extra`), see _affine, _normsum,
                     _silu_err, FUSE_R_ULPS, PV_XS_ULPS.
  fp32 accumulations strided fp32 conv outputs, fp32-engine convs, column sums against the float64 sums of the float64 conv
                     result, depth sums, cfg statistics, the time-bias table, the loss: F32_REL_L2 / F32_MAX_REL of train_audit.
  fp32 elementwise   sampler updates, cfg_combine, the fp32 gn_apply / normsum / broadcast_add: per element
                     |err| <= 2 k 2^-24 sum|terms|, k = the fp32 roundings of the kernel's expression (counted beside each use).
  copies and casts   cfg_mirror, seam.z_to_bf16, the conditioning half, the bf16 z half against bf16(z), every buffer part a
                     launch must leave alone: bit for bit.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional

import torch
import torch.nn.functional as F

from tests.train_audit import (BF16_FLOOR, BF16_REL_L2, BF16_ULPS, F32_MAX_REL, F32_REL_L2, F64, act_ndhwc, bf16_ulp, cmp_bf16,
                               cmp_exact, cmp_f32, format_table, _row)

__all__ = ["audit_forward", "require_ok", "bf16_tol", "format_table", "conv64", "slab_budget", "cmp_bf16", "cmp_f32", "cmp_exact",
           "cmp_elem", "cmp_same", "unaccounted", "SKIP", "REFS", "_INPUTS"]

# forward ops that may carry no record: launches that compute nothing (copies between ranks, memsets, stream joins)
SKIP: Dict[str, str] = {
    "halo.exchange": "comm: copies boundary slices between depth neighbours (sharded programs only)",
    "halo.exchange.async": "comm: the same copy on the second stream (sharded programs only)",
    "halo.join": "comm: a stream wait, no kernel",
    "gn.sync": "comm: all-reduce of statistics + boundary-slice copy (sharded programs only)",
    "attn.sync": "comm: all-reduce of statistics and the depth sum (sharded programs only)",
    "halo.zero_ends": "two memsets of halo slices (sharded programs only; nothing is emitted on one GPU)",
}

EPS32 = 2.0 ** -24          # half an fp32 ulp, relative: one fp32 rounding of a value v moves it by at most EPS32 |v|
# Second roundings the sources show (each a per-element term, scaled by the reference's own intermediate):
#  * the gather kernel's fused GroupNorm tail (csrc/conv_mfma.hip) stages the conv result r through LDS as bf16 before it adds
#    gn(h): r is rounded to nearest (half an ulp of r), and that error passes through the SiLU with |silu'| <= 1.1.  The
#    streaming tail (csrc/conv1_stream.hip) adds its fp32 accumulators: no such term there.
FUSE_R_ULPS = 0.5
#  * ctsi_attn_pv rounds the normalised depth sum xs to bf16 (its MFMA operand, "rounded to bf16 like its output"): every
#    output moves by at most sum_ci |W[co][ci]| (half an ulp of xs[ci] + the fp32 error of xs[ci]).
PV_XS_ULPS = 0.5
SILU_SLOPE = 1.1            # max |d silu / dz| (1.0998 at z = 2.4): how an error before a SiLU passes through it
SLAB_BUDGET_FRACTION = 0.25  # of the free device memory, for the columns of one float64 conv call


# ---- comparisons -----------------------------------------------------------------------------------------------------------
def cmp_elem(out: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> dict:
    """fp32 elementwise class: every element within its own tolerance (`ulps` = the worst err / tol)."""
    o, r = out.detach().to(F64).reshape(-1), ref.to(F64).reshape(-1)
    err = (o - r).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    worst = float((err / tol.to(F64).reshape(-1).clamp_min(1e-300)).max()) if r.numel() else 0.0
    rn, rmax = float(r.norm()), float(r.abs().max()) if r.numel() else 0.0
    emax = float(err.max()) if r.numel() else 0.0
    rel = float(err.norm()) / rn if rn > 0 else (0.0 if emax == 0 else math.inf)
    mrel = emax / rmax if rmax > 0 else (0.0 if emax == 0 else math.inf)
    return dict(cls="elem", rel_l2=rel, max_rel=mrel, ulps=worst, ok=worst <= 1.0)


def cmp_same(out: torch.Tensor, ref: torch.Tensor) -> dict:
    """bit for bit, any dtype of 2, 4 or 8 bytes (NaNs compare by their bits)."""
    o, r = out.detach().contiguous().reshape(-1), ref.detach().contiguous().reshape(-1)
    assert o.dtype == r.dtype and o.numel() == r.numel(), (o.dtype, r.dtype, o.numel(), r.numel())
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[o.element_size()]
    bad = int((o.view(it) != r.view(it)).sum())
    return dict(cls="exact", rel_l2=0.0 if bad == 0 else math.inf, max_rel=0.0 if bad == 0 else math.inf, ulps=float("nan"),
                ok=bad == 0, mismatches=bad)


def bf16_tol(ref: torch.Tensor, extra: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The per-element tolerance cmp_bf16 holds an output to: BF16_ULPS ulps of the float64 reference + BF16_FLOOR rms(ref)
    [+ extra], in the reference's shape.  Two outputs of one problem that each pass lie within tol_a + tol_b of each other."""
    r = ref.to(F64)
    rms = float(r.pow(2).mean().sqrt()) if r.numel() else 0.0
    tol = BF16_ULPS * bf16_ulp(r) + BF16_FLOOR * rms
    return tol if extra is None else tol + extra.to(F64).reshape(tol.shape)


def _keep_tol(ctx: dict, row: dict, ref: torch.Tensor, extra: Optional[torch.Tensor]) -> dict:
    """With audit_forward(keep_tol=True) a bf16 conv output's row carries its per-element tolerance (NDHWC, float64): the
    op tests compare two kernel forms of one problem element by element with it."""
    if ctx.get("keep_tol"):
        row["tol"] = bf16_tol(ref, extra)
    return row


def require_ok(label: str, rows: List[dict], missing: List[str]) -> None:
    """What an op test asserts of an audited program: every launch has a record (or a SKIP entry), something was audited and
    every row is inside its bound.  Prints one line per row (the log of profiles/conv_op_audit.log)."""
    for r in rows:
        ulps = "-" if r["ulps"] != r["ulps"] else f"{r['ulps']:.3f}"
        print(f"[conv-op-audit] {label} | {r['kernel']} | {r['name']}.{r['what']} {r['shape']} | {r['cls']} | "
              f"rel-L2 {r['rel_l2']:.3e} | max/max|ref| {r['max_rel']:.3e} | worst/tol {ulps} | {'ok' if r['ok'] else 'FAIL'}")
    assert not missing, f"{label}: launches without an audit record or a SKIP entry: {sorted(set(missing))}"
    assert rows, f"{label}: no launch was audited"
    bad = [{k: v for k, v in r.items() if k != "tol"} for r in rows if not r["ok"]]
    assert not bad, f"{label}: {len(bad)} audited outputs out of bounds, first: {bad[:3]}"


# ---- float64 convolution in depth slabs --------------------------------------------------------------------------------------
def slab_budget(device=None) -> int:
    """Bytes the columns of one float64 conv call may take: SLAB_BUDGET_FRACTION of what torch.cuda.mem_get_info reports free."""
    free, _ = torch.cuda.mem_get_info(device)
    return int(free * SLAB_BUDGET_FRACTION)


def conv64(x: torch.Tensor, w: torch.Tensor, stride, padding, transposed: bool, budget: int) -> torch.Tensor:
    """float64 conv3d / conv_transpose3d of x (n, c, d, h, w) with depth stride 1 and a 'same' depth kernel (kd = 2 pd + 1), in
    depth slabs with a pd-slice overlap.  torch's non-MIOpen path materialises columns of taps * channels * plane * 8 bytes per
    depth slice; a slab holds as many slices as `budget` bytes of columns allow (at least one).  Output slice j reads input
    slices j - pd .. j + pd only, so a slab computed from its own slices plus pd neighbours on each side (zeros beyond the
    volume's ends, as the padding gives) holds the same sums as one call."""
    x, w = x.to(F64), w.to(F64)
    n, c, d, h, wd = x.shape
    kd, kh, kw = w.shape[2:]
    pd, ph, pw = padding
    sh, sw = stride
    if kd != 2 * pd + 1:
        raise ValueError("conv64 slabs along depth: the depth kernel must be 'same' (kd = 2 pd + 1, stride 1)")
    if transposed:
        cout, ho, wo = w.shape[1], (h - 1) * sh - 2 * ph + kh, (wd - 1) * sw - 2 * pw + kw
        per_slice = kd * kh * kw * cout * h * wd * 8
    else:
        cout, ho, wo = w.shape[0], (h + 2 * ph - kh) // sh + 1, (wd + 2 * pw - kw) // sw + 1
        per_slice = kd * kh * kw * c * ho * wo * 8
    slab = max(1, min(d, int(budget) // max(per_slice, 1)))
    out = torch.empty((n, cout, d, ho, wo), dtype=F64, device=x.device)
    for a in range(0, d, slab):
        b = min(d, a + slab)
        lo, hi = max(a - pd, 0), min(b + pd, d)
        xs = x[:, :, lo:hi].contiguous()
        if transposed:
            y = F.conv_transpose3d(xs, w, stride=(1, sh, sw), padding=(pd, ph, pw))
        else:
            y = F.conv3d(xs, w, stride=(1, sh, sw), padding=(pd, ph, pw))
        out[:, :, a:b] = y[:, :, a - lo:a - lo + (b - a)]
        del xs, y
    return out


CONV_CACHE_BYTES = 2 << 30   # what a shared-reference cache may hold (operands + float64 results) before its oldest entries go


def _conv64_shared(ctx: dict, x: torch.Tensor, w: torch.Tensor, stride, padding, transposed: bool) -> torch.Tensor:
    """conv64, or -- with audit_forward(conv_cache={...}) -- the float64 result an earlier launch of the SAME problem got: the op
    tests run one case on many kernel forms, and the reference depends on the operands only.  A cached result is taken only if
    the launch's own operands equal the cached ones bit for bit (the weights are compared as fp32: every engine's weights are
    fp32 tensors before their rounding), so each launch is still judged from exactly what it read."""
    cache = ctx.get("conv_cache")
    if cache is None:
        return conv64(x, w, stride, padding, transposed, ctx["budget"])
    key = (tuple(x.shape), str(x.dtype), tuple(w.shape), tuple(stride), tuple(padding), bool(transposed))
    w32 = w.to(torch.float32)
    for cx, cw, cy in cache.setdefault("entries", {}).get(key, ()):
        if torch.equal(cx, x) and torch.equal(cw, w32):
            return cy.clone()
    y = conv64(x, w, stride, padding, transposed, ctx["budget"])
    ent = (x.contiguous().clone(), w32.clone(), y.clone())
    cache["entries"].setdefault(key, []).append(ent)
    cache["bytes"] = cache.get("bytes", 0) + sum(t.numel() * t.element_size() for t in ent)
    while cache["bytes"] > CONV_CACHE_BYTES and len(cache["entries"]) > 1:
        old = cache["entries"].pop(next(iter(cache["entries"])))
        cache["bytes"] -= sum(t.numel() * t.element_size() for e in old for t in e)
    return y


# ---- operand access ----------------------------------------------------------------------------------------------------------
def _val(v):
    return v() if callable(v) and not isinstance(v, torch.Tensor) else v


def _clone(v):
    v = _val(v)
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        return v.detach().clone()
    return act_ndhwc(v).clone()          # an Act: its logical NDHWC contents


# what `snapshot` copies before the op runs: everything the op reads, and every buffer of which it may only write a part
_INPUTS = {
    "conv_fwd": ("x1", "x2", "weight", "bias", "residual"),
    "gn_colsum": ("x",),
    "gn_finalize": ("colsum", "sums"),
    "gn_apply": ("x", "sums", "gamma", "beta", "tbias", "step_ptr", "residual"),
    "attn_depthsum": ("x",),
    "attn_normsum": ("depthsum", "sums", "gamma", "beta"),
    "attn_pv": ("depthsum", "sums", "gamma", "beta", "w", "bias"),
    "attn_softmax_rowsum": ("qk",),
    "attn_broadcast_add": ("x", "p", "rowsum"),
    "cfg_stats": ("eps", "scale", "step_ptr"),
    "cfg_stats_finalize": ("partials",),
    "cfg_combine": ("eps", "scale", "step_ptr", "stats"),
    "cfg_mirror": ("zin",),
    "sampler_step": ("z", "eps", "hist", "noise", "zin", "coef", "step_ptr", "nonfinite"),
    "sampler_advance": ("step_ptr",),
    "train.inputs": ("z0", "noise", "cond", "t_rows", "sqrt_ac", "sqrt_1mac", "xin", "w1", "b1", "w2", "b2", "w_all", "b_all"),
    "loss.fwd": ("pred", "noise", "mask", "norm"),
    "seam.z_to_bf16": ("z",),
}


def snapshot(rec: dict) -> dict:
    sn = {k: _clone(rec.get(k)) for k in _INPUTS[rec["kind"]]}
    if rec["kind"] == "conv_fwd" and rec.get("fuse_gn") is not None:
        g = rec["fuse_gn"]
        sn["gn_x"], sn["gn_sums"], sn["gn_gamma"], sn["gn_beta"] = (_clone(g[k]) for k in ("x", "sums", "gamma", "beta"))
    return sn


# ---- shared arithmetic -------------------------------------------------------------------------------------------------------
def _silu(z):
    return z * torch.sigmoid(z)


def _silu_err(z):
    """|silu_f(z) - silu(z)| for an exact fp32 argument z (csrc/ctsi_internal.h: z * rcp(1 + exp2(-1.4427 z)), hardware exp2 and
    rcp at 1 ulp = 2 EPS32 each).  The product t = -1.4427 z is rounded once, which moves exp2(t) by |t| ln 2 EPS32 < |z| EPS32
    relative; then exp2 (2), the add (1), rcp (2) and the final product (1): at most (6 + |z|) EPS32 of |silu(z)|.  The fp32
    engine's z / (1 + expf(-z)) has fewer roundings and the same bound."""
    return EPS32 * (6.0 + z.abs()) * _silu(z).abs()


def _gn_stats(sums, slot, n, groups, c, count, eps):
    """mean and rstd per channel, (n, c), from the fp64 (sum, sumsq) slot, as the kernels form them (in double)."""
    s = sums[slot:slot + n * groups * 2].to(F64).view(n, groups, 2)
    m = s[..., 0] / count
    var = (s[..., 1] / count - m * m).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + float(eps))
    cpg = c // groups
    return m.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)


def _affine(x, m, rstd, gamma, beta, k):
    """v = x sc + sh with sc = gamma rstd, sh = beta - m sc, and the fp32 error bound 2 k EPS32 (|x sc| + |m sc| + |beta|).
    k (bf16 engine) = 7: rstd -> fp32, gamma rstd, m -> fp32, m sc, beta - .., x sc, + sh.  k (fp32 engine) = 4: sc and sh are
    formed in double and rounded once each, then x sc, + sh."""
    shape = (x.shape[0],) + (1,) * (x.dim() - 2) + (x.shape[-1],)
    sc = (gamma.to(F64) * rstd).view(shape)
    msc = (m * gamma.to(F64) * rstd).view(shape)
    b = beta.to(F64).view((1,) * (x.dim() - 1) + (-1,))
    v = x * sc + (b - msc)
    return v, 2.0 * k * EPS32 * ((x * sc).abs() + msc.abs() + b.abs())


def _tile_sums(v: torch.Tensor, rows: int, tps: int) -> torch.Tensor:
    """v (n, items, c) -> (n, tps, c): sums over consecutive tiles of `rows` items (the last one ragged)."""
    n, items, c = v.shape
    pad = tps * rows - items
    assert 0 <= pad < rows, (items, rows, tps)
    if pad:
        v = torch.cat([v, v.new_zeros((n, pad, c))], 1)
    return v.view(n, tps, rows, c).sum(2)


def _slab_totals(colsum: torch.Tensor, off: int, n: int, tps: int, cpad: int, nclass: int, c: int):
    """A column-sum slab [2][nclass * n * tps][cpad] at `off` -> (sum, sumsq) per (sample, channel), float64; tiles of class k of
    sample i start at (k * n + i) * tps (include/ctsi.h)."""
    slab = nclass * n * tps * cpad
    both = colsum[off:off + 2 * slab].to(F64).view(2, nclass, n, tps, cpad)
    t = both.sum((1, 3))[..., :c]
    return t[0], t[1]


# ---- references and checks, one function per kind -----------------------------------------------------------------------------
def _chk_conv_fwd(rec, sn, R, ctx):
    f32 = bool(rec.get("f32"))
    x = sn["x1"] if sn["x2"] is None else torch.cat([sn["x1"], sn["x2"]], -1)
    if rec["cin_w"] is not None:
        x = x[..., :rec["cin_w"]]            # the remaining channels are layout padding: the weights do not carry them
    w = sn["weight"].detach().to(x.device, torch.float32)      # (an op test may hand the engine a host tensor)
    w = w.to(F64) if f32 else w.to(torch.bfloat16).to(F64)     # the bf16 kernels read a bf16 image (round to nearest even)
    y = _conv64_shared(ctx, x.permute(0, 4, 1, 2, 3), w, rec["s"], rec["p"], rec["transposed"])
    del x
    if sn["bias"] is not None:
        y += sn["bias"].to(F64)[:y.shape[1]].view(1, -1, 1, 1, 1)
    rows = []
    if rec["stats"] is not None:           # the slab holds sums of the unrounded result (csrc/conv_mfma.hip epilogue)
        st = rec["stats"]
        s1, s2 = _slab_totals(_val(rec["colsum"]), 0, y.shape[0], st["tps"], st["cpad"], st["nclass"], y.shape[1])
        rows.append(R("colsum1", s1, cmp_f32(s1, y.sum((2, 3, 4)))))
        rows.append(R("colsum2", s2, cmp_f32(s2, (y * y).sum((2, 3, 4)))))
    if sn.get("residual") is not None:
        y += sn["residual"].to(F64).permute(0, 4, 1, 2, 3)
    if rec["act"] == 1:
        y = torch.tanh(y)
    elif rec["act"] == 2:
        # ReLU (planar halo-tile plans, bf16 output, no sums; csrc/conv3_halo_k32_body.inc, `out_v`): __builtin_fmaxf(v, 0) on
        # the fp32 accumulator, then the one rounding to bf16.  max(., 0) is exact and commutes with a monotone rounding, so the
        # output is still one rounding of the fp32 sum: no per-element term.  Where the float64 result is within the fp32
        # accumulation error of zero the two may take different sides; that is what BF16_FLOOR covers at every near-zero element.
        y = torch.relu(y)
    elif rec["act"] != 0:
        raise ValueError(f"conv_fwd: no reference for the epilogue act = {rec['act']}")
    if rec["f32_out"] is not None:          # fp32 with element strides: every element of the tensor is one output
        o = rec["f32_out"]
        assert o.numel() == y.numel(), "the strided output must cover its tensor"
        view = torch.as_strided(o, tuple(y.shape), rec["f32_strides"])
        return rows + [R("y", view, cmp_f32(view, y))]
    out = act_ndhwc(rec["out"])
    y = y.permute(0, 2, 3, 4, 1)
    if f32:
        return rows + [R("y", out, cmp_f32(out, y))]
    g = rec["fuse_gn"]
    if g is None:
        return rows + [_keep_tol(ctx, R("y", out, cmp_bf16(out, y)), y, None)]
    h = sn["gn_x"].to(F64)
    m, rstd = _gn_stats(sn["gn_sums"], g["slot"], h.shape[0], g["groups"], h.shape[-1], float(g["count"]), g["eps"])
    v, e = _affine(h, m, rstd, sn["gn_gamma"], sn["gn_beta"], 7)
    pre = v + y
    e = e + 2.0 * 2 * EPS32 * (v.abs() + y.abs())          # the two adds of the tail
    if not rec["stream_tail"]:
        e = e + FUSE_R_ULPS * bf16_ulp(y)
    if g["silu"]:
        e = SILU_SLOPE * e + _silu_err(pre)
        pre = _silu(pre)
    return rows + [_keep_tol(ctx, R("y", out, cmp_bf16(out, pre, extra=e)), pre, e)]


def _chk_gn_colsum(rec, sn, R, ctx):
    x = sn["x"].to(F64)
    n, c = x.shape[0], x.shape[-1]
    X = x.reshape(n, -1, c)
    tps, rows_ = rec["tps"], rec["tile_rows"]
    got = _val(rec["colsum"])[:2 * n * tps * c].to(F64).view(2, n, tps, c)
    return [R("colsum1", got[0], cmp_f32(got[0], _tile_sums(X, rows_, tps))),
            R("colsum2", got[1], cmp_f32(got[1], _tile_sums(X * X, rows_, tps)))]


def _chk_gn_finalize(rec, sn, R, ctx):
    n, c, groups, slot = rec["n"], rec["c"], rec["groups"], rec["slot"]
    ref = torch.zeros((n, groups, 2), dtype=F64, device=sn["colsum"].device)
    for pt in rec["parts"]:
        s1, s2 = _slab_totals(sn["colsum"], pt["off"], n, pt["tps"], pt["cpad"], pt["nclass"], c)
        ref[..., 0] += s1.view(n, groups, -1).sum(-1)
        ref[..., 1] += s2.view(n, groups, -1).sum(-1)
    sums = _val(rec["sums"])
    got = sums[slot:slot + n * groups * 2].view(n, groups, 2)
    rows = [R("sum", got[..., 0], cmp_f32(got[..., 0], ref[..., 0])), R("sumsq", got[..., 1], cmp_f32(got[..., 1], ref[..., 1]))]
    keep = torch.ones(sums.numel(), dtype=torch.bool, device=sums.device)
    keep[slot:slot + n * groups * 2] = False
    return rows + [R("others", sums[keep], cmp_same(sums[keep], sn["sums"][keep]))]


def _gn_chain(rec, sn, x, k_aff):
    n, c = x.shape[0], x.shape[-1]
    count = float((c // rec["groups"]) * rec["d_stat"] * x.shape[2] * x.shape[3])
    m, rstd = _gn_stats(sn["sums"], rec["slot"], n, rec["groups"], c, count, rec["eps"])
    v, e = _affine(x, m, rstd, sn["gamma"], sn["beta"], k_aff)
    if rec["silu_pre"]:
        e = SILU_SLOPE * e + _silu_err(v)
        v = _silu(v)
    if sn["tbias"] is not None:
        step = int(sn["step_ptr"][0]) if sn["step_ptr"] is not None else 0
        tb = sn["tbias"].reshape(-1)
        r0 = rec["tbias_off"] + step * n * rec["tbias_stride"]
        tbr = torch.stack([tb[r0 + i * rec["tbias_stride"]:r0 + i * rec["tbias_stride"] + c] for i in range(n)]).to(F64)
        v = v + tbr.view(n, 1, 1, 1, c)
        e = e + 2.0 * EPS32 * v.abs()                      # one add
    if sn["residual"] is not None:
        v = v + sn["residual"].to(F64)
        e = e + 2.0 * EPS32 * v.abs()                      # one add
    if rec["silu_post"]:
        e = SILU_SLOPE * e + _silu_err(v)
        v = _silu(v)
    return v, e


def _chk_gn_apply(rec, sn, R, ctx):
    out = act_ndhwc(rec["out"])
    if rec.get("f32"):
        v, e = _gn_chain(rec, sn, sn["x"].to(F64), 4)
        return [R("y", out, cmp_elem(out, v, e))]
    v, e = _gn_chain(rec, sn, sn["x"].to(F64), 7)
    return [R("y", out, cmp_bf16(out, v, extra=e))]


def _chk_attn_depthsum(rec, sn, R, ctx):
    x = sn["x"].to(F64)
    n, d, h, w, c = x.shape
    S = x.sum(1).reshape(n, h * w, c)
    S2 = (x * x).sum(1).reshape(n, h * w, c)
    ds = rec["depthsum"][:n * h * w * c].view(n, h * w, c)
    tps, pos = rec["tps"], rec["tile_pos"]
    got = _val(rec["colsum"])[:2 * n * tps * c].to(F64).view(2, n, tps, c)
    return [R("S", ds, cmp_f32(ds, S)), R("colsum1", got[0], cmp_f32(got[0], _tile_sums(S, pos, tps))),
            R("colsum2", got[1], cmp_f32(got[1], _tile_sums(S2, pos, tps)))]


def _normsum(rec, sn, n, hw, c, k):
    """xs = gamma rstd (S - D mean) + D beta and its fp32 bound 2 k EPS32 (|gamma rstd| (|S| + |D mean|) + |D beta|).  k = 8 in
    the bf16 engine (rstd -> fp32, mean -> fp32, D mean, S - .., gamma rstd, the product, D beta, the add); the fp32 engine
    evaluates the expression in double and rounds once: k = 1."""
    d = rec["d"]
    S = sn["depthsum"][:n * hw * c].to(F64).view(n, hw, c)
    m, rstd = _gn_stats(sn["sums"], rec["slot"], n, rec["groups"], c, float((c // rec["groups"]) * d * hw), rec["eps"])
    gr = (sn["gamma"].to(F64) * rstd).view(n, 1, c)
    dm = (d * m).view(n, 1, c)
    db = (d * sn["beta"].to(F64)).view(1, 1, c)
    return gr * (S - dm) + db, 2.0 * k * EPS32 * (gr.abs() * (S.abs() + dm.abs()) + db.abs())


def _chk_attn_normsum(rec, sn, R, ctx):
    out = act_ndhwc(rec["out"])
    n, _, h, w, c = out.shape
    if rec.get("f32"):
        xs, e = _normsum(rec, sn, n, h * w, c, 1)
        return [R("xs", out, cmp_elem(out, xs.view(out.shape), e))]
    xs, e = _normsum(rec, sn, n, h * w, c, 8)
    return [R("xs", out, cmp_bf16(out, xs.view(out.shape), extra=e.view(out.shape)))]


def _chk_attn_pv(rec, sn, R, ctx):
    out = act_ndhwc(rec["out"])
    n, _, h, w, c = out.shape
    xs, e = _normsum(rec, sn, n, h * w, c, 8)
    W = sn["w"].to(F64)                                     # bf16 [cout][cin], the kernel's own operand
    P = xs @ W.t() + sn["bias"].to(F64).view(1, 1, c)
    extra = (PV_XS_ULPS * bf16_ulp(xs) + e) @ W.abs().t()
    return [R("P", out, cmp_bf16(out, P.view(out.shape), extra=extra.view(out.shape)))]


def _chk_attn_softmax_rowsum(rec, sn, R, ctx):
    qk = sn["qk"].to(F64)
    n, d, h, w, c2 = qk.shape
    c, heads = c2 // 2, rec["heads"]
    hd = c // heads
    q = qk[..., :c].reshape(n, d, h * w, heads, hd)
    k = qk[..., c:].reshape(n, d, h * w, heads, hd)
    logits = torch.einsum("nqphc,nkphc->nphqk", q, k) * hd ** -0.5
    rs = torch.softmax(logits, -1).sum(-1).permute(0, 3, 1, 2)          # (n, d, hw, heads)
    got = rec["out"][:n * d * h * w * heads].view(n, d, h * w, heads)
    return [R("rowsum", got, cmp_f32(got, rs))]


def _chk_attn_broadcast_add(rec, sn, R, ctx):
    out = act_ndhwc(rec["out"])
    x, p = sn["x"].to(F64), sn["p"].to(F64)
    n, d, h, w, c = x.shape
    if sn["rowsum"] is not None:
        heads = rec["heads"]
        rs = sn["rowsum"][:n * d * h * w * heads].to(F64).view(n, d, h, w, heads).repeat_interleave(c // heads, -1)
        p = p * rs
    y = x + p
    if rec.get("f32"):
        return [R("y", out, cmp_elem(out, y, 2.0 * EPS32 * (x.abs() + p.abs())))]            # k = 1: the add
    return [R("y", out, cmp_bf16(out, y, extra=2.0 * 2 * EPS32 * (x.abs() + p.abs())))]       # k = 2: p rowsum, the add


def _cfg_row(sn):
    step = int(sn["step_ptr"][0]) if sn["step_ptr"] is not None else 0
    return float(sn["scale"][step, 0]), float(sn["scale"][step, 1])


def _chk_cfg_stats(rec, sn, R, ctx):
    n, bps = rec["n"], rec["bps"]
    s, _ = _cfg_row(sn)
    e = sn["eps"].to(F64).reshape(2 * n, -1)
    ec, eu = e[:n], e[n:]
    eg = eu + s * (ec - eu)
    ref = torch.stack([ec.sum(1), (ec * ec).sum(1), eg.sum(1), (eg * eg).sum(1)], 1)
    got = rec["partials"].view(n, bps, 4).sum(1)
    names = ("sum_c", "sumsq_c", "sum_g", "sumsq_g")
    return [R(names[k], got[:, k], cmp_f32(got[:, k], ref[:, k])) for k in range(4)]


def _chk_cfg_stats_finalize(rec, sn, R, ctx):
    n, bps, count = rec["n"], rec["bps"], float(rec["count"])
    t = sn["partials"].view(n, bps, 4).sum(1)
    vc = ((t[:, 1] - t[:, 0] ** 2 / count) / (count - 1.0)).clamp_min(0)
    vg = ((t[:, 3] - t[:, 2] ** 2 / count) / (count - 1.0)).clamp_min(0)
    sc, sg = vc.sqrt(), vg.sqrt()
    ref = torch.stack([sc, sg, torch.where(sg == 0, torch.ones_like(sg), sc / sg), torch.full_like(sc, count)], 1)
    return [R("stats", rec["stats"], cmp_f32(rec["stats"], ref))]


def _chk_cfg_combine(rec, sn, R, ctx):
    n = rec["n"]
    s, phi = _cfg_row(sn)
    e = sn["eps"].to(F64)
    ec, eu = e[:n], e[n:]
    shape = (n,) + (1,) * (e.dim() - 1)
    m = torch.ones(shape, dtype=F64, device=e.device)
    if sn["stats"] is not None and phi != 0.0:
        m = (phi * sn["stats"][:, 2] + (1.0 - phi)).to(torch.float32).to(F64).view(shape)     # formed in double, rounded once
    ref = (eu + s * (ec - eu)) * m
    # k = 4: c - u, the fma, m -> fp32, the product with m
    tol = 2.0 * 4 * EPS32 * m.abs() * (abs(s) * (ec.abs() + eu.abs()) + eu.abs())
    got = rec["eps"]
    return [R("eps_g", got[:n], cmp_elem(got[:n], ref, tol)), R("eps_u", got[n:], cmp_same(got[n:], sn["eps"][n:]))]


def _chk_cfg_mirror(rec, sn, R, ctx):
    zin, n, L = act_ndhwc(rec["zin"]), rec["n"], rec["L"]
    ref = sn["zin"].clone()
    ref[n:, ..., :L] = ref[:n, ..., :L]
    return [R("zin", zin, cmp_same(zin, ref))]


def _nan_to_num(v):
    v = torch.where(torch.isnan(v), torch.zeros_like(v), v)
    v = torch.where(v == math.inf, torch.ones_like(v), v)
    return torch.where(v == -math.inf, -torch.ones_like(v), v)


def _count(v):
    return [int(torch.isnan(v).sum()), int(torch.isinf(v).sum())]


def _chk_sampler_step(rec, sn, R, ctx):
    """The four updates of csrc/elementwise.hip / csrc/multistep.hip in float64, with the fp32 bound 2 k EPS32 sum|terms| of
    each stored value (an intermediate's bound is carried into the terms it enters, scaled by its coefficient; clamps and
    nan_to_num do not widen it).  k, from the sources: ddim / ddpm 8 (c0 eps, z - .., the division, c2 z0, c3 .., their sum,
    c4 noise, the last add), dpmpp 5 (c0 z, one fma; ca z, two fmas), heun 7 (c0 z, two fmas; c4 z, three fmas)."""
    kind, n, L = rec["sampler"], rec["n"], rec["L"]
    step = int(sn["step_ptr"][0])
    cf = [float(v) for v in sn["coef"][step].to(F64)]
    z, ep = sn["z"].to(F64), sn["eps"][:n].to(F64)                  # NDHWC; a guided program's eps holds 2n rows
    nz = None if sn["noise"] is None else sn["noise"].to(F64).permute(0, 2, 3, 4, 1)
    hist = None if sn["hist"] is None else sn["hist"].to(F64)
    counts = [0] * 6
    guarded = kind != "ddpm"
    if guarded:
        counts[0:2] = _count(ep)
        ep = _nan_to_num(ep)
    new_hist, writes_z = None, True
    if kind in ("ddim", "ddpm"):
        c0, c1, c2, c3, c4 = cf[:5]
        z0 = (z - c0 * ep) / c1
        t0 = (z.abs() + (c0 * ep).abs()) / abs(c1)
        if guarded:
            counts[2:4] = _count(z0)
            z0 = _nan_to_num(z0).clamp(-10.0, 10.0)
            zn = c2 * z0 + c3 * ep
            terms = abs(c2) * t0 + (c3 * ep).abs()
        else:
            z0 = z0.clamp(-1.0, 1.0)
            zn = c2 * z0 + c3 * z
            terms = abs(c2) * t0 + (c3 * z).abs()
        if nz is not None:
            zn = zn + c4 * nz
            terms = terms + (c4 * nz).abs()
        k = 8
    elif kind == "dpmpp":
        c0, c1, ca, cb, cc = cf[:5]
        x0 = c0 * z - c1 * ep
        t0 = (c0 * z).abs() + (c1 * ep).abs()
        counts[2:4] = _count(x0)
        x0 = _nan_to_num(x0).clamp(-10.0, 10.0)
        zn = ca * z + cb * x0 + cc * hist
        terms = (ca * z).abs() + abs(cb) * t0 + (cc * hist).abs()
        new_hist, hist_terms, k = x0, t0, 5
    elif kind == "heun":
        c0, c1, c2, kd, c4, c5, c6, c7 = cf
        closing = kd != 0.0
        use_d1 = c1 != 0.0 or c6 != 0.0
        hh = hist if use_d1 else torch.zeros_like(z)
        dd = c0 * z + c1 * hh - c2 * ep
        t0 = (c0 * z).abs() + (c1 * hh).abs() + (c2 * ep).abs()
        counts[2:4] = _count(dd)
        dd = _nan_to_num(dd).clamp(-10.0, 10.0)
        zn = c4 * z + c5 * dd
        terms = (c4 * z).abs() + abs(c5) * t0
        if closing:
            zn = zn + c6 * hh
            terms = terms + (c6 * hh).abs()
            if nz is not None and c7 != 0.0:
                zn = zn + c7 * nz
                terms = terms + (c7 * nz).abs()
        else:
            new_hist, hist_terms, writes_z = dd, t0, False
        k = 7
    else:
        raise ValueError(f"unknown sampler kind {kind}")
    if guarded:
        counts[4:6] = _count(zn)
        zn = _nan_to_num(zn)
    tol = 2.0 * k * EPS32 * terms
    rows = []
    zout = rec["z"]
    if writes_z:
        rows.append(R("z", zout, cmp_elem(zout, zn, tol)))
    else:
        rows.append(R("z", zout, cmp_same(zout, sn["z"])))
    # the z half of the network input: rows [0, n), channels [0, L); everything else of that tensor stays as it was
    zin = act_ndhwc(rec["zin"])
    half = zin[:n, ..., :L]
    if zin.dtype == torch.bfloat16:
        if writes_z:
            rows.append(R("zin", half, cmp_exact(half.contiguous(), zout.to(torch.bfloat16))))
        else:
            rows.append(R("zin", half, cmp_bf16(half, zn, extra=tol)))
    else:
        rows.append(R("zin", half, cmp_same(half, zout) if writes_z else cmp_elem(half, zn, tol)))
    rest = sn["zin"].clone()
    rest[:n, ..., :L] = half
    rows.append(R("zin.rest", zin, cmp_same(zin, rest)))
    if rec["hist"] is not None:
        if new_hist is not None:
            rows.append(R("hist", rec["hist"], cmp_elem(rec["hist"], new_hist, 2.0 * k * EPS32 * hist_terms)))
        else:
            rows.append(R("hist", rec["hist"], cmp_same(rec["hist"], sn["hist"])))
    if rec["nonfinite"] is not None:
        ref = sn["nonfinite"].clone()
        ref[step] += torch.tensor(counts, dtype=ref.dtype, device=ref.device)
        rows.append(R("nonfinite", rec["nonfinite"], cmp_same(rec["nonfinite"], ref)))
    return rows


def _chk_sampler_advance(rec, sn, R, ctx):
    return [R("step", rec["step_ptr"], cmp_same(rec["step_ptr"], sn["step_ptr"] + 1))]


def _chk_train_inputs(rec, sn, R, ctx):
    L = rec["L"]
    xin = act_ndhwc(rec["xin"])
    t = sn["t_rows"].long()
    n = t.numel()
    a = sn["sqrt_ac"].to(F64)[t].view(n, 1, 1, 1, 1)
    s = sn["sqrt_1mac"].to(F64)[t].view(n, 1, 1, 1, 1)
    z0, nz = sn["z0"].to(F64).permute(0, 2, 3, 4, 1), sn["noise"].to(F64).permute(0, 2, 3, 4, 1)
    zt = a * z0 + s * nz
    rows = [R("z_t", xin[..., :L], cmp_bf16(xin[..., :L], zt, extra=2.0 * 3 * EPS32 * ((a * z0).abs() + (s * nz).abs()))),   # k = 3
            R("cond", xin[..., L:], cmp_exact(xin[..., L:].contiguous(), sn["cond"].permute(0, 2, 3, 4, 1).to(torch.bfloat16)))]
    # time embedding (csrc/elementwise.hip: four launches behind one op, every stage stored in te_scratch = [sincos | first
    # Linear, pre-activation | temb]): each stage is checked from the stage the kernels stored before it.
    # sincos: arg = t freq, freq = expf(-i step), step = logf(1e4) / (half - 1), all fp32.  Relative error of arg: the exponent
    # i step carries 3 roundings (logf, the division, the product), which move freq by 3 i step EPS32; expf (2 ulp = 4 EPS32)
    # and the product with t (1): (3 i step + 5) EPS32.  sin / cos move by at most |arg| times that, plus their own 2 ulp
    # (4 EPS32, |result| <= 1); doubled as every fp32-elementwise bound here.
    dim, td = rec["dim"], rec["time_dim"]
    half = dim // 2
    sc = rec["te_scratch"]
    sincos, lin1, temb = sc[:n * dim].view(n, dim), sc[n * dim:n * (dim + td)].view(n, td), sc[n * (dim + td):n * (dim + 2 * td)].view(n, td)
    i = torch.arange(half, dtype=F64, device=t.device)
    stepv = math.log(10000.0) / (half - 1)
    arg = sn["t_rows"].to(F64).view(n, 1) * torch.exp(-i * stepv).view(1, half)
    tol = 2.0 * EPS32 * (arg.abs() * (3.0 * i * stepv + 5.0).view(1, half) + 4.0)
    rows.append(R("sincos", sincos, cmp_elem(sincos, torch.cat([arg.sin(), arg.cos()], 1), torch.cat([tol, tol], 1))))
    w1, b1, w2, b2 = (sn[k].to(F64) for k in ("w1", "b1", "w2", "b2"))
    rows.append(R("lin1", lin1, cmp_f32(lin1, sincos.to(F64) @ w1.t() + b1)))
    rows.append(R("temb", temb, cmp_f32(temb, _silu(lin1.to(F64)) @ w2.t() + b2)))
    tb = _silu(temb.to(F64)) @ sn["w_all"].to(F64).t() + sn["b_all"].to(F64)
    return rows + [R("tbias", rec["tbias"], cmp_f32(rec["tbias"], tb))]


def _chk_loss_fwd(rec, sn, R, ctx):
    pred, noise = sn["pred"].to(F64), sn["noise"].to(F64).permute(0, 2, 3, 4, 1)      # (n, d, h, w, L)
    df2 = (pred - noise) ** 2
    if sn["mask"] is not None:
        df2 = df2 * sn["mask"].to(F64).permute(0, 2, 1)[:, :, None, None, :]
    per = df2.sum((1, 2, 3, 4))
    ref = torch.cat([(sn["norm"].to(F64) * per).sum().view(1), per])
    return [R("loss", rec["out"], cmp_f32(rec["out"], ref))]


def _chk_seam(rec, sn, R, ctx):
    out = act_ndhwc(rec["out"])
    return [R("z_bf16", out, cmp_exact(out, sn["z"].permute(0, 2, 3, 4, 1).to(torch.bfloat16).contiguous()))]


REFS = {
    "conv_fwd": _chk_conv_fwd,
    "gn_colsum": _chk_gn_colsum,
    "gn_finalize": _chk_gn_finalize,
    "gn_apply": _chk_gn_apply,
    "attn_depthsum": _chk_attn_depthsum,
    "attn_normsum": _chk_attn_normsum,
    "attn_pv": _chk_attn_pv,
    "attn_softmax_rowsum": _chk_attn_softmax_rowsum,
    "attn_broadcast_add": _chk_attn_broadcast_add,
    "cfg_stats": _chk_cfg_stats,
    "cfg_stats_finalize": _chk_cfg_stats_finalize,
    "cfg_combine": _chk_cfg_combine,
    "cfg_mirror": _chk_cfg_mirror,
    "sampler_step": _chk_sampler_step,
    "sampler_advance": _chk_sampler_advance,
    "train.inputs": _chk_train_inputs,
    "loss.fwd": _chk_loss_fwd,
    "seam.z_to_bf16": _chk_seam,
}


# ---- the runner ------------------------------------------------------------------------------------------------------------
def check(rec: dict, sn: dict, i: int, name: str, kern: str, ctx: dict) -> List[dict]:
    R = lambda what, out, res: _row(i, name, kern, what, tuple(out.shape), res)
    return REFS[rec["kind"]](rec, sn, R, ctx)


def unaccounted(prog, stop: Optional[int] = None) -> List[str]:
    """Names of ops[:stop] that have neither a forward record nor an entry in SKIP."""
    stop = len(prog.ops) if stop is None else stop
    return [prog.op_meta[i][0] for i in range(stop)
            if (prog.op_audit[i] is None or prog.op_audit[i].get("kind") not in REFS) and prog.op_meta[i][0] not in SKIP]


def audit_forward(prog, stop: Optional[int] = None, only: Optional[Iterable[int]] = None, budget: Optional[int] = None,
                  keep_tol: bool = False, conv_cache: Optional[dict] = None):
    """Run ops[:stop] one at a time (the inputs loaded by the caller), checking every op that has a record.  `only`: run and
    check just these op indices (one launch again on operands the caller set up, e.g. a sampler update on another coefficient
    row).  Returns (rows, unaccounted): one result row per checked output, and the names of ops with neither a record nor an
    entry in SKIP.  `keep_tol`: the rows of bf16 conv outputs also carry their per-element tolerance (`bf16_tol`);
    `conv_cache`: a dict the caller keeps, through which launches of one problem share its float64 conv (`_conv64_shared`)."""
    stop = len(prog.ops) if stop is None else stop
    idx = range(stop) if only is None else sorted(only)
    rows = []
    with prog.ctx.scope(), torch.backends.cudnn.flags(enabled=False), torch.no_grad():
        ctx = dict(budget=slab_budget(prog.ctx.device) if budget is None else budget, keep_tol=keep_tol, conv_cache=conv_cache)
        for i in idx:
            rec = prog.op_audit[i]
            name, _, kern = prog.op_meta[i]
            if rec is None or rec.get("kind") not in REFS:
                prog.ops[i]()
                continue
            sn = snapshot(rec)
            prog.ops[i]()
            rows.extend(check(rec, sn, i, name, kern, ctx))
            del sn
        prog.check_errors()
        torch.cuda.synchronize()
    return rows, unaccounted(prog, stop)
