"""Eager audit of a training program's backward pass, launch by launch (used by tests/test_gpu_train_backward_audit.py, and by
tests/loss_audit.py for the data-gradient, GroupNorm and head launches of the perceptual-loss and decode-gradient programs).

Every backward op of train_engine.UNetTrainProgram / vae_train_engine.VAETrainProgram carries an audit record
(`Program.op_audit`, parallel to `ops` / `op_meta`).  `audit_backward` runs the backward ops one at a time; for each op with a
record it copies the operands the op is about to read (including the previous contents of a destination it accumulates into --
pool buffers are reused later, so the copy is taken right there), runs the op, and recomputes its result from exactly those
operands in float64 torch on the device (cudnn / MIOpen off).  Each number therefore describes one launch: errors of earlier
launches do not compound.

Record kinds and what they compute (Acts are bf16 NDHWC; `out` / `dw` / ... are the op's destinations):
  chsum               out[c] = scale * sum_rows src[row, c]                                            (fp32, overwritten)
  wgrad               out[r, g, t] = scale * dW of R = conv3d(G, W, stride (1, s), padding p), R = r[:, :r_ch], G = g[:, :g_ch]
                      (fp32, overwritten; a transposed layer's gradient in the same terms: R = its input, G = its output grad)
  dgrad               op "convT": out = conv_transpose3d(g, W[:, w_ci]), op "conv": out = conv3d(g, W), W = bf16(weight())
                      (bf16, overwritten)
  add                 dst = bf16(fp32(dst) + fp32(src))                                                  (bf16, bit-exact)
  gn_bwd              GroupNorm (+SiLU, +residual, +SiLU) backward from x, dy, the fp64 statistics slot, gamma, beta:
                      dx (bf16, + add), g_out (bf16), dgamma / dbeta / dxsum / dtbias (fp32, overwritten)
  depthsum            out = bf16(sum_d src)
  loss_bwd            out[b, v, ch] = bf16(2 norm[b] mask (pred - noise) gscale) for ch < L, 0 beyond
  linear_wgrad_multi  per layer dw = g^T x, db = scale * sum_rows g                                   (fp32, overwritten)
  linear_bwd_chain    the time-embedding backward: three fp32 Linear backward steps, each one's dx the next one's dy
  head_grad           mode 0: out = bf16(scale * g * (1 - y^2)), channels >= c zero; mode 1: out[:c] = bf16(out + scale * g)
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

F64 = torch.float64

# backward ops that may carry no record: pure memsets / copies only (none at present -- every launch computes something)
SKIP: Dict[str, str] = {}

# per output class: fp32 outputs (weight / bias / GroupNorm parameter gradients) and bf16 outputs (data gradients)
F32_REL_L2 = 1e-4
F32_MAX_REL = 1e-3
BF16_ULPS = 1.0
BF16_FLOOR = 1e-5          # absolute floor, x rms(ref)
BF16_REL_L2 = 4e-3         # against bf16(ref)
# Bounds set from the measurement (profiles/train_bwd_audit.log), each with its reason:
#  * BF16_FLOOR: the 1e-6 estimate failed the data gradients of the VAE convs at elements ~1e-5 rms(ref) across: fp32
#    accumulation over K = 27 x 128 .. 27 x 512 products leaves ~sqrt(K) 2^-24 ~ 4e-6 of the operand scale, one bf16 ulp of a
#    near-zero element is smaller than that.
#  * GroupNorm dx: pass 3 of ctsi_gn_bwd multiplies bf16(g) (the g buffer of pass 1, or its re-derivation rounded the same
#    way), so each element may also be off by rstd |gamma| ulp_bf16(g) -- a second bf16 rounding inside the launch, added to
#    that element's tolerance (GN_DX_G_ULPS of it).  rel-L2 against bf16(ref) keeps the plain 4e-3.
#  * GroupNorm dxsum (a conv bias gradient): formed in fp32 as rstd (gamma sum g - V S1 - S2 sum xhat), terms that cancel
#    within a group (the group sum of dx is exactly 0); measured 1.8e-3 rel-L2 on the small U-Nets.
GN_DX_G_ULPS = 1.0
GN_DXSUM_REL_L2 = 5e-3
GN_DXSUM_MAX_REL = 1e-2


# ---- operand access ------------------------------------------------------------------------------------------------------
def act_ndhwc(a) -> torch.Tensor:
    n, c, d, h, w = a.n, a.c, a.d, a.h, a.w
    if a.halo:
        raise ValueError("the audit handles programs without depth halos only")
    return a.t[:n * d * h * w * c].view(n, d, h, w, c)


def act_ncdhw64(a, ch: Optional[int] = None) -> torch.Tensor:
    t = act_ndhwc(a)
    if ch is not None:
        t = t[..., :ch]
    return t.permute(0, 4, 1, 2, 3).to(F64)


def _clone(v):
    if v is None:
        return None
    if callable(v) and not isinstance(v, torch.Tensor):
        v = v()
        if v is None:
            return None
    if isinstance(v, torch.Tensor):
        return v.detach().clone()
    return act_ndhwc(v).clone()          # an Act: its logical NDHWC contents


_INPUTS = {
    "chsum": ("src",),
    "wgrad": ("r", "g"),
    "dgrad": ("g",),
    "add": ("dst", "src"),
    "gn_bwd": ("x", "dy", "sums", "gamma", "beta", "residual", "add"),
    "depthsum": ("src",),
    "loss_bwd": ("pred", "noise", "mask", "norm", "gscale"),
    "head_grad": ("g", "y", "out"),
}


def snapshot(rec: dict) -> dict:
    kind = rec["kind"]
    if kind == "linear_wgrad_multi":
        return dict(layers=[dict(x=_clone(l["x"]), g=_clone(l["g"])) for l in rec["layers"]])
    if kind == "linear_bwd_chain":
        st = rec["steps"]
        return dict(steps=[dict(x=_clone(s["x"][:s["rows"] * s["cin"]]), w=_clone(s["w"])) for s in st],
                    dy0=_clone(st[0]["dy"]))
    if kind == "dgrad":
        return dict(g=_clone(rec["g"]), w=_clone(rec["weight"]))
    return {k: _clone(rec.get(k)) for k in _INPUTS[kind]}


# ---- comparisons ---------------------------------------------------------------------------------------------------------
def cmp_f32(out: torch.Tensor, ref: torch.Tensor, rel_l2: float = F32_REL_L2, max_rel: float = F32_MAX_REL) -> dict:
    o, r = out.detach().to(F64).reshape(-1), ref.to(F64).reshape(-1)
    err = (o - r).abs()
    rn, rmax = float(r.norm()), float(r.abs().max()) if r.numel() else 0.0
    rel = float((o - r).norm()) / rn if rn > 0 else (0.0 if float(err.max()) == 0 else math.inf)
    mrel = float(err.max()) / rmax if rmax > 0 else (0.0 if float(err.max()) == 0 else math.inf)
    ok = rel <= rel_l2 and mrel <= max_rel
    return dict(cls="f32", rel_l2=rel, max_rel=mrel, ulps=float("nan"), ok=ok)


def bf16_ulp(r: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp at |r| (8 significant bits): 2^(e - 8) for |r| = m 2^e, m in [0.5, 1); 0 at r == 0."""
    _, e = torch.frexp(r)
    return torch.where(r == 0, torch.zeros_like(r), torch.ldexp(torch.ones_like(r), e - 8))


def cmp_bf16(out: torch.Tensor, ref: torch.Tensor, extra: Optional[torch.Tensor] = None) -> dict:
    """`extra`: a per-element tolerance added to one ulp (a documented intermediate rounding inside the launch)."""
    o, r = out.detach().to(F64).reshape(-1), ref.to(F64).reshape(-1)
    err = (o - r).abs()
    rms = float(r.pow(2).mean().sqrt()) if r.numel() else 0.0
    tol = bf16_ulp(r) + BF16_FLOOR * rms
    if extra is not None:
        tol = tol + extra.reshape(-1)
    ulps = float((err / tol.clamp_min(1e-300)).max()) if r.numel() else 0.0
    rb = r.to(torch.bfloat16).to(F64)
    rbn = float(rb.norm())
    rel = float((o - rb).norm()) / rbn if rbn > 0 else (0.0 if float(err.max()) == 0 else math.inf)
    rmax = float(r.abs().max()) if r.numel() else 0.0
    mrel = float(err.max()) / rmax if rmax > 0 else (0.0 if float(err.max()) == 0 else math.inf)
    ok = ulps <= BF16_ULPS and rel <= BF16_REL_L2
    return dict(cls="bf16", rel_l2=rel, max_rel=mrel, ulps=ulps, ok=ok)


def cmp_exact(out: torch.Tensor, ref_bf16: torch.Tensor) -> dict:
    o, r = out.reshape(-1), ref_bf16.reshape(-1)
    bad = int((o.view(torch.int16) != r.view(torch.int16)).sum())
    d = cmp_bf16(o, r.to(F64))
    d.update(cls="exact", ok=bad == 0, mismatches=bad)
    return d


# ---- references ----------------------------------------------------------------------------------------------------------
def _ncdhw(t: torch.Tensor, ch: Optional[int] = None) -> torch.Tensor:
    if ch is not None:
        t = t[..., :ch]
    return t.permute(0, 4, 1, 2, 3).to(F64)


def ref_wgrad(rec, sn):
    k, s, p = tuple(rec["k"]), tuple(rec["s"]), tuple(rec["p"])
    R, G = _ncdhw(sn["r"], rec["r_ch"]), _ncdhw(sn["g"], rec["g_ch"])
    if k == (1, 1, 1) and s == (1, 1):
        dw = torch.einsum("nrdhw,ngdhw->rg", R, G).reshape(R.shape[1], G.shape[1], 1)
    else:
        dw = torch.nn.grad.conv3d_weight(G, (R.shape[1], G.shape[1]) + k, R, stride=(1,) + s, padding=p)
        dw = dw.reshape(R.shape[1], G.shape[1], -1)
    return dw * rec["scale"]


def ref_dgrad(rec, sn):
    k, s, p = tuple(rec["k"]), tuple(rec["s"]), tuple(rec["p"])
    W = sn["w"].to(torch.bfloat16).to(F64)          # the conv kernels read bf16 weight images (round to nearest even)
    if rec["w_ci"] is not None:
        c0, cn = rec["w_ci"]
        W = W[:, c0:c0 + cn]
    if rec["op"] == "convT":
        g = _ncdhw(sn["g"], W.shape[0])
        y = F.conv_transpose3d(g, W, stride=(1,) + s, padding=p)
    else:
        g = _ncdhw(sn["g"], W.shape[1])
        y = F.conv3d(g, W, stride=(1,) + s, padding=p)
    return y.permute(0, 2, 3, 4, 1)                 # NDHWC like the output Act


def _silu(z):
    return z * torch.sigmoid(z)


def _silu_grad(z):
    sg = torch.sigmoid(z)
    return sg * (1 + z * (1 - sg))


def ref_gn_bwd(rec, sn):
    x = sn["x"].to(F64)
    n, d, h, w, c = x.shape
    vox = d * h * w
    X = x.reshape(n, vox, c)
    dy = sn["dy"].to(F64)
    DY = (dy.reshape(n, 1, h * w, c).expand(n, d, h * w, c) if rec["bcast"] else dy).reshape(n, vox, c)
    groups, cpg = rec["groups"], c // rec["groups"]
    sums = sn["sums"].reshape(n, groups, 2)
    cnt = float(cpg * vox)
    m = sums[..., 0] / cnt
    var = (sums[..., 1] / cnt - m * m).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + rec["eps"])
    mc = m.repeat_interleave(cpg, 1)[:, None, :]
    rc = rstd.repeat_interleave(cpg, 1)[:, None, :]
    gam, bet = sn["gamma"].to(F64), sn["beta"].to(F64)
    xh = (X - mc) * rc
    hh = xh * gam + bet
    gc = DY
    if rec["silu_post"]:
        cc = _silu(hh) if rec["silu_pre"] else hh
        if sn["residual"] is not None:
            cc = cc + sn["residual"].to(F64).reshape(n, vox, c)
        gc = gc * _silu_grad(cc)
    g = gc * _silu_grad(hh) if rec["silu_pre"] else gc
    s1 = (gam * g).reshape(n, vox, groups, cpg).sum((1, 3)) / cnt
    s2 = (gam * g * xh).reshape(n, vox, groups, cpg).sum((1, 3)) / cnt
    dx = rc * (gam * g - s1.repeat_interleave(cpg, 1)[:, None, :] - xh * s2.repeat_interleave(cpg, 1)[:, None, :])
    out = dict(dgamma=(g * xh).sum((0, 1)), dbeta=g.sum((0, 1)), dxsum=dx.sum((0, 1)), dtbias=gc.sum(1),
               g_out=g.reshape(n, d, h, w, c), dx_gtol=(GN_DX_G_ULPS * rc * gam.abs() * bf16_ulp(g)).reshape(n, d, h, w, c))
    if sn["add"] is not None:
        dx = dx + sn["add"].to(F64).reshape(n, vox, c)
    out["dx"] = dx.reshape(n, d, h, w, c)
    return out


def ref_loss_bwd(rec, sn, Lp):
    pred, noise = sn["pred"].to(F64), sn["noise"].to(F64)      # (n, d, h, w, L) / (n, L, d, h, w)
    n, d, h, w, L = pred.shape
    df = pred - noise.permute(0, 2, 3, 4, 1)
    m = 1.0 if sn["mask"] is None else sn["mask"].to(F64).permute(0, 2, 1)[:, :, None, None, :]
    v = 2.0 * sn["norm"].to(F64).view(n, 1, 1, 1, 1) * m * df * sn["gscale"].to(F64).view(1)
    out = torch.zeros((n, d, h, w, Lp), dtype=F64, device=pred.device)
    out[..., :L] = v
    return out


# ---- the runner ----------------------------------------------------------------------------------------------------------
def _row(i, name, kern, what, shape, res):
    res.update(op=i, name=name, kernel=kern or "-", what=what, shape="x".join(str(v) for v in shape))
    return res


def check(rec: dict, sn: dict, i: int, name: str, kern: str) -> List[dict]:
    kind = rec["kind"]
    R = lambda what, out, res: _row(i, name, kern, what, tuple(out.shape), res)
    if kind == "chsum":
        src = sn["src"]
        ref = src.reshape(-1, src.shape[-1]).to(F64).sum(0)[:rec["out"].numel()] * rec["scale"]
        return [R("db", rec["out"], cmp_f32(rec["out"], ref))]
    if kind == "wgrad":
        return [R("dW", rec["out"], cmp_f32(rec["out"], ref_wgrad(rec, sn)))]
    if kind == "dgrad":
        out = act_ndhwc(rec["out"])
        return [R("dx", out, cmp_bf16(out, ref_dgrad(rec, sn)))]
    if kind == "add":
        ref = (sn["dst"].float() + sn["src"].float()).to(torch.bfloat16)
        out = act_ndhwc(rec["dst"])
        return [R("sum", out, cmp_exact(out, ref))]
    if kind == "gn_bwd":
        ref = ref_gn_bwd(rec, sn)
        rows = [R("dx", act_ndhwc(rec["dx"]), cmp_bf16(act_ndhwc(rec["dx"]), ref["dx"], extra=ref["dx_gtol"]))]
        if rec["g_out"] is not None:
            go = act_ndhwc(rec["g_out"])
            rows.append(R("g", go, cmp_bf16(go, ref["g_out"])))
        rows.append(R("dgamma", rec["dgamma"], cmp_f32(rec["dgamma"], ref["dgamma"])))
        rows.append(R("dbeta", rec["dbeta"], cmp_f32(rec["dbeta"], ref["dbeta"])))
        if rec["dxsum"] is not None:
            o = rec["dxsum"][:ref["dxsum"].numel()]
            rows.append(R("dxsum", o, cmp_f32(o, ref["dxsum"], GN_DXSUM_REL_L2, GN_DXSUM_MAX_REL)))
        if rec["dtbias"] is not None:
            rows.append(R("dtbias", rec["dtbias"], cmp_f32(rec["dtbias"], ref["dtbias"])))
        return rows
    if kind == "depthsum":
        out = act_ndhwc(rec["out"])
        return [R("dP", out, cmp_bf16(out, sn["src"].to(F64).sum(1, keepdim=True)))]
    if kind == "loss_bwd":
        out = act_ndhwc(rec["out"])
        return [R("deps", out, cmp_bf16(out, ref_loss_bwd(rec, sn, out.shape[-1])))]
    if kind == "linear_wgrad_multi":
        rows = []
        for j, (l, s) in enumerate(zip(rec["layers"], sn["layers"])):
            X = s["x"].reshape(-1, s["x"].shape[-1]).to(F64)
            G = s["g"].reshape(-1, s["g"].shape[-1]).to(F64)
            rows.append(R(f"dW[{j}]", l["dw"], cmp_f32(l["dw"], G.t() @ X)))
            if l["db"] is not None:
                rows.append(R(f"db[{j}]", l["db"], cmp_f32(l["db"], G.sum(0) * l["scale"])))
        return rows
    if kind == "linear_bwd_chain":
        rows, dy = [], sn["dy0"].to(F64)
        for j, (st, s) in enumerate(zip(rec["steps"], sn["steps"])):
            X = s["x"].reshape(st["rows"], st["cin"]).to(F64)
            W = s["w"].reshape(st["cout"], st["cin"]).to(F64)
            DY = dy.reshape(st["rows"], st["cout"])
            a = _silu(X) if st["silu_in"] else X
            rows.append(R(f"dW[{j}]", st["dw"], cmp_f32(st["dw"], DY.t() @ a)))
            rows.append(R(f"db[{j}]", st["db"], cmp_f32(st["db"], DY.sum(0))))
            if st["dx"] is not None:
                dx = DY @ W
                if st["silu_in"]:
                    dx = dx * _silu_grad(X)
                rows.append(R(f"dx[{j}]", st["dx"], cmp_f32(st["dx"].reshape(dx.shape), dx)))
                dy = dx
        return rows
    if kind == "head_grad":
        out = act_ndhwc(rec["out"])
        if rec["active"] is not None and not rec["active"]():
            res = cmp_exact(out, sn["out"])
            return [R("unchanged", out, res)]
        g = sn["g"].to(F64).permute(0, 2, 3, 4, 1)          # (n, d, h, w, c)
        c = g.shape[-1]
        ref = sn["out"].to(F64).clone()
        if rec["mode"] == 0:
            ref.zero_()
            ref[..., :c] = rec["scale"] * g * (1 - sn["y"].to(F64).permute(0, 2, 3, 4, 1) ** 2)
        else:
            ref[..., :c] = ref[..., :c] + rec["scale"] * g
        return [R("dy" if rec["mode"] == 0 else "dz", out, cmp_bf16(out, ref))]
    raise ValueError(f"unknown audit kind {kind}")


def audit_backward(prog, start: int):
    """Run ops[start:] (the backward pass, after a forward has run) one at a time, checking every op that has a record.
    Returns (rows, unaccounted): one result row per checked output, and the names of backward ops that have neither a record
    nor an entry in SKIP."""
    rows, missing = [], []
    with prog.ctx.scope(), torch.backends.cudnn.flags(enabled=False), torch.no_grad():
        for i in range(start, len(prog.ops)):
            rec = prog.op_audit[i]
            name, _, kern = prog.op_meta[i]
            if rec is None:
                if name not in SKIP:
                    missing.append(name)
                prog.ops[i]()
                continue
            sn = snapshot(rec)
            prog.ops[i]()
            rows.extend(check(rec, sn, i, name, kern))
            del sn
        prog.check_errors()
        torch.cuda.synchronize()
    return rows, missing


def format_table(title: str, rows: List[dict]) -> str:
    out = [title, f"{'op':>5} {'name':34s} {'kernel':30s} {'out':8s} {'shape':22s} {'class':5s} {'rel-L2':>10s} "
                  f"{'max/max|ref|':>12s} {'ulps':>6s}  ok"]
    for r in rows:
        ulps = "" if r["ulps"] != r["ulps"] else f"{r['ulps']:.2f}"
        extra = f" mismatches={r['mismatches']}" if r.get("mismatches") else ""
        out.append(f"{r['op']:5d} {r['name'][:34]:34s} {r['kernel'][:30]:30s} {r['what']:8s} {r['shape'][:22]:22s} "
                   f"{r['cls']:5s} {r['rel_l2']:10.3e} {r['max_rel']:12.3e} {ulps:>6s}  {'ok' if r['ok'] else 'FAIL'}{extra}")
    worst: Dict[tuple, dict] = {}
    for r in rows:
        key = (r["kernel"].split("_m")[0] if r["kernel"].startswith("conv_mfma") else r["kernel"], r["what"].split("[")[0], r["cls"])
        wv = worst.setdefault(key, dict(n=0, rel_l2=0.0, max_rel=0.0, ulps=0.0, fail=0))
        wv["n"] += 1
        wv["rel_l2"] = max(wv["rel_l2"], r["rel_l2"])
        wv["max_rel"] = max(wv["max_rel"], r["max_rel"])
        if r["ulps"] == r["ulps"]:
            wv["ulps"] = max(wv["ulps"], r["ulps"])
        wv["fail"] += 0 if r["ok"] else 1
    out.append("worst per (kernel, output, class):")
    for key, wv in sorted(worst.items()):
        out.append(f"  {key[0][:30]:30s} {key[1]:8s} {key[2]:5s} n={wv['n']:4d} rel-L2 {wv['rel_l2']:.3e} "
                   f"max/max|ref| {wv['max_rel']:.3e} ulps {wv['ulps']:.2f} failed {wv['fail']}")
    return "\n".join(out)
