"""Helpers for the `-m gpu` tests: drive single libctsi ops through engine.Program."""
import ctypes as C
import importlib
import os

import torch

from tests import fwd_audit as A

E = importlib.import_module("video-to-video-diffusion_amd.engine")
_ptr = E._ptr


def ctx():
    return E.Ctx.get(torch.device("cuda", 0))


def to_act(prog, x_ncdhw, c_pad=None):
    """fp32 NCDHW (any device) -> bf16 NDHWC Act on the engine stream."""
    n, c, d, h, w = x_ncdhw.shape
    ct = c if c_pad is None else c_pad
    buf = prog.persistent((n * d * h * w * ct,), torch.bfloat16, zero=True)
    xx = x_ncdhw.to(prog.ctx.device, torch.float32).contiguous()
    prog.lib.ncdhw_f32_to_ndhwc_bf16(_ptr(xx), _ptr(buf), n, c, d, h, w, ct, 0, prog.ctx.sptr)
    # kept alive with the program, but not in `keep`: that list holds the engine's own allocations (tests/poison.py checks them)
    prog.__dict__.setdefault("_test_inputs", []).append(xx)
    return E.Act(buf, n, ct, d, h, w)


def from_act(prog, a):
    out = torch.empty((a.n, a.c, a.d, a.h, a.w), dtype=torch.float32, device=prog.ctx.device)
    prog.lib.ndhwc_bf16_to_ncdhw_f32(_ptr(a.t), _ptr(out), a.n, a.c, a.d, a.h, a.w, prog.ctx.sptr)
    return out


_CONV64 = {}          # float64 conv references, shared by the kernel forms of one case (fwd_audit._conv64_shared)


def audit_label(what=""):
    """The running test's id (pytest sets PYTEST_CURRENT_TEST) [+ what]: the label of the printed audit rows."""
    test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0].split("::", 1)[-1]
    return f"{test} {what}".strip()


def audit_program(prog, what=""):
    """Run `prog` (laid out, inputs loaded) launch by launch under fwd_audit.audit_forward and require every row `ok` and every
    launch accounted for.  Returns (rows, tol): `tol` is the per-element tolerance of the last bf16 conv output (fp32 NCDHW on
    the cpu, None if there is none) -- two forms of one problem lie within tol_a + tol_b of each other."""
    rows, missing = A.audit_forward(prog, keep_tol=True, conv_cache=_CONV64)
    kernels = "+".join(m[2] for m, r in zip(prog.op_meta, prog.op_audit) if r is not None and r.get("kind") == "conv_fwd")
    A.require_ok(audit_label(what or kernels), rows, missing)
    tols = [r.pop("tol") for r in rows if "tol" in r]
    return rows, (tols[-1].permute(0, 4, 1, 2, 3).contiguous().cpu() if tols else None)


def within_tolerances(y, y2, tol, tol2):
    """|y - y2| <= tol + tol2 per element: both lie within their tolerance of the same float64 reference."""
    return bool(((y.double() - y2.double()).abs() <= tol + tol2).all())


def run_conv(x1, x2, weight, bias, *, transposed=False, k=(3, 3, 3), s=(1, 1), p=(1, 1, 1), f32=False, act=0,
             c1_pad=None, cin_w=None, want_stats=False, groups=None, audit=False):
    """Returns (y fp32 NCDHW on cpu, sums or None).  `audit`: the program runs launch by launch under the forward audit
    (`audit_program`), every row must be `ok`; returns (y, sums, tol) with tol as `audit_program` returns it."""
    c = ctx()
    with c.scope():
        prog = E.Program(c)
        a1 = to_act(prog, x1, c1_pad)
        a2 = to_act(prog, x2) if x2 is not None else None
        cout = weight.shape[1] if transposed else weight.shape[0]
        kw = dict(transposed=transposed, k=k, s=s, p=p, cout=cout, cin_w=cin_w, want_stats=want_stats, act=act)
        slot = None
        prog.zero_gn_op()
        if f32:
            # probe output dims with a throw-away plan
            desc = E.ConvDesc(int(transposed), k[0], k[1], k[2], s[0], s[1], p[0], p[1], p[2], a1.n, a1.c,
                              0 if a2 is None else a2.c, cout, a1.d, a1.h, a1.w, 0)
            plan = C.c_void_p()
            prog.lib.conv_plan_create(C.byref(plan), C.byref(desc))
            do, ho, wo = C.c_int(), C.c_int(), C.c_int()
            prog.lib.conv_plan_out_dims(plan, C.byref(do), C.byref(ho), C.byref(wo))
            prog.lib.conv_plan_destroy(plan)
            do, ho, wo = do.value, ho.value, wo.value
            y = prog.persistent((a1.n, cout, do, ho, wo), torch.float32, zero=True)
            vox = do * ho * wo
            prog.conv("t", lambda: weight, (lambda: bias) if bias is not None else None, a1, a2, f32_out=y,
                      f32_strides=(cout * vox, vox, ho * wo, wo, 1), **kw)
            out_act = None
        else:
            out_act, st = prog.conv("t", lambda: weight, (lambda: bias) if bias is not None else None, a1, a2, **kw)
            if want_stats:
                slot = prog.gn_finalize(out_act, groups, st)
        prog.finalize_layout()
        if audit:
            _, tol = audit_program(prog)
        else:
            prog.run()
        res = y.clone() if f32 else from_act(prog, out_act)
        sums = None
        if slot is not None:
            sums = prog._gn_sums[slot:slot + out_act.n * groups * 2].clone().reshape(out_act.n, groups, 2)
    torch.cuda.synchronize()
    if audit:
        return res.cpu(), (sums.cpu() if sums is not None else None), tol
    return res.cpu(), (sums.cpu() if sums is not None else None)
