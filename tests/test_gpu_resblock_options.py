"""GPU: the ResBlock options -- scale-shift time conditioning and dropout on conv2's input (csrc/norm_act.hip, csrc/f32_ops.hip,
csrc/norm_bwd.hip)
-- from the kernels up to sampling and training, against tests/resblock_restatement.py.

Kernels: float64 from the kernel's own operands.
  forward bf16   `cmp_bf16` of tests/train_audit.py (one bf16 ulp + its floor, rel-L2 4e-3 against bf16(ref)).  The pass is fp32 from
                 the bf16 load to the single rounding at the store (coefficients, the hardware exp2 / rcp of SiLU at 1 ulp each, the
                 dropout scale): ~1e-6 relative, under the floor -- no `extra` term.
  forward fp32   `cmp_f32`.
  backward dx    `cmp_bf16`, again WITHOUT an `extra` term: unlike ctsi_gn_bwd, whose third pass multiplies a bf16-rounded g (the
                 GN_DX_G_ULPS term of tests/train_audit.py), ctsi_gn_bwd_mod re-derives gu from dy in fp32 and rounds dx once at the
                 store.  The source performs no intermediate bf16 rounding, so there is no term to add; the fp32 column sums over
                 <= 600 voxels x cpg channels (~1e-6 relative to the terms of dx) sit under the 1e-5 rms floor.
  d_s, d_b, d_e, dgamma, dbeta, dxsum   `cmp_f32` with its default bounds (1e-4 rel-L2, 1e-3 of the largest element).

Every scale-shift case asserts that its float64 reference is more than 0.25 rel-L2 away from three wrong forms (additive, s = 0,
halves swapped): a kernel that ignored or mis-ordered the modulation cannot pass.
"""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref_ops as R
from tests import poison as PZ
from tests import resblock_restatement as RR
from tests import vpred_restatement as VR
from tests.helpers import (MID_UNET, TINY_CFG, TINY_UNET, formula_input, formula_noise, formula_sd, load_formula, rel_l2,
                           unet_cfg)
from tests.test_host_resblock_options import keep_mask_np
from tests.train_audit import cmp_bf16, cmp_f32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
E = importlib.import_module("video-to-video-diffusion_amd.engine")
E32 = importlib.import_module("video-to-video-diffusion_amd.engine_f32")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
U = importlib.import_module("video-to-video-diffusion_amd.unet3d")
NET_TOL = 3e-2          # tests/test_gpu_network.py: the bf16 engine against the fp32 oracle
FLOOR = 2e-7            # tests/test_gpu_fp32_mode.py
U24 = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resblock_default_launches.json")

# (n, C, d, h, w): the contiguous form with several samples and a ragged tail; 256 % (C / 8) != 0, the grid-stride non-CONSTQ form;
# more than one 1024-chunk block per sample and more than one backward tile; 256 channels
CASES = [(2, 32, 3, 5, 7), (2, 40, 3, 5, 7), (1, 64, 6, 10, 10), (2, 256, 2, 6, 6)]
IDS = ["n%d_c%d_%dx%dx%d" % c for c in CASES]
GROUPS, EPS = 8, 1e-5
P_DROP, LAYER, SEED = 0.25, 5, 0x9E3779B97F4A7C15
TB_OFF, TB_PAD = 8, 24       # the block's columns start at TB_OFF of a wider time row, as in the stacked projection


def _ptr(t, off_bytes=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + off_bytes)


@pytest.fixture(scope="module")
def G():
    from tests import gpu_utils
    return gpu_utils


def _operands(case, film, f32=False):
    n, c, d, h, w = case
    g = torch.Generator().manual_seed(100 + c + 7 * d + (1 if film else 0))
    x = torch.randn((n, d, h, w, c), generator=g)
    dy = torch.randn((n, d, h, w, c), generator=g)
    gamma = 1.0 + 0.3 * torch.randn(c, generator=g)
    beta = 0.3 * torch.randn(c, generator=g)
    width = 2 * c if film else c
    stride = TB_OFF + width + TB_PAD
    rows = torch.full((2 * n, stride), float("nan"))                       # max_rows = 2n: row blocks 0 and 1
    rows[:, TB_OFF:TB_OFF + width] = 0.5 * torch.randn((2 * n, width), generator=g)
    dt = torch.float32 if f32 else torch.bfloat16
    x, dy = x.to(DEV, dt).contiguous(), dy.to(DEV, dt).contiguous()
    sums = RR.group_sums(x, GROUPS).to(DEV).contiguous()
    return dict(x=x, dy=dy, gamma=gamma.to(DEV), beta=beta.to(DEV), rows=rows.to(DEV), stride=stride, width=width, sums=sums)


def _seed_buf():
    return torch.tensor([SEED - (1 << 64)], dtype=torch.int64, device=DEV)


def _thr(drop):
    return U.dropout_threshold(P_DROP) if drop else 0


def _inv(drop):
    return 65536.0 / (65536.0 - _thr(drop))


def _device_mask(G, case, seed_buf, thr, layer=LAYER):
    n, c, d, h, w = case
    count = n * d * h * w * c
    out = torch.full((count,), 7, dtype=torch.uint8, device=DEV)
    ctx = G.ctx()
    with ctx.scope():
        ctx.lib.dropout_mask(_ptr(seed_buf), layer, thr, count, _ptr(out), ctx.sptr)
    torch.cuda.synchronize()
    return out.view(n, d, h, w, c)


def _fwd(G, case, ops, film, drop, step=None, seed_buf=None):
    n, c, d, h, w = case
    ctx = G.ctx()
    y = torch.full_like(ops["x"], float("nan"))
    step_ptr = None if step is None else torch.tensor([step], dtype=torch.int32, device=DEV)
    with ctx.scope():
        ctx.lib.gn_apply_mod(_ptr(ops["x"]), _ptr(y), _ptr(ops["sums"]), _ptr(ops["gamma"]), _ptr(ops["beta"]), n, c, d, h, w, d,
                             GROUPS, EPS, 1, _ptr(ops["rows"], 4 * TB_OFF), ops["stride"], _ptr(step_ptr), None, 0, int(film),
                             _thr(drop), _inv(drop), _ptr(seed_buf) if drop else None, LAYER, ctx.sptr)
    torch.cuda.synchronize()
    return y


def _row_block(ops, n, step):
    return ops["rows"][step * n:(step + 1) * n, TB_OFF:TB_OFF + ops["width"]]


def _wrong_forms_are_far(ref_args, ref, tag):
    for form in ("additive", "noscale", "swapped"):
        apart = rel_l2(RR.pass_fwd64(*ref_args, form=form), ref)
        print(f"  {tag}: the {form} form is {apart:.3f} rel-L2 from the reference")
        assert apart > 0.25, (form, apart)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("film", [False, True], ids=["additive", "film"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_bf16(G, case, film, drop):
    n = case[0]
    ops = _operands(case, film)
    seed_buf = _seed_buf()
    y = _fwd(G, case, ops, film, drop, seed_buf=seed_buf)
    keep = None
    if drop:
        keep = _device_mask(G, case, seed_buf, _thr(True))
        first = keep.reshape(-1)[:4096].cpu().numpy()
        assert np.array_equal(first, keep_mask_np(SEED, LAYER, _thr(True), first.size))
        frac = float(keep.float().mean())
        assert abs(frac - 0.75) < 5 * (0.75 * 0.25 / keep.numel()) ** 0.5, frac
    args = (ops["x"], ops["sums"], ops["gamma"], ops["beta"], _row_block(ops, n, 0), GROUPS, EPS, film)
    ref = RR.pass_fwd64(*args, keep=keep, inv=_inv(drop))
    res = cmp_bf16(y, ref)
    print(f"forward {case} film={film} drop={drop}: {res['ulps']:.3f} ulp, rel-L2 {res['rel_l2']:.2e}")
    assert torch.isfinite(y.float()).all() and res["ok"], res
    if film:
        _wrong_forms_are_far(args, RR.pass_fwd64(*args), f"{case}")
    if drop:
        assert bool(((y.float() == 0) | (keep == 1)).all())           # a dropped element is an exact zero
    assert torch.equal(_fwd(G, case, ops, film, drop, seed_buf=seed_buf), y)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_bf16_step_ptr_selects_the_row_block(G, case):
    n = case[0]
    ops = _operands(case, True)
    seed_buf = _seed_buf()
    y = _fwd(G, case, ops, True, True, step=1, seed_buf=seed_buf)
    keep = _device_mask(G, case, seed_buf, _thr(True))
    ref = RR.pass_fwd64(ops["x"], ops["sums"], ops["gamma"], ops["beta"], _row_block(ops, n, 1), GROUPS, EPS, True, keep=keep,
                        inv=_inv(True))
    other = RR.pass_fwd64(ops["x"], ops["sums"], ops["gamma"], ops["beta"], _row_block(ops, n, 0), GROUPS, EPS, True, keep=keep,
                          inv=_inv(True))
    res = cmp_bf16(y, ref)
    print(f"forward {case} step_ptr = 1: {res['ulps']:.3f} ulp, rel-L2 {res['rel_l2']:.2e}; row block 0 is {rel_l2(other, ref):.3f} away")
    assert res["ok"], res
    assert rel_l2(other, ref) > 0.25


@pytest.mark.parametrize("case", [(2, 32, 3, 5, 7), (2, 40, 3, 5, 7), (1, 192, 2, 3, 5)], ids=lambda c: "n%d_c%d_%dx%dx%d" % c)
def test_forward_bf16_without_options_is_the_default_pass(G, case):
    """ctsi_gn_apply_mod(film=0, p_thr16=0) is ctsi_gn_apply(silu_pre=1, tbias): the same raw bf16 (contiguous ranges with a ragged
    tail, no constant chunk, grid-stride over three blocks' worth of chunks per row)."""
    n, c, d, h, w = case
    ops = _operands(case, False)
    ctx = G.ctx()
    y = torch.full_like(ops["x"], float("nan"))
    step_ptr = torch.tensor([1], dtype=torch.int32, device=DEV)
    with ctx.scope():
        ctx.lib.gn_apply(_ptr(ops["x"]), _ptr(y), _ptr(ops["sums"]), _ptr(ops["gamma"]), _ptr(ops["beta"]), n, c, d, h, w, d, GROUPS,
                         EPS, 1, _ptr(ops["rows"], 4 * TB_OFF), ops["stride"], _ptr(step_ptr), None, 0, ctx.sptr)
    torch.cuda.synchronize()
    y_mod = _fwd(G, case, ops, False, False, step=1)
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y_mod.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_fp32(G, case):
    n, c, d, h, w = case
    ops = _operands(case, True, f32=True)
    ctx = G.ctx()

    def run(step):
        y = torch.full_like(ops["x"], float("nan"))
        sp = None if step is None else torch.tensor([step], dtype=torch.int32, device=DEV)
        with ctx.scope():
            ctx.lib.gn_apply_mod_f32(_ptr(ops["x"]), _ptr(y), _ptr(ops["sums"]), _ptr(ops["gamma"]), _ptr(ops["beta"]), n, c, d, h,
                                     w, d, GROUPS, EPS, 1, _ptr(ops["rows"], 4 * TB_OFF), ops["stride"], _ptr(sp), None, 0, 1,
                                     ctx.sptr)
        torch.cuda.synchronize()
        return y

    for step in (None, 1):
        y = run(step)
        args = (ops["x"], ops["sums"], ops["gamma"], ops["beta"], _row_block(ops, n, step or 0), GROUPS, EPS, True)
        ref = RR.pass_fwd64(*args)
        res = cmp_f32(y, ref)
        print(f"forward fp32 {case} step {step}: rel-L2 {res['rel_l2']:.2e}, max {res['max_rel']:.2e}")
        assert res["ok"], res
        assert torch.equal(run(step), y)
    _wrong_forms_are_far(args, ref, f"{case}")


def _bwd(G, case, ops, film, drop, seed_buf):
    n, c, d, h, w = case
    ctx = G.ctx()
    ws = torch.full((ctx.lib.gn_bwd_mod_workspace_floats(n, c, d, h, w, GROUPS),), float("nan"), device=DEV)
    out = dict(dx=torch.full_like(ops["x"], float("nan")), dgamma=torch.full((c,), float("nan"), device=DEV),
               dbeta=torch.full((c,), float("nan"), device=DEV), dxsum=torch.full((c,), float("nan"), device=DEV),
               dtb=torch.full((n, ops["stride"]), -77.0, device=DEV))
    with ctx.scope():
        ctx.lib.gn_bwd_mod(_ptr(ops["x"]), _ptr(ops["dy"]), _ptr(ops["sums"]), _ptr(ops["gamma"]), _ptr(ops["beta"]), n, c, d, h, w,
                           GROUPS, EPS, _ptr(ops["rows"], 4 * TB_OFF), ops["stride"], int(film), _thr(drop), _inv(drop),
                           _ptr(seed_buf) if drop else None, LAYER, _ptr(out["dx"]), _ptr(ws), _ptr(out["dgamma"]),
                           _ptr(out["dbeta"]), _ptr(out["dtb"], 4 * TB_OFF), ops["stride"], _ptr(out["dxsum"]), ctx.sptr)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("film", [False, True], ids=["additive", "film"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward(G, case, film, drop):
    n = case[0]
    ops = _operands(case, film)
    seed_buf = _seed_buf()
    got = _bwd(G, case, ops, film, drop, seed_buf)
    keep = _device_mask(G, case, seed_buf, _thr(True)) if drop else None
    ref = RR.pass_bwd64(ops["x"], ops["dy"], ops["sums"], ops["gamma"], ops["beta"], _row_block(ops, n, 0), GROUPS, EPS, film,
                        keep=keep, inv=_inv(drop))
    lo, hi = TB_OFF, TB_OFF + ops["width"]
    rows = [("dx", cmp_bf16(got["dx"], ref["dx"])), ("drow", cmp_f32(got["dtb"][:, lo:hi], ref["drow"])),
            ("dgamma", cmp_f32(got["dgamma"], ref["dgamma"])), ("dbeta", cmp_f32(got["dbeta"], ref["dbeta"])),
            ("dxsum", cmp_f32(got["dxsum"], ref["dxsum"]))]
    for name, res in rows:
        print(f"backward {case} film={film} drop={drop} {name}: ulps {res['ulps']:.3f} rel-L2 {res['rel_l2']:.2e} "
              f"max {res['max_rel']:.2e}")
    for name, res in rows:
        assert res["ok"], (name, res)
    if film:      # both halves carry a gradient, in the order (d_s | d_b)
        c = case[1]
        assert rel_l2(got["dtb"][:, lo:lo + c], ref["drow"][:, c:]) > 0.25
    assert bool((got["dtb"][:, :lo] == -77.0).all()) and bool((got["dtb"][:, hi:] == -77.0).all())    # the block's columns only
    again = _bwd(G, case, ops, film, drop, seed_buf)
    assert all(torch.equal(again[k], got[k]) for k in got)


# ---------------------------------------------------------------------------------------------------------------------
# the network, inference
# ---------------------------------------------------------------------------------------------------------------------
def _film_unet(pkg, kw, seed):
    un = pkg.UNet3D(**kw, use_scale_shift_norm=True)
    sd = load_formula(un, seed)
    return un.to(DEV), sd


def _sd64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


NET = [(TINY_UNET, (2, 8, 4, 8, 8), (8, 10, 11), [500, 37]), (MID_UNET, (1, 4, 6, 12, 8), (9, 12, 13), [999])]


@pytest.mark.parametrize("kw,shape,seeds,t", NET, ids=["tiny", "mid"])
def test_unet_forward_against_the_restatement(pkg, kw, shape, seeds, t):
    un, sd = _film_unet(pkg, kw, seeds[0])
    x, c, t = formula_input(shape, seeds[1]), formula_input(shape, seeds[2]), torch.tensor(t)
    out = un(x.to(DEV), t.to(DEV), c.to(DEV)).cpu()
    ref = RR.unet_forward(sd, unet_cfg(kw), x, t, c)
    additive = RR.unet_forward(sd, unet_cfg(kw), x, t, c, form="additive")
    e, apart = rel_l2(out, ref), rel_l2(additive, ref)
    print(f"U-Net {shape}: rel-L2 to the restatement {e:.3e}; the additive restatement on the same weights is {apart:.3f} away")
    assert torch.isfinite(out).all() and e < NET_TOL, e
    assert apart > 0.25, apart
    prog = [p for k, p in un._ctsi_programs.items() if k[0] == "unet"][0]
    names = [m[0] for m in prog.op_meta]
    blocks = sum(1 for m in un.modules() if type(m).__name__ == "ResBlock3D")
    assert names.count("gn.apply_mod") == blocks
    recs = [a for a in prog.op_audit if a and a.get("kind") == "gn_apply_mod"]
    assert len(recs) == blocks and all(r["film"] and r["drop"] is None for r in recs)
    assert torch.equal(un(x.to(DEV), t.to(DEV), c.to(DEV)).cpu(), out)
    # fp32 mode: within 4 x the fp32 restatement's own distance to float64
    un.inference_precision = "fp32"
    o32 = un(x.to(DEV), t.to(DEV), c.to(DEV)).cpu()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        ref64 = RR.unet_forward(_sd64(sd), unet_cfg(kw), x.double(), t, c.double())
    finally:
        torch.set_default_dtype(old)
    e32, e = rel_l2(ref, ref64), rel_l2(o32, ref64)
    print(f"U-Net {shape} fp32: engine {e:.3g}, fp32 restatement {e32:.3g}")
    assert e <= max(4.0 * e32, FLOOR), (e, e32)
    p32 = [p for k, p in un._ctsi_programs.items() if k[0] == "unet" and "fp32" in k][0]
    assert [m[0] for m in p32.op_meta].count("gn.apply_mod") == blocks


def _t_desc(g, n):
    return [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(n)]


def _noise_fn(i, shape):
    return formula_noise(i, shape)


@pytest.fixture(scope="module")
def film_tiny(pkg):
    return _film_unet(pkg, TINY_UNET, 8)


def test_ddim_captured_equals_eager(pkg):
    un, sd = _film_unet(pkg, TINY_UNET, 8)
    g = pkg.GaussianDiffusion()
    shape, n_steps = (1, 8, 4, 8, 8), 4
    cond = formula_input(shape, 15)
    sp = pkg.DDIMSampler(g, un)
    runs = [sp.sample(shape, cond.to(DEV), n_steps, DEV, eta=0.0, progress=False, noise_fn=_noise_fn) for _ in range(2)]
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])
    progs = [p for k, p in un._ctsi_programs.items() if k[0] == "sampler"]
    assert len(progs) == 1 and progs[0].graph is not None
    assert "gn.apply_mod" in [m[0] for m in progs[0].op_meta[:progs[0].unet_op_count]]
    t_desc = _t_desc(g, n_steps)
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope():       # the same steps eagerly: a separately built program, launch by launch (no graph)
        prog = E.UNetProgram(ctx, un, 1, 4, 8, 8, g.timesteps + 1, "fast")
        prog.add_sampler_step("ddim", False)
        prog.load_latents(_noise_fn(-1, shape).to(DEV), cond.to(DEV))
        prog.set_schedule(t_desc, S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0).to(DEV))
        for _ in t_desc:
            prog.run()
        eager = prog.z_ncdhw()
    torch.cuda.synchronize()
    assert torch.equal(eager, runs[0])
    # and the oracle's loop on the restated U-Net: PSNR within 0.1 dB of the restatement under bf16 autocast (test_gpu_network.py)
    bufs = R.diffusion_buffers("cosine", 1000)

    def restated(autocast):
        def run():
            with RR.resblock_options():
                return R.ddim_sample(lambda z, t, c: R.unet_forward(sd, unet_cfg(TINY_UNET), z, t, c, ""), bufs, shape, cond,
                                     n_steps, eta=0.0, noise_fn=_noise_fn).float()
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                return run()
        return run()

    ref, zb = restated(False), restated(True)
    p_hip, p_bf = R.psnr(runs[0].cpu(), ref, 20.0), R.psnr(zb, ref, 20.0)
    print(f"ddim: final latent PSNR {p_hip:.2f} dB against the restatement, restatement under autocast {p_bf:.2f} dB")
    assert p_hip >= p_bf - 0.1, (p_hip, p_bf)


def test_guided_ddim_per_evaluation(pkg, film_tiny):
    """The criterion of tests/test_gpu_cfg.py::test_per_evaluation_tiny, on the scale-shift model: every guided eps within
    1.25 x (|s| D_c + |1 - s| D_u) of the float64 combination of two fp32 evaluations, every update within 1e-4."""
    from tests.test_gpu_cfg import _per_evaluation
    _per_evaluation(pkg.GaussianDiffusion(), film_tiny[0], (1, 8, 4, 8, 8), 3.0, "bf16", 20)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_v_prediction_ddim_per_evaluation(pkg, film_tiny, precision):
    """The criterion of tests/test_gpu_vpred.py::test_per_evaluation_on_the_engine: the v program's first eps is the conversion of
    the epsilon program's raw output on the same z, within 4 x 2^-24 of the magnitudes involved; the run is finite."""
    un = film_tiny[0]
    ge, gv = pkg.GaussianDiffusion(), pkg.GaussianDiffusion(prediction_type="v_prediction")
    shape = (1, 8, 4, 8, 8)
    cond = formula_input(shape, 20).to(DEV)
    z_t = torch.randn(shape, generator=torch.Generator().manual_seed(21))
    t_desc = _t_desc(ge, 3)
    raw, eps = [], []
    prev = un.inference_precision
    un.inference_precision = precision
    try:
        kw = dict(kind="ddim", t_desc=t_desc, progress=False, z_init=z_t.to(DEV))
        S.run_sampler(ge, un, shape, cond, DEV, eps_trajectory=raw, **kw)
        out = S.run_sampler(gv, un, shape, cond, DEV, eps_trajectory=eps, **kw)
    finally:
        un.inference_precision = prev
    assert torch.isfinite(out).all()
    rows = VR.vp_rows(gv.alphas_cumprod, t_desc[:1])
    ref, mag = VR.convert(raw[0].cpu(), z_t, rows), VR.convert_magnitude(raw[0].cpu(), z_t, rows)
    err = (eps[0].cpu().double() - ref).abs()
    used = float((err / (4 * U24 * mag).clamp_min(1e-300)).max())
    print(f"{precision}: v program eps[0] vs conversion of the epsilon program's raw output: worst |err| / bound {used:.3f}")
    assert (err <= 4 * U24 * mag).all(), used


# ---------------------------------------------------------------------------------------------------------------------
# training: one step of the tiny model in four configurations
# ---------------------------------------------------------------------------------------------------------------------
TRAIN_SHAPE = (2, 8, 6, 8, 8)        # the latent shape of tests/test_gpu_train.py, where the bf16-autocast yardstick is finite on every
                                     # host (at 3 x 3 coarse slices the CPU's bf16 conv weight gradient came out NaN on one)
T_FIX = torch.tensor([37, 812])
CONFIGS = {"default": (False, 0.0), "film": (True, 0.0), "film+drop": (True, 0.2), "additive+drop": (False, 0.2)}


def _train_inputs(shape=TRAIN_SHAPE):
    return formula_input(shape, 31), formula_input(shape, 32), formula_noise(-1, shape)


def _train_model(pkg, film, p):
    un = pkg.UNet3D(**TINY_UNET, use_scale_shift_norm=film, dropout=p)
    sd = {"unet." + k: v for k, v in load_formula(un, 8).items()}
    for k, v in pkg.GaussianDiffusion('cosine', 1000).state_dict().items():
        sd["diffusion." + k] = v
    return un.to(DEV).train(), sd


def _step(pkg, un, seed=None):
    g = pkg.GaussianDiffusion().to(DEV)
    z0, cond, noise = (x.to(DEV) for x in _train_inputs())
    for p in un.parameters():
        p.grad = None
    un.dropout_seed = seed          # None: drawn from the default CPU generator
    loss, _ = g.training_loss(un, z0, cond, t=T_FIX.to(DEV), noise=noise.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), {k: p.grad.float().cpu().clone() for k, p in un.named_parameters()}


def _train_prog(un):
    progs = [p for k, p in un._ctsi_programs.items() if k[0] == "unet-train"]
    assert len(progs) == 1
    return progs[0]


def _exported_masks(G, prog):
    """name -> callable(shape): the keep mask of a layer from ctsi_dropout_mask, the program's seed buffer and layer ids."""
    st = prog.drop_state

    def one(layer_id):
        def make(shape):
            n, c, d, h, w = shape
            m = _device_mask(G, (n, c, d, h, w), st.seed, st.thr, layer=layer_id)
            return m.permute(0, 4, 1, 2, 3).float().cpu()
        return make

    return {name: one(lid) for name, lid, _ in prog.dropout_layers}


def _oracle(sd, masks, inv, autocast=False):
    sd = {k: v.clone() for k, v in sd.items()}
    names = [k for k in sd if k.startswith("unet.")]
    for k in names:
        sd[k].requires_grad_(True)
    z0, cond, noise = _train_inputs()
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            loss = RR.training_loss(sd, unet_cfg(TINY_UNET), z0, cond, T_FIX, noise, masks=masks, inv=inv)
    else:
        loss = RR.training_loss(sd, unet_cfg(TINY_UNET), z0, cond, T_FIX, noise, masks=masks, inv=inv)
    loss.float().backward()
    return float(loss.detach()), {k[len("unet."):]: sd[k].grad.float() for k in names}


@pytest.mark.parametrize("tag", list(CONFIGS))
def test_training_step(G, pkg, tag):
    film, p = CONFIGS[tag]
    un, sd = _train_model(pkg, film, p)
    seed = 0x0123456789ABCDEF
    loss, grads = _step(pkg, un, seed if p > 0 else None)
    prog = _train_prog(un)
    names = [m[0] for m in prog.op_meta]
    blocks = len(prog.dropout_layers)
    assert blocks == sum(1 for m in un.modules() if type(m).__name__ == "ResBlock3D")
    assert [lid for _, lid, _ in prog.dropout_layers] == list(range(blocks))
    mod = film or p > 0
    assert names.count("gn.apply_mod") == (blocks if mod else 0) and names.count("gn.bwd_mod") == (blocks if mod else 0)
    masks, inv = None, 1.0
    if p > 0:
        st = prog.drop_state
        assert st.thr == U.dropout_threshold(p) and int(st.seed.item()) & (2 ** 64 - 1) == seed
        masks, inv = _exported_masks(G, prog), st.inv
    ref_loss, ref_g = _oracle(sd, masks, inv)
    ac_loss, ac_g = _oracle(sd, masks, inv, autocast=True)
    print(f"[{tag}] loss: hip {loss:.6f}  restatement {ref_loss:.6f}  restatement under bf16 autocast {ac_loss:.6f}")
    assert abs(loss - ref_loss) <= 2e-2 * abs(ref_loss)
    worst = []
    gmax = max(float(g.norm()) for g in ref_g.values())
    for name, g in grads.items():
        if float(ref_g[name].norm()) < 1e-5 * gmax:     # q / k thirds of qkv etc.: (numerically) zero in the reference
            assert float(g.norm()) <= 1e-3 * gmax, name
            continue
        if ".qkv." in name:
            c = g.shape[0] // 3
            e_h, e_a = rel_l2(g[2 * c:], ref_g[name][2 * c:]), rel_l2(ac_g[name][2 * c:], ref_g[name][2 * c:])
        else:
            e_h, e_a = rel_l2(g, ref_g[name]), rel_l2(ac_g[name], ref_g[name])
        worst.append((e_h / (2 * e_a + 2e-2), e_h, e_a, name))
    worst.sort(reverse=True)
    for ratio, e_h, e_a, name in worst[:6]:
        print(f"  {name:50s} hip {e_h:.3e}  autocast {e_a:.3e}")
    assert worst[0][0] <= 1.0, worst[0]
    if film:
        for name, g in grads.items():
            if name.endswith("time_mlp.1.weight") and "time_embed" not in name:
                c = g.shape[0] // 2
                assert float(g[:c].abs().max()) > 0 and float(g[c:].abs().max()) > 0, name
    if p > 0:
        loss2, grads2 = _step(pkg, un, seed)
        assert loss2 == loss and all(torch.equal(grads2[k], grads[k]) for k in grads)
        loss3, grads3 = _step(pkg, un, seed + 1)
        assert loss3 != loss and any(not torch.equal(grads3[k], grads[k]) for k in grads)
        # a drawn seed: taken from the default CPU generator, after t and noise, and only with dropout on
        torch.manual_seed(3)
        _step(pkg, un, None)
        drawn = int(prog.drop_state.seed.item())
        torch.manual_seed(3)
        assert drawn == int(torch.randint(-(1 << 63), (1 << 63) - 1, (1,), dtype=torch.int64).item())
        # eval(): the no-dropout loss, bit for bit that of the same weights with dropout = 0
        un.eval()
        e_loss, _ = _step(pkg, un, seed)
        twin, _ = _train_model(pkg, film, 0.0)
        t_loss, _ = _step(pkg, twin, None)
        assert e_loss == t_loss and e_loss != loss
        un.train()
        un.dropout = 0.0            # read at each forward: the same model, no dropout, no seed drawn
        state = torch.random.get_rng_state()
        z_loss, _ = _step(pkg, un, None)
        assert z_loss == t_loss and torch.equal(state, torch.random.get_rng_state())


def test_checkpoint_round_trip_and_optimizer_step(pkg):
    """A scale-shift state dict loads strictly into a scale-shift model and gives the same output; one FusedAdamW step with EMA
    lowers the loss on the fixed batch."""
    un, _ = _train_model(pkg, True, 0.0)
    x, c, t = formula_input((1, 8, 4, 8, 8), 10).to(DEV), formula_input((1, 8, 4, 8, 8), 11).to(DEV), torch.tensor([500], device=DEV)
    un.eval()
    out = un(x, t, c)
    other = pkg.UNet3D(**TINY_UNET, use_scale_shift_norm=True)
    other.load_state_dict({k: v.cpu() for k, v in un.state_dict().items()}, strict=True)
    assert torch.equal(other.to(DEV).eval()(x, t, c), out)
    un.train()
    g = pkg.GaussianDiffusion().to(DEV)
    z0, cond, noise = (v.to(DEV) for v in _train_inputs())
    opt = pkg.FusedAdamW(list(un.parameters()), lr=2e-4, engine_modules=[un])
    losses = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        loss, _ = g.training_loss(un, z0, cond, t=T_FIX.to(DEV), noise=noise.to(DEV))
        losses.append(loss.item())
        if len(losses) == 1:
            loss.backward()
            opt.step()
    print(f"scale-shift loss before / after one FusedAdamW step: {losses[0]:.6f} / {losses[1]:.6f}")
    assert losses[1] < losses[0]


# ---------------------------------------------------------------------------------------------------------------------
# poison-and-guard
# ---------------------------------------------------------------------------------------------------------------------
def test_poison_sampler_and_training_step(pkg):
    model = pkg.VideoToVideoDiffusion(dict(TINY_CFG, unet_use_scale_shift_norm=True, unet_dropout=0.2))
    sd = formula_sd(model, 11)
    for k, v in pkg.GaussianDiffusion('cosine', 1000).state_dict().items():
        sd["diffusion." + k] = v
    model.load_state_dict(sd, strict=True)
    model.eval().to(DEV)
    shape = (1, 8, 5, 6, 10)
    cond = formula_input(shape, 12).to(DEV)
    nf = lambda i, shp: formula_noise(i, shp).to(DEV)

    def sample():
        traj = []
        out = pkg.DDIMSampler(model.diffusion, model.unet).sample(shape, cond, 3, DEV, progress=False, noise_fn=nf,
                                                                  trajectory=traj)
        torch.cuda.synchronize()
        return {"z0": out, "trajectory": traj}

    PZ.run_scenario(sample, name="film-sample[ddim]", modules=[model], ragged=True, inside=PZ.reevaluate(sample))
    tshape = (2, 8, 3, 6, 10)
    z0, tc, noise = (t.to(DEV) for t in (formula_input(tshape, 31), formula_input(tshape, 32), formula_noise(-1, tshape)))
    t = torch.tensor([5, 990], device=DEV)
    model.unet.train()
    model.unet.dropout_seed = 77

    def train():
        for p in model.unet.parameters():
            p.grad = None
        loss, _ = model.diffusion.training_loss(model.unet, z0, tc, t=t, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
        return {"loss": loss.detach(), "grad": {k: p.grad for k, p in model.unet.named_parameters() if p.grad is not None}}

    PZ.run_scenario(train, name="film-drop-train", modules=[model], ragged=True, inside=PZ.reevaluate(train))
    model.invalidate_engine_cache()


# ---------------------------------------------------------------------------------------------------------------------
# the default path: the launches of the parent commit, name for name
# ---------------------------------------------------------------------------------------------------------------------
def default_launch_names(pkg):
    """The launch names of a default tiny U-Net's forward, DDIM-10 and one training step (what the fixture records)."""
    un = pkg.UNet3D(**TINY_UNET)
    load_formula(un, 8)
    un.to(DEV)
    shape = (1, 8, 4, 8, 8)
    x, c = formula_input(shape, 10).to(DEV), formula_input(shape, 11).to(DEV)
    un(x, torch.tensor([500], device=DEV), c)
    g = pkg.GaussianDiffusion()
    pkg.DDIMSampler(g, un).sample(shape, c, 10, DEV, eta=0.0, progress=False, noise_fn=_noise_fn)
    un.train()
    z0, cond, noise = (v.to(DEV) for v in _train_inputs((2, 8, 2, 6, 6)))
    loss, _ = g.to(DEV).training_loss(un, z0, cond, t=T_FIX.to(DEV), noise=noise.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    out = {}
    for key, prog in un._ctsi_programs.items():
        if key[0] in ("unet", "sampler", "unet-train"):
            assert key[0] not in out
            out[key[0]] = [m[0] for m in prog.op_meta]
    return out


def test_default_path_issues_the_parents_launches(pkg):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = default_launch_names(pkg)
    assert set(got) == set(want) == {"unet", "sampler", "unet-train"}
    for k in want:
        assert got[k] == want[k], k
        assert not any("mod" in n for n in got[k])
