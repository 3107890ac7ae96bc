"""GPU: v-prediction (csrc/prediction.hip, prediction.py, GaussianDiffusion(prediction_type=)).

 1. ctsi_pred_to_eps against the float64 restatement (tests/vpred_restatement.py);
 2. ctsi_q_sample_v: ctsi_q_sample's bits, and the v target against float64;
 3. the engine U-Net per evaluation: the v program's eps against the conversion of the epsilon program's raw output;
 4. every sampler on the analytic Gaussian model: v* under 'v_prediction' against eps* under 'epsilon';
 5. 'epsilon' is untouched by a v run on the same model;
 6. guidance on a v model; captured == eager; a batch of two == two single runs;
 7. training: the loss and its gradient on the program's own buffers, parameter gradients against the fp32 oracle, one
    optimizer step;
 8. depth sharding (world 2, lock-step);
 9. poison-and-guard on the v sampler and the v training step;
10. the single-step API with per-sample t.
Every measured figure is printed before it is asserted (profiles/vpred_tests.log is that output)."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import ref_ops as R
from tests import poison as PZ
from tests import vpred_restatement as VR
from tests.helpers import TINY_UNET, bf16_round, formula_input, formula_noise, load_formula, rel_l2, tiny_model_sd, unet_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = importlib.import_module("video-to-video-diffusion_amd.engine")
E32 = importlib.import_module("video-to-video-diffusion_amd.engine_f32")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
P = importlib.import_module("video-to-video-diffusion_amd.parallel")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
U24 = 2.0 ** -24
V = "v_prediction"


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _t_desc(g, n):
    return [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(n)]


def _keys(unet):
    return list(getattr(unet, "_ctsi_programs", {}).keys())


@pytest.fixture(scope="module")
def tiny_unet(pkg):
    un = pkg.UNet3D(**TINY_UNET)
    load_formula(un, 8)
    return un.to(DEV)


class _precision:
    def __init__(self, unet, p):
        self.unet, self.p = unet, p

    def __enter__(self):
        self.prev = self.unet.inference_precision
        self.unet.inference_precision = self.p

    def __exit__(self, *exc):
        self.unet.inference_precision = self.prev


# ---------------------------------------------------------------------------------------------------------------------
# 1. ctsi_pred_to_eps against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_row", [False, True])          # rows_per_step 1 / n
@pytest.mark.parametrize("doubled", [False, True])          # z_rows = n with 2n output rows
@pytest.mark.parametrize("with_hist", [False, True])        # b1 zero / nonzero
@pytest.mark.parametrize("shape", [(2, 8, 4, 8, 8), (1, 3, 5, 7, 9)])      # the second: no 16-byte path
def test_pred_to_eps_against_float64(shape, with_hist, doubled, per_row):
    """|got - ref| <= 4 * 2^-24 * (|a v| + |b0 z| + |b1 h|) elementwise: three products and two sums, each one fp32 rounding
    of a term of that size (the rule of test_gpu_cfg.test_combine_against_float64)."""
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    n, Lc, d, h, w = shape
    rows_out = 2 * n if doubled else n
    rps = rows_out if per_row else 1
    per = Lc * d * h * w
    v = _randn((rows_out, per), 11)
    z = 0.7 * _randn((n, per), 12) + 0.1
    hist = 1.3 * _randn((n, per), 13) if with_hist else None
    live = torch.tensor([[0.31 + 0.07 * r, 0.95 - 0.05 * r, (0.4 - 0.09 * r) if with_hist else 0.0, 0.0]
                         for r in range(rps)], dtype=torch.float32)
    decoy = torch.full((rps, 4), 5.0)                        # step 0 of the table: different values, never used
    table = torch.cat([decoy, live]).to(DEV).contiguous()
    step = torch.ones(1, dtype=torch.int32, device=DEV)      # points at row block 1
    out, zd = v.to(DEV).contiguous(), z.to(DEV).contiguous()
    hd = None if hist is None else hist.to(DEV).contiguous()
    with ctx.scope():
        lib.pred_to_eps(_ptr(out), _ptr(zd), _ptr(hd), _ptr(table), _ptr(step), rps, rows_out, n, per, ctx.sptr)
    torch.cuda.synchronize()
    rows = live.double()[[b % rps for b in range(rows_out)]]
    zz = z[[b % n for b in range(rows_out)]]
    hh = None if hist is None else hist[[b % n for b in range(rows_out)]]
    ref, mag = VR.convert(v, zz, rows, hh), VR.convert_magnitude(v, zz, rows, hh)
    got = out.cpu().double()
    used = float(((got - ref).abs() / (4 * U24 * mag).clamp_min(1e-300)).max())
    print(f"pred_to_eps {shape} hist={with_hist} rows={rows_out} rows_per_step={rps}: worst |err| / bound = {used:.3f}")
    assert torch.equal(zd.cpu(), z) and (hist is None or torch.equal(hd.cpu(), hist))       # read only
    assert ((got - ref).abs() <= 4 * U24 * mag).all(), used


@pytest.mark.parametrize("shape", [(2, 8, 4, 8, 8), (1, 3, 5, 7, 9)])
def test_pred_to_eps_identity_row_keeps_the_bits(shape):
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    n, per = shape[0], int(np.prod(shape[1:]))
    v = _randn((n, per), 21)
    v[0, :4] = torch.tensor([0.0, -0.0, 1.5e-38, -3e38])     # zeros of both signs, the smallest and the largest normals
    out, z, hist = v.to(DEV), _randn((n, per), 22).to(DEV), _randn((n, per), 23).to(DEV)
    row = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV)
    with ctx.scope():
        lib.pred_to_eps(_ptr(out), _ptr(z), _ptr(hist), _ptr(row), None, 1, n, n, per, ctx.sptr)     # NULL step_ptr: row 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), v.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# 2. ctsi_q_sample_v
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,t", [((2, 8, 2, 6, 6), [0, 999]), ((1, 3, 3, 5, 7), [500]), ((2, 8, 2, 6, 6), [1, 37])])
def test_q_sample_v(pkg, shape, t):
    """The z_t slice: the bits of ctsi_q_sample.  The target: |got - ref| <= 3 * 2^-24 * (|sqrt(abar) noise| + |sqrt(1 -
    abar) z0|) against float64 on the same fp32 coefficient tables (one product, one fma)."""
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    g = pkg.GaussianDiffusion()
    n, Lc, d, h, w = shape
    z0, noise = formula_input(shape, 1), _randn(shape, 2)
    td = torch.tensor(t, dtype=torch.int32, device=DEV)
    sa, s1 = g.sqrt_alphas_cumprod.to(DEV), g.sqrt_one_minus_alphas_cumprod.to(DEV)
    z0d, nd = z0.to(DEV), noise.to(DEV)
    c_total, c_off = 2 * Lc + 1, 1
    xa = torch.full((n * d * h * w * c_total,), 3.0, dtype=torch.bfloat16, device=DEV)
    xb = xa.clone()
    vt = torch.full(shape, float("nan"), device=DEV)
    with ctx.scope():
        lib.q_sample(_ptr(z0d), _ptr(nd), _ptr(sa), _ptr(s1), _ptr(td), _ptr(xa), n, Lc, d, h, w, c_total, c_off, ctx.sptr)
        lib.q_sample_v(_ptr(z0d), _ptr(nd), _ptr(sa), _ptr(s1), _ptr(td), _ptr(xb), _ptr(vt), n, Lc, d, h, w, c_total, c_off,
                       ctx.sptr)
    torch.cuda.synchronize()
    assert torch.equal(xa.view(torch.int16).cpu(), xb.view(torch.int16).cpu())      # z_t and the channels beside it
    tt = torch.tensor(t)
    a, s = g.sqrt_alphas_cumprod[tt], g.sqrt_one_minus_alphas_cumprod[tt]
    ref = VR.v_target(a, s, z0, noise)
    mag = (VR._b(a, z0) * noise.double()).abs() + (VR._b(s, z0) * z0.double()).abs()
    err = (vt.cpu().double() - ref).abs()
    used = float((err / (3 * U24 * mag).clamp_min(1e-300)).max())
    print(f"q_sample_v {shape} t={t}: z_t bit-identical; v target worst |err| / bound = {used:.3f}")
    assert (err <= 3 * U24 * mag).all(), used
    assert torch.equal(z0d.cpu(), z0) and torch.equal(nd.cpu(), noise)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the engine U-Net, per evaluation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_per_evaluation_on_the_engine(pkg, tiny_unet, precision):
    """The network launches of the two programs are the same, so on the same z the v program's first eps is the conversion
    of the epsilon program's raw output: within the bound of test 1.  The launch is also audited from its own record."""
    ge, gv = pkg.GaussianDiffusion(), pkg.GaussianDiffusion(prediction_type=V)
    shape = (1, 8, 4, 8, 8)
    cond, z_t = formula_input(shape, 20).to(DEV), _randn(shape, 21)
    t_desc = _t_desc(ge, 3)
    raw, eps = [], []
    with _precision(tiny_unet, precision):
        kw = dict(kind="ddim", t_desc=t_desc, progress=False, z_init=z_t.to(DEV))
        S.run_sampler(ge, tiny_unet, shape, cond, DEV, eps_trajectory=raw, **kw)
        S.run_sampler(gv, tiny_unet, shape, cond, DEV, eps_trajectory=eps, **kw)
        progs = {k: p for k, p in tiny_unet._ctsi_programs.items() if k[0] == "sampler" and precision in k}
    pe = [p for k, p in progs.items() if V not in k and ("ddim", False) == k[7:9]]
    pv = [p for k, p in progs.items() if V in k]
    assert len(pv) == 1 and len(pe) >= 1
    pe, pv = pe[0], pv[0]
    assert pv.unet_op_count == pe.unet_op_count and len(pv.ops) == len(pe.ops) + 1
    assert [m[0] for m in pv.op_meta[:pv.unet_op_count]] == [m[0] for m in pe.op_meta[:pe.unet_op_count]]
    assert pv.op_meta[pv.unet_op_count][0] == "pred.to_eps"
    rows = VR.vp_rows(gv.alphas_cumprod, t_desc[:1])
    ref, mag = VR.convert(raw[0].cpu(), z_t, rows), VR.convert_magnitude(raw[0].cpu(), z_t, rows)
    err = (eps[0].cpu().double() - ref).abs()
    used = float((err / (4 * U24 * mag).clamp_min(1e-300)).max())
    print(f"{precision}: v program eps[0] vs conversion of the epsilon program's raw output: worst |err| / bound {used:.3f}")
    assert (err <= 4 * U24 * mag).all(), used
    # the audit record: run the program eagerly up to the launch, then the launch, and re-derive it from its operands
    ctx = E.Ctx.get(torch.device(DEV))
    k = pv.unet_op_count
    rec = pv.op_audit[k]
    assert rec["kind"] == "pred_to_eps" and rec["n"] == 1 and rec["z_rows"] == 1 and rec["rows_per_step"] == 1
    with ctx.scope():
        pv.load_latents(z_t.to(DEV), cond)
        pv.set_schedule(t_desc, S.ddim_coef_rows(gv.alphas_cumprod, t_desc, 0.0).to(DEV), S._step_plan(
            gv, "ddim", t_desc, 0.0, 2, None).pred)
        for op in pv.ops[:k]:
            op()
        before, zbuf = rec["out"].clone(), rec["z"].clone()
        pv.ops[k]()
        after = rec["out"].clone()
    torch.cuda.synchronize()
    row = rec["rows"][int(rec["step_ptr"].item())].cpu().double()
    ref, mag = VR.convert(before.cpu(), zbuf.cpu(), row), VR.convert_magnitude(before.cpu(), zbuf.cpu(), row)
    err = (after.cpu().double() - ref).abs()
    print(f"{precision}: audit of the pred_to_eps launch: worst |err| / bound "
          f"{float((err / (4 * U24 * mag).clamp_min(1e-300)).max()):.3f}")
    assert (err <= 4 * U24 * mag).all()
    assert torch.equal(row[:3].float(), VR.vp_rows(gv.alphas_cumprod, t_desc[:1])[0].float())


# ---------------------------------------------------------------------------------------------------------------------
# 4. analytic-model equivalence on every sampler
# ---------------------------------------------------------------------------------------------------------------------
def _restated(g, kind, noises, cond, n_steps, heun=None):
    """Float64 sampling of the analytic model driven by eps* (the engine's fp32 coefficient rows widened)."""
    mean_c = cond.double()
    z = noises[-1].double().clone()
    if kind == "heun":
        r = heun
        rows = r.rows.double()
        z = r.init[0] * z
        if r.gammas[0] > 0:
            z = z + r.init[1] * noises[0].double()
        d1, zin = torch.zeros_like(z), z.clone()
        for e in range(rows.shape[0]):
            s = float(r.sigma_eval[e])
            al = 1.0 / math.sqrt(1 + s * s)
            eps = VR.analytic(al, s * al, zin, mean_c)[0]
            c = rows[e]
            dd = (c[0] * z + c[1] * d1 - c[2] * eps).clamp(-10, 10)
            if c[3] == 0:
                d1, zin = dd, c[4] * z + c[5] * dd
            else:
                z = c[4] * z + c[5] * dd + c[6] * d1
                if r.noise_step[e] >= 0:
                    z = z + c[7] * noises[r.noise_step[e]].double()
                zin = z
        return z
    ac = g.alphas_cumprod.double()
    t_desc = list(reversed(range(g.timesteps)))[:n_steps] if kind == "ddpm" else _t_desc(g, n_steps)
    if kind == "dpmpp":
        rows, xp = S.dpm_coef_rows(g.alphas_cumprod, t_desc, 2).double(), torch.zeros_like(z)
    elif kind == "ddim":
        rows = S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0).double()
    else:
        rows = g.ddpm_coef_rows(t_desc).double().cpu()
    for i, t in enumerate(t_desc):
        e = VR.analytic(ac[t].sqrt(), (1 - ac[t]).sqrt(), z, mean_c)[0]
        if kind == "dpmpp":
            x0 = (rows[i, 0] * z - rows[i, 1] * e).clamp(-10, 10)
            z = rows[i, 2] * z + rows[i, 3] * x0 + rows[i, 4] * xp
            xp = x0
        elif kind == "ddim":
            x0 = ((z - rows[i, 0] * e) / rows[i, 1]).clamp(-10, 10)
            z = rows[i, 2] * x0 + rows[i, 3] * e
        else:
            x0 = ((z - rows[i, 0] * e) / rows[i, 1]).clamp(-1, 1)
            z = rows[i, 2] * x0 + rows[i, 3] * z + rows[i, 4] * noises[i].double()
    return z


def _analytic_run(pkg, g, kind, shape, cond, noises, n_steps, **kw):
    """One run of sampler `kind` through the generic-callable loop; the callable follows g.prediction_type."""
    nf = lambda i, shp: noises[i].to(DEV)
    if kind == "heun_churn" or kind == "heun":
        i_eps, i_v = VR.analytic_callables_edm(np.log(S.sigma_table(g.alphas_cumprod)), DEV)
    else:
        i_eps, i_v = VR.analytic_callables(g.alphas_cumprod, DEV)
    model = i_v if g.prediction_type == V else i_eps
    common = dict(progress=False, noise_fn=nf, **kw)
    if kind == "ddim":
        return pkg.DDIMSampler(g, model).sample(shape, cond.to(DEV), n_steps, DEV, **common), None
    if kind == "dpmpp":
        return pkg.DPMSolverSampler(g, model).sample(shape, cond.to(DEV), n_steps, DEV, **common), None
    if kind == "ddpm":
        return pkg.DDPMSampler(g, model).sample(shape, cond.to(DEV), DEV, num_steps=n_steps, **common), None
    sp = pkg.HeunSampler(g, model, order=2, s_churn=40.0 if kind == "heun_churn" else 0.0)
    return sp.sample(shape, cond.to(DEV), n_steps, DEV, **common), sp.coef_rows(n_steps)


@pytest.mark.parametrize("kind", ["ddim", "ddpm", "dpmpp", "heun", "heun_churn"])
def test_analytic_model_v_equals_epsilon(pkg, kind):
    """v* under 'v_prediction' and eps* under 'epsilon' sample the same process.  Yardstick: the epsilon run's own maximum
    error against the float64 restatement; the v run may show 4 times that (the conversion adds one rounding per
    evaluation, amplified like the existing ones), with an absolute floor of 2^-20 max|z|."""
    ge, gv = pkg.GaussianDiffusion(), pkg.GaussianDiffusion(prediction_type=V)
    shape, N = (1, 8, 2, 4, 4), 4
    cond = formula_input(shape, 2)
    noises = {i: _randn(shape, 500 + i) for i in range(-1, N + 1)}
    out_e, rows = _analytic_run(pkg, ge, kind, shape, cond, noises, N)
    out_v, _ = _analytic_run(pkg, gv, kind, shape, cond, noises, N)
    ref = _restated(ge, "heun" if rows is not None else kind, noises, cond, N, heun=rows)
    if kind == "heun_churn":
        assert rows.gammas[0] > 0 and sum(1 for s in rows.noise_step if s >= 0) > 0        # the churn really is on
    e_eps = float((out_e.cpu().double() - ref).abs().max())
    e_v = float((out_v.cpu().double() - ref).abs().max())
    floor = 2.0 ** -20 * float(ref.abs().max())
    print(f"analytic {kind}: max |err| vs float64: epsilon {e_eps:.3e}, v {e_v:.3e} (ratio {e_v / max(e_eps, 1e-300):.2f}; "
          f"floor {floor:.3e}, max|z| {float(ref.abs().max()):.3f})")
    assert torch.isfinite(out_v).all()
    assert e_v <= max(4 * e_eps, floor), (e_v, e_eps)


# ---------------------------------------------------------------------------------------------------------------------
# 5. 'epsilon' is untouched
# ---------------------------------------------------------------------------------------------------------------------
def test_epsilon_generate_is_bit_identical_around_a_v_run(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    v_in = formula_input((1, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    nf = lambda i, shp: _randn(shp, 900 + i).to(DEV)
    assert model.diffusion.prediction_type == "epsilon"
    before = model.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf)
    keys = _keys(model.unet)
    assert keys and not any(V in k for k in keys)
    model.diffusion.prediction_type = V          # a plain attribute: the same weights read as a v model
    try:
        as_v = model.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf)
    finally:
        model.diffusion.prediction_type = "epsilon"
    v_keys = [k for k in _keys(model.unet) if V in k]
    assert len(v_keys) == 1 and [k for k in _keys(model.unet) if V not in k] == keys
    after = model.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf)
    assert torch.isfinite(as_v).all() and not torch.equal(as_v, before)
    assert torch.equal(before, after)
    assert [k for k in _keys(model.unet) if V not in k] == keys
    # the config key builds the same thing
    cfg_v = dict(model.config, prediction_type=V)
    mv = pkg.VideoToVideoDiffusion(cfg_v).eval()
    mv.load_state_dict(model.state_dict(), strict=True)
    mv.to(DEV)
    assert torch.equal(mv.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf), as_v)


# ---------------------------------------------------------------------------------------------------------------------
# 6. guidance on a v model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_guided_v_sampling_of_the_analytic_model(pkg, phi):
    """v* is affine in c and the conversion adds the same b0 z to both branches, so the guided eps is eps* on s c: guided v
    sampling == unguided sampling on s c (test_gpu_cfg item 5, its 2e-3).  With the rescale the guided eps is m eps*(s c),
    no longer an unguided run of anything; the conversion comes first, so the run must equal the guided run of the eps*
    callable under 'epsilon' with the same (s, phi) -- held to the same figure."""
    ge, gv = pkg.GaussianDiffusion(), pkg.GaussianDiffusion(prediction_type=V)
    shape, N, s = (2, 8, 2, 4, 4), 4, 2.5
    cond = formula_input(shape, 2)
    noises = {-1: _randn(shape, 1)}
    kw = dict(guidance_scale=s, guidance_rescale=phi)
    for kind in ("ddim", "dpmpp", "heun"):
        out_v, rows = _analytic_run(pkg, gv, kind, shape, cond, noises, N, **kw)
        if phi == 0.0:
            ref = _restated(ge, kind, noises, s * cond, N, heun=rows)      # eps*(s c) = eps_u + s (eps_c - eps_u)
        else:
            ref = _analytic_run(pkg, ge, kind, shape, cond, noises, N, **kw)[0].cpu()
        err = rel_l2(out_v.cpu(), ref)
        print(f"guided v {kind} s={s} phi={phi}: rel-L2 {err:.3e}")
        assert torch.isfinite(out_v).all() and err < 2e-3, (kind, err)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_guided_v_captured_equals_eager(pkg, tiny_unet, precision):
    gv = pkg.GaussianDiffusion(prediction_type=V)
    shape, n_steps, s, phi = (1, 8, 4, 8, 8), 4, 3.0, 0.7
    cond, z_t = formula_input(shape, 41).to(DEV), _randn(shape, 43).to(DEV)
    t_desc = _t_desc(gv, n_steps)
    plan = S._step_plan(gv, "ddim", t_desc, 0.0, 2, None)
    with _precision(tiny_unet, precision):
        sp = pkg.DDIMSampler(gv, tiny_unet)
        runs = [sp.sample(shape, cond, n_steps, DEV, progress=False, z_init=z_t, guidance_scale=s, guidance_rescale=phi)
                for _ in range(2)]
        ctx = E.Ctx.get(torch.device(DEV))
        with ctx.scope():       # the same step eagerly: a separately built program, launch by launch (no graph)
            cls = E32.UNetProgramF32 if precision == "fp32" else E.UNetProgram
            prog = cls(ctx, tiny_unet, 1, 4, 8, 8, (gv.timesteps + 1) * 2, tiny_unet.attention_mode, guided=True,
                       rescale=True, prediction=V)
            prog.add_sampler_step("ddim", False)
            names = [m[0] for m in prog.op_meta[prog.unet_op_count:]]
            prog.load_latents(z_t, cond)
            prog.set_schedule([t for t in t_desc for _ in range(2)], plan.coef.to(DEV), plan.pred)
            prog.set_guidance(s, phi)
            for _ in t_desc:
                prog.run()
            eager = prog.z_ncdhw()
        torch.cuda.synchronize()
    assert names[0] == "pred.to_eps" and names[1] == "cfg.stats" and names.count("pred.to_eps") == 1     # ahead of the guidance
    assert prog.op_audit[prog.unet_op_count]["n"] == 2 and prog.op_audit[prog.unet_op_count]["z_rows"] == 1
    assert torch.isfinite(runs[0]).all()
    assert torch.equal(runs[0], runs[1]) and torch.equal(eager, runs[0])


def test_guided_v_batch_of_two_equals_two_single_runs(pkg, tiny_unet):
    gv = pkg.GaussianDiffusion(prediction_type=V)
    shape = (2, 8, 4, 8, 8)
    cond, z_t = formula_input(shape, 50).to(DEV), _randn(shape, 51).to(DEV)
    kw = dict(progress=False, guidance_scale=3.0, guidance_rescale=0.7)
    with _precision(tiny_unet, "fp32"):
        sp = pkg.DDIMSampler(gv, tiny_unet)
        both = sp.sample(shape, cond, 4, DEV, z_init=z_t, **kw)
        one = [sp.sample((1,) + shape[1:], cond[b:b + 1], 4, DEV, z_init=z_t[b:b + 1], **kw) for b in (0, 1)]
    for b in (0, 1):
        err = rel_l2(both[b:b + 1].cpu(), one[b].cpu())
        print(f"fp32 guided v: sample {b} of a batch of two vs alone rel-L2 {err:.3e}")
        assert err < 1e-5          # the figure of test_gpu_cfg.test_batch_of_two_equals_two_single_guided_runs


# ---------------------------------------------------------------------------------------------------------------------
# 7. training
# ---------------------------------------------------------------------------------------------------------------------
T_FIX = torch.tensor([37, 812])
TRAIN_SHAPE = (2, 8, 2, 6, 6)
MASK = torch.tensor([[[1., 1.]], [[1., 0.]]])          # (B, 1, T): per-sample valid counts differ


def _train_inputs():
    return formula_input(TRAIN_SHAPE, 31), formula_input(TRAIN_SHAPE, 32), formula_noise(-1, TRAIN_SHAPE)


def _norm_restated(g, mask, v_form):
    B, Lc, d, h, w = TRAIN_SHAPE
    ab = g.alphas_cumprod.double()[T_FIX]
    snr = ab / (1 - ab + 1e-8)
    wgt = VR.min_snr_weight_v(g.alphas_cumprod, T_FIX) if v_form else torch.clamp(snr, max=5.0) / (snr + 1e-8)
    if mask is None:
        return wgt / float(B * Lc * d * h * w)
    nv = mask.double().expand(B, Lc, d).reshape(B, -1).sum(1) * (h * w)
    assert not bool((nv == nv[0]).all())
    return wgt / (nv * B)


@pytest.mark.parametrize("tag", ["nomask", "mask"])
def test_v_training_loss_and_its_gradient(pkg, tiny_unet, tag):
    """The loss against float64 on the program's own prediction buffer (1e-5 relative, the figure of
    test_gpu_train_ops.test_q_sample_and_loss), d_pred against 2 norm mask (pred - v_target) rounded to bf16."""
    gv, gc = pkg.GaussianDiffusion(prediction_type=V).to(DEV), pkg.GaussianDiffusion()      # gc: the buffers on the host
    z0, cond, noise = _train_inputs()
    mask = None if tag == "nomask" else MASK
    for p in tiny_unet.parameters():
        p.grad = None
    loss, ld = gv.training_loss(tiny_unet, z0.to(DEV), cond.to(DEV), mask=None if mask is None else mask.to(DEV),
                                t=T_FIX.to(DEV), noise=noise.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert set(ld) == {"mse", "total"}
    B, Lc, d, h, w = TRAIN_SHAPE
    progs = [p for k, p in tiny_unet._ctsi_programs.items() if k[0] == "unet-train" and k[2:6] == (B, d, h, w)]
    prog = [p for k, p in tiny_unet._ctsi_programs.items() if k[0] == "unet-train" and k[2:6] == (B, d, h, w) and V in k]
    assert len(prog) == 1 and len(progs) >= 1
    prog = prog[0]
    kinds = [a for a in prog.op_audit if a and a.get("kind") == "train.inputs"]
    assert kinds and kinds[0]["kernel"] == "q_sample_v" and kinds[0]["v_target"] is prog.v_target
    assert [a for a in prog.op_audit if a and a.get("kind") == "loss.fwd"][0]["noise"] is prog.v_target
    assert [a for a in prog.op_audit if a and a.get("kind") == "loss_bwd"][0]["noise"] is prog.v_target
    pred = prog.eps.cpu().permute(0, 4, 1, 2, 3).contiguous()                       # fp32 NCDHW
    a, s = gc.sqrt_alphas_cumprod[T_FIX], gc.sqrt_one_minus_alphas_cumprod[T_FIX]
    vt = VR.v_target(a, s, z0, noise)
    vt_err = (prog.v_target.cpu().double() - vt).abs()
    vt_mag = (VR._b(a, z0) * noise.double()).abs() + (VR._b(s, z0) * z0.double()).abs()
    assert (vt_err <= 3 * U24 * vt_mag).all()
    norm = _norm_restated(gc, mask, True)
    me = torch.ones(TRAIN_SHAPE, dtype=torch.float64) if mask is None else \
        mask.double().expand(B, Lc, d)[:, :, :, None, None].expand(TRAIN_SHAPE)
    ref = float((norm * (me * (pred.double() - vt) ** 2).reshape(B, -1).sum(1)).sum())
    rel = abs(loss.item() - ref) / abs(ref)
    n_err = float(((prog.norm.cpu().double() - norm).abs() / norm).max())
    print(f"v training [{tag}]: loss {loss.item():.6f} float64 {ref:.6f} rel {rel:.2e}; norm rel {n_err:.2e}")
    assert n_err <= 2 * U24 and rel <= 1e-5
    # d_pred: the kernel's fp32 expression on the program's own fp32 operands, rounded to bf16
    df = pred - prog.v_target.cpu()
    want = bf16_round(2.0 * prog.norm.cpu().view(-1, 1, 1, 1, 1) * me.float() * df * 1.0)
    got = prog.d_eps.t.float().reshape(B, d, h, w, prog.Lp)[..., :Lc].permute(0, 4, 1, 2, 3).cpu()
    bad = int((got != want).sum())
    print(f"v training [{tag}]: d_pred elements that differ from the bf16-rounded restatement: {bad} of {got.numel()}")
    assert bad == 0
    for p in tiny_unet.parameters():
        p.grad = None


def _oracle_grads(sd, cfg, g, v_form):
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    z0, cond, noise = _train_inputs()
    a = g.sqrt_alphas_cumprod[T_FIX].float().view(-1, 1, 1, 1, 1)
    s = g.sqrt_one_minus_alphas_cumprod[T_FIX].float().view(-1, 1, 1, 1, 1)
    pred = R.unet_forward(sd, cfg, a * z0 + s * noise, T_FIX, cond, "")
    target = a * noise - s * z0 if v_form else noise
    ac = g.alphas_cumprod[T_FIX]
    snr = ac / (1 - ac + 1e-8)
    wgt = torch.clamp(snr, max=5.0) / ((snr + 1.0) if v_form else (snr + 1e-8))
    loss = (((pred - target) ** 2).reshape(pred.shape[0], -1).mean(1) * wgt).mean()
    loss.backward()
    return loss.item(), {k: v.grad for k, v in sd.items()}


def test_v_training_gradients_against_the_oracle_and_one_optimizer_step(pkg):
    """Parameter gradients of loss.backward() against the fp32 oracle's autograd (oracle/ref_ops.py's U-Net, the v target
    written here).  Yardstick: the epsilon run's rel-L2 against the same oracle, measured here; the v run within 2 x."""
    un = pkg.UNet3D(**TINY_UNET)
    sd = load_formula(un, 8)
    un.to(DEV).train()
    cfg = unet_cfg(TINY_UNET)
    z0, cond, noise = (x.to(DEV) for x in _train_inputs())
    figures = {}
    for v_form in (False, True):
        g = pkg.GaussianDiffusion(prediction_type=V if v_form else "epsilon")
        ref_loss, ref_g = _oracle_grads(sd, cfg, g, v_form)
        g.to(DEV)
        for p in un.parameters():
            p.grad = None
        loss, _ = g.training_loss(un, z0, cond, t=T_FIX.to(DEV), noise=noise.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        got = torch.cat([p.grad.float().cpu().reshape(-1) for _, p in un.named_parameters()])
        ref = torch.cat([ref_g[k].reshape(-1) for k, _ in un.named_parameters()])
        figures[v_form] = (rel_l2(got, ref), abs(loss.item() - ref_loss) / abs(ref_loss))
        print(f"{'v' if v_form else 'epsilon'} training vs fp32 oracle: gradient rel-L2 {figures[v_form][0]:.3e}, "
              f"loss rel {figures[v_form][1]:.3e}")
    assert figures[True][0] <= 2 * figures[False][0], figures
    assert figures[True][1] <= 2e-2                      # the loss figure of tests/test_gpu_train.py
    # one FusedAdamW step lowers the v loss on the fixed batch
    gv = pkg.GaussianDiffusion(prediction_type=V).to(DEV)
    opt = pkg.FusedAdamW(list(un.parameters()), lr=2e-4, engine_modules=[un])
    losses = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        loss, _ = gv.training_loss(un, z0, cond, t=T_FIX.to(DEV), noise=noise.to(DEV))
        losses.append(loss.item())
        if len(losses) == 1:
            loss.backward()
            opt.step()
    print(f"v loss before / after one FusedAdamW step: {losses[0]:.6f} / {losses[1]:.6f}")
    assert losses[1] < losses[0]


# ---------------------------------------------------------------------------------------------------------------------
# 8. depth sharding
# ---------------------------------------------------------------------------------------------------------------------
def test_sharded_v_sampling_world2(pkg, tiny_unet):
    """World 2 in lock-step on one GPU, as tests/test_gpu_sharded.py drives its ranks: DDIM-3 at latent depth 4, the v
    program sharded against unsharded, within that file's figures for epsilon (eps 3e-2, z 0.15)."""
    gv = pkg.GaussianDiffusion(prediction_type=V)
    shape = (1, 8, 4, 8, 8)
    n, Lc, d, h, w = shape
    x, c = formula_input(shape, 10), formula_input(shape, 11)
    t_desc = _t_desc(gv, 3)
    plan = S._step_plan(gv, "ddim", t_desc, 0.0, 2, None)
    ctx = E.Ctx.get(torch.device(DEV))
    world = 2
    with ctx.scope():
        ref = E.UNetProgram(ctx, tiny_unet, n, d, h, w, 8, prediction=V)
        ref.add_sampler_step("ddim", False)
        ref.load_latents(x, c)
        ref.set_schedule(t_desc, plan.coef.to(DEV), plan.pred)
        ref.run()
        eps_ref = ref.eps_ncdhw().cpu()
        for _ in t_desc[1:]:
            ref.run()
        z_ref = ref.z_ncdhw().cpu()
        comm = P.LocalComm(world)
        progs = []
        for r in range(world):
            spec = P.ShardSpec(r, world, comm, d)
            pr = E.UNetProgram(ctx, tiny_unet, n, spec.depth_local, h, w, 8, shard=spec, prediction=V)
            pr.add_sampler_step("ddim", False)
            pr.load_latents(x, c)
            pr.set_schedule(t_desc, plan.coef.to(DEV), plan.pred)
            progs.append(pr)
        assert sum(1 for m in progs[0].op_meta if m[0] == "pred.to_eps") == 1
        P.run_lockstep(progs)
        eps = torch.cat([p.eps_ncdhw() for p in progs], dim=2).cpu()
        P.run_lockstep(progs, launches=len(t_desc) - 1)
        z = torch.cat([p.z_ncdhw() for p in progs], dim=2).cpu()
    torch.cuda.synchronize()
    e_eps, e_z = rel_l2(eps, eps_ref), rel_l2(z, z_ref)
    print(f"sharded v world 2: eps rel-L2 {e_eps:.3e}, z after {len(t_desc)} evaluations rel-L2 {e_z:.3e}")
    assert torch.isfinite(z).all() and e_eps < 3e-2 and e_z < 0.15
    # and through the public loop: one virtual rank (the multi-rank arithmetic is the lock-step run above)

    class OneRank(P.LocalComm):
        rank = 0

    nf = lambda i, s_: x
    out = S.run_sampler_sharded(gv, tiny_unet, shape, c.to(DEV), ctx, x.to(DEV), kind="ddim", t_desc=t_desc, eta=0.0,
                                noise_fn=nf, comm=OneRank(1))
    e_pub = rel_l2(out.cpu(), z_ref)
    print(f"sharded v, run_sampler_sharded on one rank vs unsharded: rel-L2 {e_pub:.3e}")
    assert e_pub < 0.15


# ---------------------------------------------------------------------------------------------------------------------
# 9. poison-and-guard
# ---------------------------------------------------------------------------------------------------------------------
def test_poison_v_sampler_and_v_training_step(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    model.diffusion.prediction_type = V
    shape = (1, 8, 5, 6, 10)
    cond = formula_input(shape, 12).to(DEV)
    nf = lambda i, shp: formula_noise(i, shp).to(DEV)

    def sample():
        traj = []
        out = pkg.HeunSampler(model.diffusion, model.unet).sample(shape, cond, 3, DEV, progress=False, noise_fn=nf,
                                                                  trajectory=traj, guidance_scale=2.5)
        torch.cuda.synchronize()
        return {"z0": out, "trajectory": traj}

    PZ.run_scenario(sample, name="v-sample[heun,cfg]", modules=[model], ragged=True, inside=PZ.reevaluate(sample))
    tshape = (2, 8, 3, 6, 10)
    z0, tc, noise = (t.to(DEV) for t in (formula_input(tshape, 31), formula_input(tshape, 32), formula_noise(-1, tshape)))
    t = torch.tensor([5, 990], device=DEV)

    def train():
        for p in model.unet.parameters():
            p.grad = None
        loss, _ = model.diffusion.training_loss(model.unet, z0, tc, t=t, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
        return {"loss": loss.detach(), "grad": {k: p.grad for k, p in model.unet.named_parameters() if p.grad is not None}}

    PZ.run_scenario(train, name="v-train", modules=[model], ragged=True, inside=PZ.reevaluate(train))
    model.invalidate_engine_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 10. the single-step API
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False])
def test_single_step_api_with_a_v_callable(pkg, clip):
    """p_mean_variance / p_sample with per-sample t on a v callable against float64: eps from the conversion, then the
    posterior mean of the reference formulas (the buffers the engine reads).  1e-5 of max|mean|: a handful of fp32
    roundings of O(1) terms, the x0 division by sqrt(abar) excepted -- t stays where sqrt(abar) >= 0.1."""
    gv, gc = pkg.GaussianDiffusion(prediction_type=V).to(DEV), pkg.GaussianDiffusion()      # gc: the buffers on the host
    shape = (2, 8, 2, 4, 4)
    z_t, cond, noise = _randn(shape, 3), formula_input(shape, 4), _randn(shape, 5)
    t = torch.tensor([0, 600])
    _, v_model = VR.analytic_callables(gc.alphas_cumprod, DEV)
    mean, var, logvar = gv.p_mean_variance(v_model, z_t.to(DEV), t.to(DEV), cond.to(DEV), clip_denoised=clip)
    out = gv.p_sample(v_model, z_t.to(DEV), t.to(DEV), cond.to(DEV), clip_denoised=clip, noise=noise.to(DEV))
    torch.cuda.synchronize()
    ab = gc.alphas_cumprod.double()[t].view(-1, 1, 1, 1, 1)
    v32 = v_model(z_t.to(DEV), t.to(DEV), cond.to(DEV)).cpu()
    eps = VR.convert(v32, z_t, VR.vp_rows(gc.alphas_cumprod, t.tolist()))
    b = lambda name: getattr(gc, name).double()[t].view(-1, 1, 1, 1, 1)
    x0 = (z_t.double() - b("sqrt_one_minus_alphas_cumprod") * eps) / b("sqrt_alphas_cumprod")
    if clip:
        x0 = x0.clamp(-1, 1)
    ref_mean = b("posterior_mean_coef1") * x0 + b("posterior_mean_coef2") * z_t.double()
    nz = (t != 0).double().view(-1, 1, 1, 1, 1)
    ref_out = ref_mean + nz * torch.exp(0.5 * b("posterior_log_variance_clipped")) * noise.double()
    e_mean = float((mean.cpu().double() - ref_mean).abs().max()) / float(ref_mean.abs().max())
    e_out = float((out.cpu().double() - ref_out).abs().max()) / float(ref_out.abs().max())
    print(f"single step clip={clip}: mean max err / max|mean| {e_mean:.2e}, p_sample {e_out:.2e}")
    assert e_mean <= 1e-5 and e_out <= 1e-5
    assert torch.equal(var.cpu(), gc._extract(gc.posterior_variance, t, shape))
    # the conversion and the z_0 prediction on the device against the restatement
    e_dev = gv.model_output_to_eps(z_t.to(DEV), t.to(DEV), v32.to(DEV)).cpu().double()
    mag = VR.convert_magnitude(v32, z_t, VR.vp_rows(gc.alphas_cumprod, t.tolist()))
    assert ((e_dev - eps).abs() <= 4 * U24 * mag).all()
    x0_dev = gv._predict_z_0_from_v(z_t.to(DEV), t.to(DEV), v32.to(DEV)).cpu().double()
    x0_ref = ab.sqrt() * z_t.double() - (1 - ab).sqrt() * v32.double()
    e_x0 = float((x0_dev - x0_ref).abs().max()) / float(x0_ref.abs().max())
    print(f"single step: _predict_z_0_from_v max err / max|z0| {e_x0:.2e}")
    assert e_x0 <= 1e-5
