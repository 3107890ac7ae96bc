"""GPU: x0-form sampler updates and the zero-terminal-SNR schedule (csrc/x0_step.hip, x0_form.py,
GaussianDiffusion.update_form / rescale_zero_terminal_snr / loss_weighting).

 a. ctsi_x0_step / ctsi_x0_step_f32 against the float64 restatement (tests/x0_restatement.py), nonfinite counters included;
 b. the analytic Gaussian model through the generic-callable loop: every x0 sampler against the float64 chain, with the same
    arithmetic in torch fp32 as the yardstick, and the x0 form against the v eps form on the cosine schedule;
 c. the engine: every update re-derived from the launch's own audited operands, captured == eager, a batch of two == two single
    runs, guidance, fp32, depth sharding, poison-and-guard, and the eps form untouched around an x0 run;
 d. generate() on a rescaled model, all four samplers;
 e. training on the rescaled schedule under both loss weightings;
 f. p_mean_variance / p_sample with per-sample timesteps that include T-1.
The engine tests run the tiny U-Net at latents (2, 8, 4, 8, 8) / (1, 8, 4, 8, 8); the odd latent (1, 3, 3, 5, 7) -- three
channels, an odd element count: the one-element-per-thread path -- is run where no U-Net is involved (a, b, f): the tiny
U-Net's stride-2 level does not take odd extents.  Every measured figure is printed before it is asserted
(profiles/x0_form_tests.log is that output)."""
import ctypes as C
import importlib

import pytest
import torch

from tests import poison as PZ
from tests import vpred_restatement as VR
from tests import x0_restatement as XR
from tests.helpers import TINY_UNET, formula_input, formula_noise, load_formula, rel_l2, tiny_model_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = importlib.import_module("video-to-video-diffusion_amd.engine")
E32 = importlib.import_module("video-to-video-diffusion_amd.engine_f32")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
P = importlib.import_module("video-to-video-diffusion_amd.parallel")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
U24 = 2.0 ** -24
V = "v_prediction"
F64 = torch.float64
SHAPES = [(2, 8, 4, 8, 8), (1, 3, 3, 5, 7)]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _ndhwc(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _ncdhw(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _t_desc(g, n):
    return [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(n)]


def _keys(unet):
    return list(getattr(unet, "_ctsi_programs", {}).keys())


def _diffusion(pkg, schedule, form="x0"):
    """'cosine' / 'linear': the plain schedule of a v model in the given update form; '<name>-ztsnr': rescaled (x0)."""
    g = pkg.GaussianDiffusion(schedule.split("-")[0], prediction_type=V)
    if schedule.endswith("ztsnr"):
        return g.rescale_zero_terminal_snr()
    g.update_form = form
    return g


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


def _kernel_bounds(x_got, z_got, z, v, row, hist, noise):
    """(worst |X err| / bound, worst |z' err| / bound) of one launch against XR.kernel on NDHWC tensors:
    |X - X64| <= 4 * 2^-24 (|alpha z| + |sigma v|), |z' - z'64| <= 4 * 2^-24 (|a z| + |b X| + |c h| + |s n|) + |b| (bound on X)."""
    x64, z64, mag_x, mag = XR.kernel(z, v, row, hist, noise)
    bx = 4 * U24 * mag_x
    bz = 4 * U24 * mag + abs(float(row[3])) * bx
    ux = 0.0 if x_got is None else float(((x_got.double() - x64).abs() / bx.clamp_min(1e-300)).max())
    uz = float(((z_got.double() - z64).abs() / bz.clamp_min(1e-300)).max())
    return ux, uz


# ---------------------------------------------------------------------------------------------------------------------
# a. the kernel against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [10.0, 1.0, 0.0])
@pytest.mark.parametrize("operands", ["hist+noise", "none"])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_x0_step_against_float64(shape, f32, operands, clip):
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    n, Lc, d, h, w = shape
    full = operands == "hist+noise"
    z, v = 1.7 * _randn((n, d, h, w, Lc), 1) + 0.2, 1.3 * _randn((n, d, h, w, Lc), 2)
    hist = 0.9 * _randn((n, d, h, w, Lc), 3) if full else None
    noise = _randn(shape, 4) if full else None                      # NCDHW
    live = torch.tensor([0.62, 0.78, 0.55, 0.41, -0.23 if full else 0.0, 0.37 if full else 0.0, clip, 0.0])
    table = torch.stack([torch.full((8,), 5.0), live]).to(DEV).contiguous()       # row 0: a decoy, never used
    step = torch.ones(1, dtype=torch.int32, device=DEV)
    c_total, c_off = (2 * Lc + 4, 4) if Lc % 4 == 0 else (2 * Lc + 1, 1)
    zin = torch.full((n, d, h, w, c_total), 3.0, dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)
    nf = torch.zeros((2, 6), dtype=torch.int32, device=DEV)
    zd, vd = z.to(DEV), v.to(DEV)
    hd, nd = (None if t is None else t.to(DEV) for t in (hist, noise))
    fn = lib.x0_step_f32 if f32 else lib.x0_step
    with ctx.scope():
        fn(_ptr(zd), _ptr(vd), _ptr(hd), _ptr(nd), _ptr(zin), c_total, c_off, _ptr(table), _ptr(step), n, Lc, d, h, w,
           _ptr(nf), ctx.sptr)
    torch.cuda.synchronize()
    n_nd = None if noise is None else _ndhwc(noise)
    z_got = zd.cpu()
    ux, uz = _kernel_bounds(None if hd is None else hd.cpu(), z_got, z, v, live, hist, n_nd)
    print(f"x0_step {shape} {'fp32' if f32 else 'bf16'} zin, {operands}, clip {clip}: worst |err| / bound X {ux:.3f}, z' {uz:.3f}")
    assert ux <= 1.0 and uz <= 1.0
    if clip > 0 and hd is not None:
        assert float(hd.cpu().abs().max()) <= clip
        assert clip != 1.0 or bool((hd.cpu().abs() == 1.0).any())           # the clamp really bites at clip 1
    zs = zin.cpu().float()
    want = z_got if f32 else z_got.to(torch.bfloat16).float()
    assert torch.equal(zs[..., c_off:c_off + Lc], want)                    # the slice: z' in the slice's precision
    keep = torch.ones(c_total, dtype=torch.bool)
    keep[c_off:c_off + Lc] = False
    assert bool((zs[..., keep] == 3.0).all())                              # the neighbouring channels are untouched
    assert torch.equal(vd.cpu(), v) and (nd is None or torch.equal(nd.cpu(), noise))      # read only
    assert int(nf.abs().sum()) == 0


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_x0_step_counts_and_sanitises_nonfinite_values(shape, f32):
    """NaN / +-Inf in v are counted in columns 0, 1 and enter as 0 / +-1 (torch.nan_to_num), as ctsi_ddim_step treats its eps;
    a NaN / Inf of z reaches X (columns 2, 3) and z' (columns 4, 5), both sanitised.  Row = *step_ptr."""
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    n, Lc, d, h, w = shape
    z, v = _randn((n, d, h, w, Lc), 5), _randn((n, d, h, w, Lc), 6)
    fz, fv = z.view(-1), v.view(-1)
    fv[1], fv[7], fv[10], fv[-1] = float("nan"), float("inf"), float("-inf"), float("nan")
    fz[20], fz[33] = float("inf"), float("nan")
    row = torch.tensor([0.6, 0.8, 0.5, 0.4, 0.0, 0.0, 10.0, 0.0])
    table = torch.stack([torch.zeros(8), torch.zeros(8), row]).to(DEV).contiguous()
    step = torch.full((1,), 2, dtype=torch.int32, device=DEV)
    zin = torch.zeros((n, d, h, w, Lc), dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)
    hist = torch.zeros((n, d, h, w, Lc), device=DEV)
    nf = torch.zeros((4, 6), dtype=torch.int32, device=DEV)
    zd, vd = z.to(DEV), v.to(DEV)
    with ctx.scope():
        (lib.x0_step_f32 if f32 else lib.x0_step)(_ptr(zd), _ptr(vd), _ptr(hist), None, _ptr(zin), Lc, 0, _ptr(table),
                                                  _ptr(step), n, Lc, d, h, w, _ptr(nf), ctx.sptr)
    torch.cuda.synchronize()
    counts = nf.cpu()
    print(f"x0_step nonfinite {shape}: row 2 = {counts[2].tolist()}")
    assert counts[2].tolist() == [2, 2, 1, 1, 1, 1] and int(counts[[0, 1, 3]].abs().sum()) == 0
    x64, z64, _, _ = XR.kernel(z, v, row)
    z64 = XR.nan_to_num(z64)
    got_z, got_x = zd.cpu(), hist.cpu()
    assert bool(torch.isfinite(got_z).all()) and bool(torch.isfinite(got_x).all())
    assert float(got_x.view(-1)[20]) == 1.0 and float(got_x.view(-1)[33]) == 0.0
    assert float(got_z.view(-1)[20]) == 1.0 and float(got_z.view(-1)[33]) == 0.0
    assert bool(((got_z.double() - z64).abs() <= 1e-6 * (1 + z64.abs())).all())
    assert bool(((got_x.double() - x64).abs() <= 1e-6 * (1 + x64.abs())).all())


# ---------------------------------------------------------------------------------------------------------------------
# b. the analytic model through the generic-callable loop
# ---------------------------------------------------------------------------------------------------------------------
CASES = {"ddim-eta0": ("ddim", 0.0), "ddim-eta0.5": ("ddim", 0.5), "ddpm-12": ("ddpm", 0.0), "dpmpp-2": ("dpmpp", 0.0)}


def _sample_analytic(pkg, g, kind, eta, shape, cond, noises, model=None, **kw):
    """One run through sampler._run_generic; the callable is the analytic v* (fp32 out).  Returns (out, t_desc, plan)."""
    nf = lambda i, shp: noises[i].to(DEV)
    model = model or XR.analytic_callables(g.alphas_cumprod, DEV)[1]
    common = dict(progress=False, noise_fn=nf, **kw)
    if kind == "ddpm":
        t_desc = list(reversed(range(g.timesteps)))[:12]
        out = pkg.DDPMSampler(g, model).sample(shape, cond.to(DEV), DEV, num_steps=12, **common)
    elif kind == "ddim":
        t_desc = _t_desc(g, 10)
        out = pkg.DDIMSampler(g, model).sample(shape, cond.to(DEV), 10, DEV, eta=eta, **common)
    else:
        t_desc = _t_desc(g, 10)
        out = pkg.DPMSolverSampler(g, model, order=2).sample(shape, cond.to(DEV), 10, DEV, **common)
    return out.cpu(), t_desc, S._step_plan(g, kind, t_desc, eta, 2, None)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("schedule", ["cosine", "cosine-ztsnr", "linear-ztsnr"])
@pytest.mark.parametrize("shape", SHAPES)
def test_analytic_model_against_the_float64_chain(pkg, shape, schedule, case):
    """The engine's run against the float64 chain on the same (fp32, widened) rows, noise and v* callable.  Yardstick: the same
    chain with every update in torch fp32 on the same inputs; the engine may show 4 times its error (the margin of the
    section 18 tests)."""
    kind, eta = CASES[case]
    g = _diffusion(pkg, schedule)
    cond = formula_input(shape, 2)
    noises = {i: _randn(shape, 700 + i) for i in range(-1, 12)}
    out, t_desc, plan = _sample_analytic(pkg, g, kind, eta, shape, cond, noises)
    assert plan.x0 and (kind != "ddim" or eta == 0 or plan.with_noise)
    vm = XR.v_model(g.alphas_cumprod, cond)
    ref = XR.chain(plan.coef.double(), noises[-1], vm, t_desc, noises, F64)
    f32 = XR.chain(plan.coef, noises[-1], lambda z, t: vm(z, t).float(), t_desc, noises, torch.float32)
    e_eng = float((out.double() - ref).abs().max())
    e_f32 = float((f32.double() - ref).abs().max())
    print(f"analytic {case} {schedule} {shape}: max |err| vs float64: engine {e_eng:.3e}, torch fp32 {e_f32:.3e} "
          f"(ratio {e_eng / max(e_f32, 1e-300):.2f}); max|z| {float(ref.abs().max()):.3f}")
    assert bool(torch.isfinite(out).all())
    assert e_eng <= 4 * e_f32, (e_eng, e_f32)


def test_x0_form_against_the_eps_form_on_the_cosine_schedule(pkg):
    """DDIM-10 on the plain cosine schedule: the v eps form divides by alpha = 1.6e-5 at its first step; against the same
    float64 chain the x0 form's error must be at most 1/50 of it (a CPU simulation in fp32 gives 1/800)."""
    shape = SHAPES[0]
    cond = formula_input(shape, 2)
    noises = {-1: _randn(shape, 699)}
    gx, ge = _diffusion(pkg, "cosine"), _diffusion(pkg, "cosine", "eps")
    out_x, t_desc, plan = _sample_analytic(pkg, gx, "ddim", 0.0, shape, cond, noises)
    out_e, _, plan_e = _sample_analytic(pkg, ge, "ddim", 0.0, shape, cond, noises)
    assert plan.x0 and not plan_e.x0 and plan_e.pred is not None
    ref = XR.chain(plan.coef.double(), noises[-1], XR.v_model(gx.alphas_cumprod, cond), t_desc, None, F64)
    e_x, e_e = float((out_x.double() - ref).abs().max()), float((out_e.double() - ref).abs().max())
    print(f"DDIM-10 cosine v model: max |err| vs float64: x0 form {e_x:.3e}, eps form {e_e:.3e} (ratio 1/{e_e / e_x:.0f}); "
          f"max|z| {float(ref.abs().max()):.3f}")
    assert e_x <= e_e / 50, (e_x, e_e)


# ---------------------------------------------------------------------------------------------------------------------
# c. the engine
# ---------------------------------------------------------------------------------------------------------------------
def _eager_program(pkg, unet, g, kind, eta, shape, t_desc, precision, guided=None):
    ctx = E.Ctx.get(torch.device(DEV))
    n, Lc, d, h, w = shape
    plan = S._step_plan(g, kind, t_desc, eta, 2, None)
    cls = E32.UNetProgramF32 if precision == "fp32" else E.UNetProgram
    nb = 2 if guided else 1
    kw = dict(guided=True, rescale=guided[1] > 0) if guided else {}
    prog = cls(ctx, unet, n, d, h, w, (g.timesteps + 1) * nb * n, unet.attention_mode, prediction=V, **kw)
    prog.add_sampler_step(kind, plan.with_noise, update_form="x0")
    return ctx, plan, prog


@pytest.mark.parametrize("kind,eta,precision,schedule", [("ddim", 0.5, "bf16", "cosine-ztsnr"), ("dpmpp", 0.0, "fp32", "cosine"),
                                                         ("ddpm", 0.0, "bf16", "linear-ztsnr"), ("dpmpp", 0.0, "bf16", "cosine-ztsnr")])
def test_every_update_from_its_own_operands_and_captured_equals_eager(pkg, tiny_unet, kind, eta, precision, schedule):
    """A separately built program run launch by launch: before every ctsi_x0_step its audited operands are read back, after it
    its results, and the update is re-derived in float64 within the bounds of test a.  No ctsi_pred_to_eps launch exists.  The
    eager run's final state equals the public sampler's (a captured graph) bit for bit, and so does a second captured run."""
    g = _diffusion(pkg, schedule)
    shape = (2, 8, 4, 8, 8)
    n, Lc, d, h, w = shape
    cond, z_t = formula_input(shape, 20).to(DEV), _randn(shape, 21).to(DEV)
    t_desc = list(reversed(range(g.timesteps)))[:4] if kind == "ddpm" else _t_desc(g, 3)
    noises = {i: _randn(shape, 800 + i) for i in range(len(t_desc))}
    with _precision(tiny_unet, precision):
        ctx, plan, prog = _eager_program(pkg, tiny_unet, g, kind, eta, shape, t_desc, precision)
        names = [m[0] for m in prog.op_meta[prog.unet_op_count:]]
        assert names == ["sampler.step", "sampler.advance"] and "pred.to_eps" not in [m[0] for m in prog.op_meta]
        k = prog.unet_op_count
        rec = prog.op_audit[k]
        assert rec["kind"] == "x0_step" and rec["sampler"] == kind and rec["v"] is prog.eps and rec["z"] is prog.z
        assert (rec["hist"] is not None) == (kind == "dpmpp") and (rec["noise"] is not None) == plan.with_noise
        worst = [0.0, 0.0]
        with ctx.scope():
            prog.load_latents(z_t, cond)
            prog.set_schedule([t for t in plan.t for _ in range(n)], plan.coef.to(DEV), plan.pred)
            for e in range(len(t_desc)):
                if plan.noise_step[e] >= 0:
                    prog.noise.copy_(noises[plan.noise_step[e]].to(DEV))
                for op in prog.ops[:k]:
                    op()
                row = rec["coef"][int(rec["step_ptr"].item())].cpu()
                z0, v0 = rec["z"].cpu(), rec["v"].cpu()
                h0 = None if rec["hist"] is None else rec["hist"].cpu()
                n0 = None if rec["noise"] is None else _ndhwc(rec["noise"].cpu())
                prog.ops[k]()
                z1 = rec["z"].cpu()
                h1 = None if rec["hist"] is None else rec["hist"].cpu()
                zin = rec["zin"].t.cpu().float().view(n, d, h, w, -1)[..., :Lc]
                for op in prog.ops[k + 1:]:
                    op()
                assert torch.equal(row, plan.coef[e])
                ux, uz = _kernel_bounds(h1, z1, z0, v0, row, h0, n0)
                worst = [max(worst[0], ux), max(worst[1], uz)]
                assert torch.equal(zin, z1 if precision == "fp32" else z1.to(torch.bfloat16).float())
            eager = prog.z_ncdhw()
            assert int(prog.nonfinite.abs().sum()) == 0
        torch.cuda.synchronize()
        print(f"{kind} eta {eta} {precision} {schedule}: audit of {len(t_desc)} x0_step launches: worst |err| / bound X "
              f"{worst[0]:.3f}, z' {worst[1]:.3f}")
        assert worst[0] <= 1.0 and worst[1] <= 1.0
        nf = lambda i, shp: noises[i].to(DEV)
        runs = [S.run_sampler(g, tiny_unet, shape, cond, DEV, kind=kind, t_desc=t_desc, progress=False, eta=eta,
                              noise_fn=nf, z_init=z_t) for _ in range(2)]
    assert bool(torch.isfinite(runs[0]).all())
    assert torch.equal(runs[0], runs[1]) and torch.equal(eager, runs[0])
    key = [kk for kk in _keys(tiny_unet) if "x0" in kk and kk[0] == "sampler" and precision in kk and kk[7] == kind]
    assert key and all(V in kk for kk in key)


def test_batch_of_two_equals_two_single_runs(pkg, tiny_unet):
    g = _diffusion(pkg, "cosine-ztsnr")
    shape = (2, 8, 4, 8, 8)
    cond, z_t = formula_input(shape, 50).to(DEV), _randn(shape, 51).to(DEV)
    kw = dict(progress=False, guidance_scale=3.0, guidance_rescale=0.7)
    with _precision(tiny_unet, "fp32"):
        sp = pkg.DPMSolverSampler(g, tiny_unet)
        both = sp.sample(shape, cond, 4, DEV, z_init=z_t, **kw)
        one = [sp.sample((1,) + shape[1:], cond[b:b + 1], 4, DEV, z_init=z_t[b:b + 1], **kw) for b in (0, 1)]
    for b in (0, 1):
        err = rel_l2(both[b:b + 1].cpu(), one[b].cpu())
        print(f"fp32 guided x0 dpmpp: sample {b} of a batch of two vs alone rel-L2 {err:.3e}")
        assert err < 1e-5          # the figure of test_gpu_cfg.test_batch_of_two_equals_two_single_guided_runs


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_guided_x0_equals_guided_eps_form_from_step_1_onwards(pkg, tiny_unet, precision):
    """phi = 0 on the plain cosine schedule: the conversion is affine with the same sigma z in both branches and weights that
    sum to 1, so guiding the raw v is guiding eps.  The first step (alpha = 1.6e-5) is where the eps form loses its digits,
    so both forms run the remaining timesteps from the same state.  The 2e-3 of DESIGN section 15 is a figure for fp32
    arithmetic (its analytic-model test; its engine tests compare bf16 programs per evaluation, on the recorded state):
      - fp32: the two final latents, rel-L2 < 2e-3;
      - both precisions: every step of the eps form restarted from the x0 run's recorded state, rel-L2 < 2e-3 per step.
    In bf16 the final latents of two differently rounded updates are not comparable at that figure: a last-bit difference of
    z flips roundings of the U-Net's bf16 input (2^-8 each) and the s = 3 guidance carries them on.  Measured: 6.1e-3 between
    the two forms, printed beside what the eps form does to ITSELF when its initial state moves by one fp32 ulp."""
    gx, ge = _diffusion(pkg, "cosine"), _diffusion(pkg, "cosine", "eps")
    shape = (1, 8, 4, 8, 8)
    cond, z_t = formula_input(shape, 41).to(DEV), _randn(shape, 43).to(DEV)
    t_desc = _t_desc(gx, 5)[1:]
    kw = dict(kind="ddim", progress=False, guidance_scale=3.0, guidance_rescale=0.0)
    with _precision(tiny_unet, precision):
        raw_x, raw_e, traj_x = [], [], []
        out_x = S.run_sampler(gx, tiny_unet, shape, cond, DEV, t_desc=t_desc, z_init=z_t, eps_trajectory=raw_x,
                              trajectory=traj_x, **kw)
        out_e = S.run_sampler(ge, tiny_unet, shape, cond, DEV, t_desc=t_desc, z_init=z_t, eps_trajectory=raw_e, **kw)
        moved = S.run_sampler(ge, tiny_unet, shape, cond, DEV, t_desc=t_desc, z_init=z_t * (1.0 + 2.0 ** -23), **kw)
        states, per_step = [z_t] + traj_x, 0.0
        for i in range(len(t_desc)):
            one = []
            S.run_sampler(ge, tiny_unet, shape, cond, DEV, t_desc=t_desc[i:], z_init=states[i], trajectory=one, **kw)
            per_step = max(per_step, rel_l2(one[0].cpu(), traj_x[i].cpu()))
    err, self_err = rel_l2(out_x.cpu(), out_e.cpu()), rel_l2(moved.cpu(), out_e.cpu())
    # the first evaluation sees the same z: the x0 program's record is the guided v, the eps program's the guided eps
    rows = VR.vp_rows(gx.alphas_cumprod, t_desc[:1])
    conv = VR.convert(raw_x[0].cpu(), z_t.cpu(), rows)
    e0 = rel_l2(raw_e[0].cpu(), conv)
    print(f"{precision}: guided (s = 3) x0 vs eps form from step 1 onwards: final latents rel-L2 {err:.3e} (the eps form "
          f"against itself from a state one ulp away: {self_err:.3e}); worst single step from the recorded state "
          f"{per_step:.3e}; first guided eps vs the conversion of the first guided v {e0:.3e}")
    assert bool(torch.isfinite(out_x).all()) and e0 < 2e-3 and per_step < 2e-3
    assert precision != "fp32" or err < 2e-3


def test_guided_x0_with_rescale_against_the_restatement(pkg):
    """phi = 0.7 through the generic-callable loop on the analytic model: v_g = v_u + s (v_c - v_u), m = phi std(v_c) /
    std(v_g) + 1 - phi per sample on the MODEL OUTPUT (Lin et al.), v = m v_g, then the x0 update.  rel-L2 within 2e-3."""
    g = _diffusion(pkg, "cosine-ztsnr")
    shape, s, phi = (2, 8, 4, 8, 8), 2.5, 0.7
    cond = formula_input(shape, 2)
    noises = {-1: _randn(shape, 1)}
    vc, vu = XR.v_model(g.alphas_cumprod, cond), XR.v_model(g.alphas_cumprod, torch.zeros_like(cond))

    def guided(z, t):
        c, u = vc(z, t), vu(z, t)
        gd = u + s * (c - u)
        std = lambda x: x.reshape(x.shape[0], -1).std(dim=1).view(-1, 1, 1, 1, 1)
        return (phi * std(c) / std(gd) + 1 - phi) * gd

    for kind in ("ddim", "dpmpp"):
        out, t_desc, plan = _sample_analytic(pkg, g, kind, 0.0, shape, cond, noises, guidance_scale=s, guidance_rescale=phi)
        ref = XR.chain(plan.coef.double(), noises[-1], guided, t_desc, None, F64)
        err = rel_l2(out, ref)
        print(f"guided x0 {kind} s={s} phi={phi} on the rescaled cosine schedule: rel-L2 {err:.3e}")
        assert bool(torch.isfinite(out).all()) and err < 2e-3


def test_sharded_x0_sampling_world2(pkg, tiny_unet):
    """World 2 in lock-step on one GPU, as tests/test_gpu_vpred.py drives its ranks: DDIM-3 from T-1 of the rescaled schedule
    at latent depth 4, sharded against unsharded, within that test's figures (raw output 3e-2, z 0.15)."""
    g = _diffusion(pkg, "cosine-ztsnr")
    shape = (1, 8, 4, 8, 8)
    n, Lc, d, h, w = shape
    x, c = formula_input(shape, 10), formula_input(shape, 11)
    t_desc = _t_desc(g, 3)
    plan = S._step_plan(g, "ddim", t_desc, 0.0, 2, None)
    ctx = E.Ctx.get(torch.device(DEV))
    world = 2
    with ctx.scope():
        ref = E.UNetProgram(ctx, tiny_unet, n, d, h, w, 8, prediction=V)
        ref.add_sampler_step("ddim", False, update_form="x0")
        ref.load_latents(x, c)
        ref.set_schedule(t_desc, plan.coef.to(DEV), plan.pred)
        ref.run()
        v_ref = ref.eps_ncdhw().cpu()
        for _ in t_desc[1:]:
            ref.run()
        z_ref = ref.z_ncdhw().cpu()
        comm = P.LocalComm(world)
        progs = []
        for r in range(world):
            spec = P.ShardSpec(r, world, comm, d)
            pr = E.UNetProgram(ctx, tiny_unet, n, spec.depth_local, h, w, 8, shard=spec, prediction=V)
            pr.add_sampler_step("ddim", False, update_form="x0")
            pr.load_latents(x, c)
            pr.set_schedule(t_desc, plan.coef.to(DEV), plan.pred)
            progs.append(pr)
        assert not any(m[0] == "pred.to_eps" for m in progs[0].op_meta)
        assert sum(1 for a in progs[0].op_audit if a and a.get("kind") == "x0_step") == 1
        P.run_lockstep(progs)
        v = torch.cat([p.eps_ncdhw() for p in progs], dim=2).cpu()
        P.run_lockstep(progs, launches=len(t_desc) - 1)
        z = torch.cat([p.z_ncdhw() for p in progs], dim=2).cpu()
    torch.cuda.synchronize()
    e_v, e_z = rel_l2(v, v_ref), rel_l2(z, z_ref)
    print(f"sharded x0 world 2: raw v rel-L2 {e_v:.3e}, z after {len(t_desc)} evaluations rel-L2 {e_z:.3e}")
    assert bool(torch.isfinite(z).all()) and e_v < 3e-2 and e_z < 0.15

    class OneRank(P.LocalComm):
        rank = 0

    out = S.run_sampler_sharded(g, tiny_unet, shape, c.to(DEV), ctx, x.to(DEV), kind="ddim", t_desc=t_desc, eta=0.0,
                                noise_fn=lambda i, s_: x, comm=OneRank(1))
    e_pub = rel_l2(out.cpu(), z_ref)
    print(f"sharded x0, run_sampler_sharded on one rank vs unsharded: rel-L2 {e_pub:.3e}")
    assert e_pub < 0.15
    assert any(k[0] == "sampler-shard" and "x0" in k for k in _keys(tiny_unet))


def _ztsnr_model(pkg):
    base, _, _ = tiny_model_sd(pkg)
    m = pkg.VideoToVideoDiffusion({**base.config, 'prediction_type': V, 'zero_terminal_snr': True}).eval()
    sd = base.state_dict()
    sd.update({"diffusion." + k: v for k, v in m.diffusion.state_dict().items()})
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def test_poison_x0_sampler(pkg):
    model = _ztsnr_model(pkg)
    assert model.diffusion.update_form == "x0" and float(model.diffusion.alphas_cumprod[-1]) == 0.0
    shape = (1, 8, 5, 6, 10)
    cond = formula_input(shape, 12).to(DEV)
    nf = lambda i, shp: formula_noise(i, shp).to(DEV)

    def sample():
        traj = []
        out = pkg.DPMSolverSampler(model.diffusion, model.unet).sample(shape, cond, 3, DEV, progress=False, noise_fn=nf,
                                                                       trajectory=traj, guidance_scale=2.5)
        out2 = pkg.DDIMSampler(model.diffusion, model.unet).sample(shape, cond, 3, DEV, eta=0.5, progress=False, noise_fn=nf)
        torch.cuda.synchronize()
        return {"z0": out, "trajectory": traj, "ddim": out2}

    PZ.run_scenario(sample, name="x0-sample[dpmpp,cfg + ddim,eta]", modules=[model], ragged=True, inside=PZ.reevaluate(sample))
    model.invalidate_engine_cache()


def test_eps_form_generate_is_bit_identical_around_an_x0_run(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    v_in = formula_input((1, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    nf = lambda i, shp: _randn(shp, 900 + i).to(DEV)
    d = model.diffusion
    d.prediction_type = V                          # the same weights read as a v model, eps form
    before = model.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf)
    keys = _keys(model.unet)
    assert keys and not any("x0" in k for k in keys)
    d.update_form = "x0"
    try:
        as_x0 = model.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf)
    finally:
        d.update_form = "eps"
    x0_keys = [k for k in _keys(model.unet) if "x0" in k]
    assert len(x0_keys) == 1 and [k for k in _keys(model.unet) if "x0" not in k] == keys
    after = model.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf)
    assert bool(torch.isfinite(as_x0).all()) and not torch.equal(as_x0, before)
    assert torch.equal(before, after)
    assert [k for k in _keys(model.unet) if "x0" not in k] == keys
    # and an 'epsilon' model is untouched as well
    d.prediction_type = "epsilon"
    e1 = model.generate(v_in, "dpmpp_2m", 3, target_depth=4, noise_fn=nf)
    d.prediction_type, d.update_form = V, "x0"
    model.generate(v_in, "dpmpp_2m", 3, target_depth=4, noise_fn=nf)
    d.prediction_type, d.update_form = "epsilon", "eps"
    assert torch.equal(model.generate(v_in, "dpmpp_2m", 3, target_depth=4, noise_fn=nf), e1)


# ---------------------------------------------------------------------------------------------------------------------
# d. generate() end to end on a rescaled model
# ---------------------------------------------------------------------------------------------------------------------
def _x0_programs(unet):
    return [p for k, p in unet._ctsi_programs.items() if "x0" in k]


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m", "heun"])
def test_generate_on_a_rescaled_model(pkg, sampler):
    model = _ztsnr_model(pkg)
    v_in = formula_input((1, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    nf = lambda i, shp: _randn(shp, 900 + i).to(DEV)
    out = model.generate(v_in, sampler, 4, target_depth=4, noise_fn=nf)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 1, 4, 16, 16) and bool(torch.isfinite(out).all())
    progs = [p for k, p in model.unet._ctsi_programs.items() if k[0] == "sampler"]
    assert len(progs) == 1 and int(progs[0].nonfinite.abs().sum()) == 0
    assert (len(_x0_programs(model.unet)) == 1) == (sampler != "heun")            # Heun keeps its eps-form program
    print(f"generate({sampler!r}) on the rescaled tiny model: finite, nonfinite table all zero, |out| max "
          f"{float(out.abs().max()):.3f}")
    model.invalidate_engine_cache()


def test_ddim_and_ddpm_trajectories_on_a_rescaled_model(pkg):
    """The latent trajectory of DDIM-4 from T-1 equals the restated chain on the program's own raw outputs, step by step within
    the kernel's bound; DDPM runs a 6-step prefix from T-1 (generate() itself always runs all T)."""
    model = _ztsnr_model(pkg)
    g = model.diffusion
    shape = (1, 8, 4, 4, 4)
    cond, z_t = formula_input(shape, 60).to(DEV), _randn(shape, 61).to(DEV)
    traj, raw = [], []
    out = S.run_sampler(g, model.unet, shape, cond, DEV, kind="ddim", t_desc=_t_desc(g, 4), progress=False, z_init=z_t,
                        trajectory=traj, eps_trajectory=raw)
    plan = S._step_plan(g, "ddim", _t_desc(g, 4), 0.0, 2, None)
    assert len(traj) == len(raw) == 5 and plan.t[0] == g.timesteps - 1 and float(plan.coef[0, 0]) == 0.0
    z, worst = z_t.cpu(), 0.0
    for i in range(5):
        _, uz = _kernel_bounds(None, traj[i].cpu(), z, raw[i].cpu(), plan.coef[i], None, None)
        worst, z = max(worst, uz), traj[i].cpu()
    print(f"DDIM-4 on the rescaled tiny model: trajectory vs the restated chain on the program's raw v: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0 and torch.equal(out, traj[-1]) and bool(torch.isfinite(out).all())
    nf = lambda i, shp: _randn(shp, 300 + i).to(DEV)
    o2 = pkg.DDPMSampler(g, model.unet).sample(shape, cond, DEV, progress=False, noise_fn=nf, num_steps=6)
    progs = _x0_programs(model.unet)
    assert bool(torch.isfinite(o2).all()) and len(progs) == 2 and all(int(p.nonfinite.abs().sum()) == 0 for p in progs)
    model.invalidate_engine_cache()


def test_stitching_and_ema_weights_on_a_rescaled_model(pkg):
    """sample_with_stitching drives the same step programs: two windows as one batch equal the windows one by one (fp32, the
    1e-5 of test_gpu_cfg.test_guided_stitching_equals_window_by_window), through x0 programs only.  `with ema.applied()`
    samples the averaged weights and restores the live ones: the same generate() before and after, bit for bit."""
    model = _ztsnr_model(pkg)
    v_full = formula_input((1, 1, 4, 16, 24), 17).clamp(-1, 1).to(DEV)            # two windows along w
    sampler = pkg.DPMSolverSampler(model.diffusion, model.unet)
    kw = dict(patch_size=(4, 16, 16), target_patch_size=(4, 16, 16), stride=(2, 8, 8), device=DEV, progress=False)
    outs = {}
    model.set_inference_precision("fp32")
    try:
        for wb in (1, None):
            torch.manual_seed(123)
            outs[wb] = sampler.sample_with_stitching(v_full, model.vae, 3, window_batch=wb, **kw).cpu()
    finally:
        model.set_inference_precision("bf16")
    err = rel_l2(outs[None], outs[1])
    print(f"fp32 x0 stitching on the rescaled tiny model: two windows as one batch vs one by one rel-L2 {err:.3e}")
    assert tuple(outs[1].shape) == (1, 1, 4, 16, 24) and bool(torch.isfinite(outs[1]).all()) and err < 1e-5
    keys = [k for k in _keys(model.unet) if k[0] == "sampler"]
    assert keys and all("x0" in k for k in keys)
    v_in = formula_input((1, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    nf = lambda i, shp: _randn(shp, 900 + i).to(DEV)
    ema = pkg.EMAWeights(model, decay=0.5, warmup=False)
    with torch.no_grad():
        for prm in model.unet.parameters():
            prm.mul_(1.01)
    ema.update()
    live = model.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf)
    with ema.applied():
        averaged = model.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf)
    again = model.generate(v_in, "ddim", 3, target_depth=4, noise_fn=nf)
    assert bool(torch.isfinite(averaged).all()) and not torch.equal(averaged, live) and torch.equal(again, live)
    model.invalidate_engine_cache()


# ---------------------------------------------------------------------------------------------------------------------
# e. training on the rescaled schedule
# ---------------------------------------------------------------------------------------------------------------------
TRAIN_SHAPE = (2, 8, 2, 6, 6)


def _train_inputs():
    return formula_input(TRAIN_SHAPE, 31), formula_input(TRAIN_SHAPE, 32), formula_noise(-1, TRAIN_SHAPE)


@pytest.mark.parametrize("weighting", ["min_snr", "uniform"])
def test_training_loss_on_the_rescaled_schedule(pkg, tiny_unet, weighting):
    """t = [37, T-1].  The per-sample factor against float64 (2 * 2^-24, the bound of the v test), and the loss within 6e-8
    relative of float64 on the program's own buffers (prediction, v target, norm): fp64 accumulation, one rounding."""
    g = _diffusion(pkg, "cosine-ztsnr").to(DEV)
    g.loss_weighting = weighting
    gc = _diffusion(pkg, "cosine-ztsnr")
    z0, cond, noise = _train_inputs()
    t = torch.tensor([37, g.timesteps - 1])
    for p in tiny_unet.parameters():
        p.grad = None
    loss, ld = g.training_loss(tiny_unet, z0.to(DEV), cond.to(DEV), t=t.to(DEV), noise=noise.to(DEV))
    torch.cuda.synchronize()
    assert set(ld) == {"mse", "total"}
    B, Lc, d, h, w = TRAIN_SHAPE
    prog = [p for k, p in tiny_unet._ctsi_programs.items() if k[0] == "unet-train" and k[2:6] == (B, d, h, w) and V in k]
    assert len(prog) == 1
    prog = prog[0]
    wgt = VR.min_snr_weight_v(gc.alphas_cumprod, t) if weighting == "min_snr" else torch.ones(2, dtype=F64)
    norm = wgt / float(B * Lc * d * h * w)
    n_err = float(((prog.norm.cpu().double() - norm).abs() / norm.clamp_min(1e-300)).max())
    assert weighting == "uniform" or float(prog.norm.cpu()[1]) == 0.0
    pred = _ncdhw(prog.eps.cpu()).double()
    vt = prog.v_target.cpu().double()
    a, s = gc.sqrt_alphas_cumprod[t], gc.sqrt_one_minus_alphas_cumprod[t]
    vt64 = VR.v_target(a, s, z0, noise)
    assert bool(((vt - vt64).abs() <= 3 * U24 * ((VR._b(a, z0) * noise.double()).abs() + (VR._b(s, z0) * z0.double()).abs())).all())
    assert torch.equal(vt[1], -z0[1].double())                   # at abar = 0 the target is -z_0 exactly
    ref = float((prog.norm.cpu().double() * ((pred - vt) ** 2).reshape(B, -1).sum(1)).sum())
    rel = abs(loss.item() - ref) / abs(ref)
    print(f"training on the rescaled schedule [{weighting}]: loss {loss.item():.6f} float64 {ref:.6f} rel {rel:.2e}; "
          f"norm rel {n_err:.2e}")
    assert n_err <= 2 * U24 and rel <= 6e-8


def test_terminal_step_is_trained_only_under_uniform_weighting(pkg):
    un = pkg.UNet3D(**TINY_UNET)
    load_formula(un, 8)
    un.to(DEV).train()
    shape = (1,) + TRAIN_SHAPE[1:]
    z0, cond, noise = (x[:1].to(DEV) for x in _train_inputs())
    g = _diffusion(pkg, "cosine-ztsnr").to(DEV)
    t = torch.tensor([g.timesteps - 1], device=DEV)
    grads = {}
    for weighting in ("min_snr", "uniform"):
        g.loss_weighting = weighting
        for p in un.parameters():
            p.grad = None
        loss, _ = g.training_loss(un, z0, cond, t=t, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
        gw = un.conv_out[2].weight.grad
        grads[weighting] = (loss.item(), float(gw.float().abs().max()))
        print(f"single sample at t = T-1 [{weighting}]: loss {loss.item():.6f}, max |conv_out grad| {grads[weighting][1]:.3e}")
    assert grads["min_snr"] == (0.0, 0.0)
    assert grads["uniform"][0] > 0.0 and grads["uniform"][1] > 0.0
    # one FusedAdamW step lowers the uniform loss on a fixed batch that holds T-1
    z0, cond, noise = (x.to(DEV) for x in _train_inputs())
    tt = torch.tensor([37, g.timesteps - 1], device=DEV)
    opt = pkg.FusedAdamW(list(un.parameters()), lr=2e-4, engine_modules=[un])
    losses = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        loss, _ = g.training_loss(un, z0, cond, t=tt, noise=noise)
        losses.append(loss.item())
        if len(losses) == 1:
            loss.backward()
            opt.step()
    print(f"uniform loss before / after one FusedAdamW step: {losses[0]:.6f} / {losses[1]:.6f}")
    assert losses[1] < losses[0]
    assert shape[0] == 1


# ---------------------------------------------------------------------------------------------------------------------
# f. the single-step API
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("shape", [(3, 8, 2, 4, 4), (3, 3, 3, 5, 7)])
def test_single_step_api_with_per_sample_timesteps(pkg, shape, clip):
    """p_mean_variance / p_sample at t = [T-1, 500, 0] of the rescaled schedule against float64, within the kernel's bounds:
    X = alpha z - sigma v (clamped to [-1, 1] with clip_denoised), mean = coef1 X + coef2 z, sample = mean + [t != 0]
    exp(logvar / 2) noise."""
    g, gc = _diffusion(pkg, "cosine-ztsnr").to(DEV), _diffusion(pkg, "cosine-ztsnr")
    z_t, cond, noise = _randn(shape, 3), formula_input(shape, 4), _randn(shape, 5)
    t = torch.tensor([g.timesteps - 1, 500, 0])
    v_model = XR.analytic_callables(gc.alphas_cumprod, DEV)[1]
    mean, var, logvar = g.p_mean_variance(v_model, z_t.to(DEV), t.to(DEV), cond.to(DEV), clip_denoised=clip)
    out = g.p_sample(v_model, z_t.to(DEV), t.to(DEV), cond.to(DEV), clip_denoised=clip, noise=noise.to(DEV))
    torch.cuda.synchronize()
    v32 = v_model(z_t.to(DEV), t.to(DEV), cond.to(DEV)).cpu()
    rows = XR.rows(gc, "ddpm", t.tolist())
    rows[:, 6] = 1.0 if clip else 0.0
    assert float(rows[0, 0]) == 0.0 and float(rows[2, 5]) == 0.0
    worst = [0.0, 0.0]
    for b in range(3):
        r_mean = rows[b].clone()
        r_mean[5] = 0.0
        _, um = _kernel_bounds(None, mean[b].cpu(), z_t[b], v32[b], r_mean.float(), None, None)
        _, uo = _kernel_bounds(None, out[b].cpu(), z_t[b], v32[b], rows[b].float(), None, noise[b])
        worst = [max(worst[0], um), max(worst[1], uo)]
    print(f"single step {shape} clip={clip}: worst |err| / bound: mean {worst[0]:.3f}, p_sample {worst[1]:.3f}")
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(out).all())
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    assert torch.equal(var.cpu(), gc._extract(gc.posterior_variance, t, shape))
    assert torch.equal(logvar.cpu(), gc._extract(gc.posterior_log_variance_clipped, t, shape))
    x0_dev = g._predict_z_0_from_v(z_t.to(DEV), t.to(DEV), v32.to(DEV)).cpu()
    assert torch.equal(x0_dev[0], -v32[0])                       # alpha = 0, sigma = 1: z_0 = -v, no division anywhere
