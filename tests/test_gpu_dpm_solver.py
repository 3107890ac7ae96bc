"""GPU: DPM-Solver++(2M) (sampler.DPMSolverSampler, csrc/multistep.hip ctsi_dpm_step / ctsi_dpm_step_f32).

1. convergence order on an analytic model through the generic-callable path (exact eps of Gaussian data);
2. per-step parity of the engine U-Net runs against a float64 restatement of the update, bf16 and fp32 modes;
3. captured replay == eager, repeated calls and the history reset between volumes, bit for bit;
4. a batch of two == two single runs;  5. depth sharding (virtual ranks);  6. batched stitching;  7. generate()."""
import importlib
import logging
import time

import numpy as np
import pytest
import torch

from tests.helpers import TINY_UNET, formula_input, load_formula, rel_l2, tiny_model_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = importlib.import_module("video-to-video-diffusion_amd.engine")
E32 = importlib.import_module("video-to-video-diffusion_amd.engine_f32")
P = importlib.import_module("video-to-video-diffusion_amd.parallel")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
FULL_CFG = {'model': {'in_channels': 1, 'latent_dim': 8, 'vae_base_channels': 128, 'vae_scaling_factor': 1.0},
            'pretrained': {'use_pretrained': True, 'vae': {'enabled': True, 'checkpoint_path': 'unused'}},
            'noise_schedule': 'cosine', 'diffusion_timesteps': 1000}

# Gaussian data x0 ~ N(MU, SD^2) per element: the clamp at +-10 never binds (|x0_pred| stays near MU + |z|)
MU, SD = 0.5, 1.0


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _t_desc(g, n):
    return [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(n)]


def _analytic_model(g):
    """eps*(z, t) = sigma (z - alpha MU) / (alpha^2 SD^2 + sigma^2), evaluated in float64 and returned in fp32."""
    ac = g.alphas_cumprod.double().to(DEV)

    def model(z, t, c):
        ab = ac[t].view(-1, 1, 1, 1, 1)
        a, s = ab.sqrt(), (1 - ab).sqrt()
        return (s * (z.double() - a * MU) / (a * a * SD * SD + s * s)).float()
    return model


def _exact_endpoint(g, z_t):
    ab = float(g.alphas_cumprod.double()[999])
    a, s = np.sqrt(ab), np.sqrt(1 - ab)
    return MU + SD * (z_t.double() - a * MU) / np.sqrt(a * a * SD * SD + s * s)


def _restated(g, z_t, n, kind, order=2):
    """The same solver in float64 on the analytic eps (the fp32 rows the engine uses, widened)."""
    ac = g.alphas_cumprod.double()
    t_desc = _t_desc(g, n)
    z = z_t.double().clone()
    if kind == "dpmpp":
        rows = S.dpm_coef_rows(g.alphas_cumprod, t_desc, order).double()
        xp = torch.zeros_like(z)
    else:
        rows = S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0).double()
    for i, t in enumerate(t_desc):
        a, s = ac[t].sqrt(), (1 - ac[t]).sqrt()
        e = s * (z - a * MU) / (a * a * SD * SD + s * s)
        if kind == "dpmpp":
            x0 = (rows[i, 0] * z - rows[i, 1] * e).clamp(-10, 10)
            z = rows[i, 2] * z + rows[i, 3] * x0 + rows[i, 4] * xp
            xp = x0
        else:
            x0 = ((z - rows[i, 0] * e) / rows[i, 1]).clamp(-10, 10)
            z = rows[i, 2] * x0 + rows[i, 3] * e
    return z


# ---------------------------------------------------------------------------------------------------------------------
# 1. analytic convergence order (generic callable -> ctsi_dpm_step)
# ---------------------------------------------------------------------------------------------------------------------
# float64 calibration of this setup (MU 0.5, SD 1): DPM++(2M) endpoint error 6.8e-2 / 1.66e-2 / 3.44e-3 at N = 10 / 20 /
# 40 (observed order 2.04, 2.27); DDIM 0.115 / 5.95e-2 / 3.02e-2 (order ~1).  The engine adds the fp32 conditioning of
# the first step (1/alpha = 6.4e4 at t = 999): ~1e-4 on the endpoint.
def test_analytic_convergence_order(pkg):
    g = pkg.GaussianDiffusion()
    model = _analytic_model(g)
    shape = (2, 4, 8, 16, 16)
    z_t = _randn(shape, 1)
    cond = torch.zeros(shape, device=DEV)
    exact = _exact_endpoint(g, z_t)
    err_dpm, err_ddim = {}, {}
    for n in (10, 20, 40):
        out = pkg.DPMSolverSampler(g, model).sample(shape, cond, n, DEV, progress=False, z_init=z_t.to(DEV)).cpu()
        ddim = pkg.DDIMSampler(g, model).sample(shape, cond, n, DEV, progress=False, z_init=z_t.to(DEV)).cpu()
        err_dpm[n], err_ddim[n] = rel_l2(out, exact), rel_l2(ddim, exact)
        e_rest = rel_l2(out, _restated(g, z_t, n, "dpmpp"))
        print(f"N={n}: DPM++(2M) {err_dpm[n]:.3e}  DDIM {err_ddim[n]:.3e}  engine vs float64 restatement {e_rest:.2e}")
        assert torch.isfinite(out).all()
        assert e_rest < 2e-3, e_rest
        assert err_dpm[n] < 0.75 * err_ddim[n]
    p1, p2 = np.log2(err_dpm[10] / err_dpm[20]), np.log2(err_dpm[20] / err_dpm[40])
    q2 = np.log2(err_ddim[20] / err_ddim[40])
    print(f"observed order: DPM++(2M) {p1:.2f}, {p2:.2f}; DDIM {q2:.2f}")
    assert p1 > 1.7 and p2 > 1.7
    assert q2 < 1.3


def test_order1_matches_the_engine_ddim(pkg):
    """order=1 is DDIM in data-prediction form; the engine's DDIM keeps the reference's +1e-8 terms (sqrt(abar + 1e-8)
    at t = 999, where abar ~ 2.4e-10), so the two differ by what those terms make of the float64 trajectories."""
    g = pkg.GaussianDiffusion()
    model = _analytic_model(g)
    shape = (1, 4, 4, 16, 16)
    z_t = _randn(shape, 2)
    cond = torch.zeros(shape, device=DEV)
    for n in (10, 20):
        d1 = pkg.DPMSolverSampler(g, model, order=1).sample(shape, cond, n, DEV, progress=False, z_init=z_t.to(DEV))
        dd = pkg.DDIMSampler(g, model).sample(shape, cond, n, DEV, progress=False, z_init=z_t.to(DEV))
        bound = rel_l2(_restated(g, z_t, n, "dpmpp", 1), _restated(g, z_t, n, "ddim"))
        got = rel_l2(d1.cpu(), dd.cpu())
        print(f"N={n}: order-1 vs engine DDIM {got:.3e}; float64 bound from the +1e-8 terms {bound:.3e}")
        assert got <= 1.1 * bound + 2e-3


def test_scalar_kernel_path_and_nonfinite_logging(pkg, caplog):
    """Three channels (no 16-byte path) and an eps with NaN / Inf: sanitised like DDIM, counted and logged after the
    loop, and the history never carries a non-finite value."""
    g = pkg.GaussianDiffusion()
    base = _analytic_model(g)
    shape = (1, 3, 5, 7, 9)
    z_t = _randn(shape, 3)
    cond = torch.zeros(shape, device=DEV)
    out = pkg.DPMSolverSampler(g, base).sample(shape, cond, 10, DEV, progress=False, z_init=z_t.to(DEV)).cpu()
    assert rel_l2(out, _restated(g, z_t, 10, "dpmpp")) < 2e-3

    def bad(z, t, c):
        e = base(z, t, c)
        e[0, 0, 0, 0, 0] = float("nan")
        e[0, 1, 0, 0, 0] = float("inf")
        return e
    with caplog.at_level(logging.ERROR):
        out = pkg.DPMSolverSampler(g, bad).sample(shape, cond, 4, DEV, progress=False, z_init=z_t.to(DEV))
    assert torch.isfinite(out).all()
    text = caplog.text
    assert "NaN/Inf in noise_pred! NaN: 1, Inf: 1" in text


# ---------------------------------------------------------------------------------------------------------------------
# 2. per-step parity of the engine runs against the float64 update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_unet(pkg):
    un = pkg.UNet3D(**TINY_UNET)
    load_formula(un, 8)
    return un.to(DEV)


@pytest.fixture(scope="module")
def full_model(pkg):
    torch.manual_seed(0)
    return pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)


def _per_step_parity(g, unet, shape, n, precision, seed):
    cond = formula_input(shape, seed).to(DEV)
    z_t = _randn(shape, seed + 1)
    traj, eps = [], []
    prev = unet.inference_precision
    unet.inference_precision = precision
    try:
        out = S.run_sampler(g, unet, shape, cond, DEV, kind="dpmpp", t_desc=_t_desc(g, n), progress=False,
                            z_init=z_t.to(DEV), trajectory=traj, eps_trajectory=eps)
    finally:
        unet.inference_precision = prev
    steps = len(_t_desc(g, n))
    assert len(traj) == len(eps) == steps and torch.equal(traj[-1], out)
    rows = S.dpm_coef_rows(g.alphas_cumprod, _t_desc(g, n), 2).double()
    zs = [z_t.double()] + [t.cpu().double() for t in traj]
    xp = torch.zeros_like(zs[0])
    worst = 0.0
    for i in range(steps):
        e = eps[i].cpu().double()
        assert torch.isfinite(e).all()
        x0 = (rows[i, 0] * zs[i] - rows[i, 1] * e).clamp(-10, 10)
        zn = rows[i, 2] * zs[i] + rows[i, 3] * x0 + rows[i, 4] * xp
        err = rel_l2(zs[i + 1], zn)
        worst = max(worst, err)
        assert err < 1e-4, f"{precision} step {i}: {err:.3g}"
        xp = x0
    print(f"{precision} {tuple(shape)} DPM++-{n}: worst per-step rel-L2 vs float64 update {worst:.2e}")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_per_step_parity_tiny(pkg, tiny_unet, precision):
    _per_step_parity(pkg.GaussianDiffusion(), tiny_unet, (1, 8, 4, 8, 8), 6, precision, 20)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_per_step_parity_config1(pkg, full_model, precision):
    _per_step_parity(full_model.diffusion, full_model.unet, (1, 8, 48, 48, 48), 5, precision, 30)


# ---------------------------------------------------------------------------------------------------------------------
# 3. captured replay == eager; repeated calls and the history reset between volumes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_captured_equals_eager_and_history_resets(pkg, tiny_unet, precision):
    g = pkg.GaussianDiffusion()
    shape, n_steps = (1, 8, 4, 8, 8), 5
    cond_a, cond_b = formula_input(shape, 41).to(DEV), formula_input(shape, 42).to(DEV)
    za, zb = _randn(shape, 43).to(DEV), _randn(shape, 44).to(DEV)
    tiny_unet.inference_precision = precision
    try:
        sp = pkg.DPMSolverSampler(g, tiny_unet)
        b1 = sp.sample(shape, cond_b, n_steps, DEV, progress=False, z_init=zb)
        b2 = sp.sample(shape, cond_b, n_steps, DEV, progress=False, z_init=zb)
        sp.sample(shape, cond_a, n_steps, DEV, progress=False, z_init=za)       # leaves its own history behind
        b3 = sp.sample(shape, cond_b, n_steps, DEV, progress=False, z_init=zb)
        # the same step eagerly: a separate program, launch by launch (no graph)
        t_desc = _t_desc(g, n_steps)
        ctx = E.Ctx.get(torch.device(DEV))
        with ctx.scope():
            cls = E32.UNetProgramF32 if precision == "fp32" else E.UNetProgram
            prog = cls(ctx, tiny_unet, 1, 4, 8, 8, g.timesteps + 1, tiny_unet.attention_mode)
            prog.add_sampler_step("dpmpp", False)
            prog.load_latents(zb, cond_b)
            prog.set_schedule(t_desc, S.dpm_coef_rows(g.alphas_cumprod, t_desc, 2).to(DEV))
            for _ in t_desc:
                prog.run()
            eager = prog.z_ncdhw()
        torch.cuda.synchronize()
    finally:
        tiny_unet.inference_precision = "bf16"
    assert torch.isfinite(b1).all()
    assert torch.equal(b1, b2) and torch.equal(b1, b3)
    assert torch.equal(eager, b1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. a batch of two == two single runs
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_of_two_equals_two_single_runs(pkg, tiny_unet):
    g = pkg.GaussianDiffusion()
    shape = (2, 8, 4, 8, 8)
    cond = formula_input(shape, 50).to(DEV)
    z_t = _randn(shape, 51).to(DEV)
    tiny_unet.inference_precision = "fp32"        # batch-invariant arithmetic (the fp32 stitching bound is 1e-5)
    try:
        sp = pkg.DPMSolverSampler(g, tiny_unet)
        both = sp.sample(shape, cond, 6, DEV, progress=False, z_init=z_t)
        one = [sp.sample((1,) + shape[1:], cond[b:b + 1], 6, DEV, progress=False, z_init=z_t[b:b + 1]) for b in (0, 1)]
    finally:
        tiny_unet.inference_precision = "bf16"
    for b in (0, 1):
        assert rel_l2(both[b:b + 1].cpu(), one[b].cpu()) < 1e-5, (b, rel_l2(both[b:b + 1].cpu(), one[b].cpu()))


# ---------------------------------------------------------------------------------------------------------------------
# 5. depth sharding with virtual ranks (the tolerance of tests/test_gpu_sharded.py: the first step's +-10 clamp flips
#    a few elements under bf16-level perturbations of eps)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,world", [((1, 8, 4, 8, 8), 2), ((1, 8, 8, 8, 8), 3)])     # 3 + 3 + 2: ragged
def test_sharded_matches_unsharded(pkg, tiny_unet, shape, world):
    g = pkg.GaussianDiffusion()
    n, L, d, h, w = shape
    x, c = _randn(shape, 60), formula_input(shape, 61)
    t_desc = _t_desc(g, 4)
    coef = S.dpm_coef_rows(g.alphas_cumprod, t_desc, 2).to(DEV)
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope():
        ref = E.UNetProgram(ctx, tiny_unet, n, d, h, w, 8)
        ref.add_sampler_step("dpmpp", False)
        ref.load_latents(x, c)
        ref.set_schedule(t_desc, coef)
        comm = P.LocalComm(world)
        progs = []
        for r in range(world):
            spec = P.ShardSpec(r, world, comm, d)
            pr = E.UNetProgram(ctx, tiny_unet, n, spec.depth_local, h, w, 8, shard=spec)
            pr.add_sampler_step("dpmpp", False)
            pr.load_latents(x, c)
            pr.set_schedule(t_desc, coef)
            progs.append(pr)
        for i in range(len(t_desc)):
            ref.run()
            P.run_lockstep(progs)
            z_ref = ref.z_ncdhw().cpu()
            z = torch.cat([p.z_ncdhw() for p in progs], dim=2).cpu()
            if i == 0:
                eps = torch.cat([p.eps_ncdhw() for p in progs], dim=2).cpu()
                assert rel_l2(eps, ref.eps_ncdhw().cpu()) < 3e-2
            assert torch.isfinite(z).all()
            assert rel_l2(z, z_ref) < 0.15, (i, rel_l2(z, z_ref))
    torch.cuda.synchronize()


def test_sharded_sampler_runs_volume_by_volume(pkg, tiny_unet):
    """run_sampler_sharded on two volumes: the program runs one volume at a time, so step 0 of volume 2 must replace the
    history volume 1 left behind."""
    g = pkg.GaussianDiffusion()
    shape = (2, 8, 4, 8, 8)
    cond = formula_input(shape, 70).to(DEV)
    z_t = _randn(shape, 71).to(DEV)
    ref = pkg.DPMSolverSampler(g, tiny_unet).sample(shape, cond, 4, DEV, progress=False, z_init=z_t)

    class OneRank(P.LocalComm):
        rank = 0

    ctx = E.Ctx.get(torch.device(DEV))
    # volume 1 alone first (zeroed history), then after volume 0 in the same cached program
    single = S.run_sampler_sharded(g, tiny_unet, (1,) + shape[1:], cond[1:], ctx, z_t[1:], kind="dpmpp",
                                   t_desc=_t_desc(g, 4), eta=0.0, noise_fn=None, comm=OneRank(1))
    out = S.run_sampler_sharded(g, tiny_unet, shape, cond, ctx, z_t, kind="dpmpp", t_desc=_t_desc(g, 4), eta=0.0,
                                noise_fn=None, comm=OneRank(1))
    assert tuple(out.shape) == shape
    assert torch.equal(out[1:], single)
    assert rel_l2(out.cpu(), ref.cpu()) < 0.15


# ---------------------------------------------------------------------------------------------------------------------
# 6. batched sample_with_stitching == window by window
# ---------------------------------------------------------------------------------------------------------------------
def test_stitching_window_batch(pkg):
    from oracle import ref_ops as R
    model, sd, cfg = tiny_model_sd(pkg)
    model.to(DEV)
    v_full = formula_input((1, 1, 6, 40, 24), 17).clamp(-1, 1).to(DEV)
    sampler = pkg.DPMSolverSampler(model.diffusion, model.unet)
    kw = dict(patch_size=(4, 16, 16), target_patch_size=(4, 16, 16), stride=(2, 8, 8), device=DEV, progress=False)
    outs = {}
    for prec in ("bf16", "fp32"):
        model.set_inference_precision(prec)
        try:
            for wb in (1, None):
                torch.manual_seed(123)
                outs[prec, wb] = sampler.sample_with_stitching(v_full, model.vae, 3, window_batch=wb, **kw).cpu()
        finally:
            model.set_inference_precision("bf16")
    assert tuple(outs["bf16", 1].shape) == (1, 1, 6, 40, 24) and torch.isfinite(outs["bf16", 1]).all()
    assert R.psnr(outs["bf16", None], outs["bf16", 1], 2.0) > 45.0
    assert rel_l2(outs["fp32", None], outs["fp32", 1]) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 7. generate() end to end at config 1
# ---------------------------------------------------------------------------------------------------------------------
def test_generate_config1_dpmpp_2m(pkg, full_model):
    v_in = (torch.rand((1, 1, 8, 192, 192), generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    nf = lambda i, s: _randn(s, 900 + i).to(DEV)
    full_model.generate(v_in, 'dpmpp_2m', 20, target_depth=48, noise_fn=nf)      # plans, weight pack, capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = full_model.generate(v_in, 'dpmpp_2m', 20, target_depth=48, noise_fn=nf)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"config 1 generate('dpmpp_2m', 20): {dt * 1e3:.1f} ms warm")
    assert tuple(out.shape) == (1, 1, 48, 192, 192)
    assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0
    from inference.generate import generate_batch
    gb = generate_batch(full_model, v_in[:, :, :4, :64, :64].contiguous(), sampler_type='dpmpp_2m', num_inference_steps=3,
                        device=DEV, noise_fn=nf)
    assert torch.isfinite(gb).all()
