"""GPU: data consistency through the public interface on the tiny model of tests/helpers.py --
`model.data_consistency` in generate(), `sampler.data_consistency` in sample_with_stitching (projected once, after the blend),
`SliceProfile.measure` under autograd (first and second order) and in a VAE training step, `measurement_residual`, and the
refusal under depth sharding.  With the attribute None the C-ABI calls and the bits are those of a plain run."""
import contextlib
import importlib
import logging

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R
from tests.helpers import formula_input, formula_noise, rel_l2, tiny_model_sd
from tests.test_gpu_consistency_ops import check_2x, mv, ulp32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CS = importlib.import_module("video-to-video-diffusion_amd.consistency")
E = importlib.import_module("video-to-video-diffusion_amd.engine")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
MT = importlib.import_module("video-to-video-diffusion_amd.metrics")


@pytest.fixture(scope="module")
def tiny(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    yield model
    model.data_consistency = None
    model.invalidate_engine_cache()


@contextlib.contextmanager
def recorded_calls():
    """The names of the C-ABI entry points called through the binding, in order (every launch of the engine is one)."""
    lib, names, saved = L.get_lib(), [], {}
    for full in L.SIGNATURES:
        short = full[len("ctsi_"):]
        saved[short] = fn = getattr(lib, short)

        def wrap(*a, _fn=fn, _name=short):
            names.append(_name)
            return _fn(*a)

        setattr(lib, short, wrap)
    try:
        yield names
    finally:
        for short, fn in saved.items():
            setattr(lib, short, fn)


def exactness(prof, got, plain, thick, dc):
    """max |thick - W got| in float64 against twice that of the torch-fp32 restatement of the projection plus one ulp."""
    W32, P32, W64 = (torch.from_numpy(a) for a in (prof.W32, prof.P32, prof.W))
    t32 = plain.clone()
    for _ in range(dc.iterations):
        t32 = t32 + mv(P32, thick - mv(W32, t32))
    q_k = float((thick.double() - mv(W64, got.double())).abs().max())
    q_t = float((thick.double() - mv(W64, t32.double())).abs().max())
    bound = 2.0 * q_t + ulp32(float(got.abs().max()))
    print(f"  exactness max|y - W x|: kernel {q_k:.3e}  torch-fp32 {q_t:.3e}  bound {bound:.3e}")
    assert q_k <= bound
    return q_k


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_generate(tiny, sampler, precision):
    v_in = formula_input((1, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    kw = dict(num_inference_steps=3, target_depth=4, noise_fn=formula_noise, precision=precision)
    tiny.data_consistency = None
    tiny.generate(v_in, sampler, **kw)                    # builds and caches the programs
    with recorded_calls() as calls_a:
        plain = tiny.generate(v_in, sampler, **kw)
    with recorded_calls() as calls_b:
        again = tiny.generate(v_in, sampler, **kw)
    torch.cuda.synchronize()
    assert torch.equal(plain, again) and calls_a == calls_b and not any(n.startswith("depth_") for n in calls_a)
    dc = CS.DataConsistency()
    tiny.data_consistency = dc
    try:
        with recorded_calls() as calls_c:
            got = tiny.generate(v_in, sampler, **kw)
        torch.cuda.synchronize()
        stats = dc.last_stats
    finally:
        tiny.data_consistency = None
    # the plain launches, then the projection as the last device step
    assert calls_c == calls_a + ["depth_project_blocks", "depth_project", "depth_project_finalize"]
    assert got.shape == plain.shape == (1, 1, 4, 16, 16)
    want = CS.DataConsistency().project(plain, v_in)
    assert torch.equal(got, want) and not torch.equal(got, plain)
    print(f"\n[generate {sampler} {precision}]")
    exactness(dc.profile(2, 4), got, plain, v_in, dc)
    assert stats.shape == (1, 5) and float(stats[0, 0]) > float(stats[0, 1]) and float(stats[0, 2]) > float(stats[0, 3])
    print(f"  residual rms before {(float(stats[0, 0]) / v_in.numel()) ** 0.5:.3e} after {(float(stats[0, 1]) / v_in.numel()) ** 0.5:.3e}")
    # afterwards the default path is back, bit for bit
    assert torch.equal(tiny.generate(v_in, sampler, **kw), plain)


def test_generate_ignores_the_attribute_when_the_depth_stays(tiny, caplog):
    v_in = formula_input((1, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    kw = dict(num_inference_steps=2, noise_fn=formula_noise)
    plain = tiny.generate(v_in, "ddim", **kw)
    tiny.data_consistency = CS.DataConsistency()
    tiny._consistency_warned = False
    try:
        with caplog.at_level(logging.WARNING, logger="video-to-video-diffusion_amd.model"):
            with recorded_calls() as calls:
                a = tiny.generate(v_in, "ddim", **kw)
                b = tiny.generate(v_in, "ddim", **kw)
    finally:
        tiny.data_consistency = None
    assert torch.equal(a, plain) and torch.equal(b, plain) and not any(n.startswith("depth_") for n in calls)
    assert sum("data_consistency" in r.getMessage() for r in caplog.records) == 1


STITCH = dict(patch_size=(4, 16, 16), target_patch_size=(12, 16, 16), stride=(2, 12, 4), device=DEV, progress=False)


@pytest.mark.parametrize("kind,fusion", [("ddim", "pixel"), ("ddim", "latent"), ("dpmpp", "latent"), ("heun", "pixel"),
                                         ("ddpm", "pixel")])
def test_stitching_projects_the_full_volume_once(pkg, tiny, kind, fusion):
    v_full = formula_input((1, 1, 6, 32, 24), 17).clamp(-1, 1).to(DEV)
    if kind == "ddpm":
        sampler, steps = S.DDPMSampler(pkg.GaussianDiffusion("cosine", 8), tiny.unet), ()
    else:
        cls = {"ddim": S.DDIMSampler, "dpmpp": S.DPMSolverSampler, "heun": S.HeunSampler}[kind]
        sampler, steps = cls(tiny.diffusion, tiny.unet), (3,)
    assert sampler.data_consistency is None

    def run():
        torch.manual_seed(7)
        with recorded_calls() as calls:
            out = sampler.sample_with_stitching(v_full, tiny.vae, *steps, fusion=fusion, **STITCH)
        torch.cuda.synchronize()
        return out, calls

    plain, calls0 = run()
    dc = CS.DataConsistency(clamp=(-1.0, 1.0), iterations=2)
    sampler.data_consistency = dc
    got, calls1 = run()
    assert plain.shape == got.shape == (1, 1, 18, 32, 24)
    assert calls0.count("depth_project") == 0 and calls1.count("depth_project") == 1 and calls1[-1] == "depth_project_finalize"
    want = CS.DataConsistency(clamp=(-1.0, 1.0), iterations=2).project(plain, v_full)
    assert torch.equal(got, want) and not torch.equal(got, plain)
    assert (6, 18) in dc._profiles and len(dc._profiles) == 1        # the profile of the full depths, not of a window
    stats = dc.last_stats
    assert float(stats[0, 0]) > float(stats[0, 1])
    sampler.data_consistency = None
    assert torch.equal(run()[0], plain)


def test_stitching_without_a_depth_change_warns_once(tiny, caplog):
    v_full = formula_input((1, 1, 4, 32, 24), 17).clamp(-1, 1).to(DEV)
    sampler = S.DDIMSampler(tiny.diffusion, tiny.unet)
    kw = dict(patch_size=(4, 16, 16), target_patch_size=(4, 16, 16), stride=(2, 12, 4), device=DEV, progress=False)

    def run():
        torch.manual_seed(7)
        return sampler.sample_with_stitching(v_full, tiny.vae, 2, **kw)

    plain = run()
    sampler.data_consistency = CS.DataConsistency()
    with caplog.at_level(logging.WARNING, logger="video-to-video-diffusion_amd.sampler"):
        with recorded_calls() as calls:
            a, b = run(), run()
    assert torch.equal(a, plain) and torch.equal(b, plain) and not any(n.startswith("depth_") for n in calls)
    assert sum("data_consistency" in r.getMessage() for r in caplog.records) == 1


def _autograd_case(prof, dtype, dev, einsum):
    x = torch.tanh(formula_input((2, 1, prof.d_out, 5, 7), 31)).to(device=dev, dtype=dtype).requires_grad_(True)
    a = formula_input((2, 1, prof.d_in, 5, 7), 32).to(device=dev, dtype=dtype)
    b = formula_input((2, 1, prof.d_out, 5, 7), 33).to(device=dev, dtype=dtype)
    y = mv(torch.from_numpy(prof.W32), x) if einsum else prof.measure(x)
    loss = (y * a).sum() + 0.5 * (y * y * a).sum()
    g, = torch.autograd.grad(loss, x, create_graph=True)
    gg, = torch.autograd.grad((g * b).sum(), x)
    return y.detach(), g.detach(), gg.detach()


@pytest.mark.parametrize("name,kw", [("box-3to8", dict(kind="box")), ("gauss-2to12", dict(kind="gaussian", fwhm=1.5))])
def test_measure_gradient_and_double_gradient(name, kw):
    prof = CS.SliceProfile(*((3, 8) if name == "box-3to8" else (2, 12)), **kw)
    got = _autograd_case(prof, torch.float32, DEV, einsum=False)
    ref = _autograd_case(prof, torch.float64, "cpu", einsum=True)
    t32 = _autograd_case(prof, torch.float32, DEV, einsum=True)
    print(f"\n[measure autograd {name}]")
    for tag, k, r, t in zip(("forward", "gradient", "double gradient"), got, ref, t32):
        assert float(r.abs().max()) > 0
        check_2x(tag, k.cpu(), r, t.cpu())


def _vae_oracle(sd, x, W, autocast):
    sdg = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    ctx = torch.autocast("cpu", dtype=torch.bfloat16) if autocast else contextlib.nullcontext()
    with ctx:
        recon = R.vae_decode(sdg, R.vae_encode(sdg, x, 0.5), 0.5)
    recon = recon.float()
    m = lambda v: torch.einsum("kj,ncjhw->nckhw", W, v)
    loss = F.mse_loss(recon, x) + 0.5 * F.mse_loss(m(recon), m(x))
    loss.backward()
    return loss.item(), {k: v.grad.detach().float() for k, v in sdg.items()}


def test_vae_training_step_with_a_measurement_term(pkg):
    """One VAE training step with mse + 0.5 mse(W recon, W x): the criterion of tests/test_gpu_vae_train.py -- per parameter
    err_hip <= 2 err_autocast + 2e-2 (rel-L2 against the fp32 oracle), loss within 2 %."""
    from tests.test_gpu_vae_train import _judge, _tiny
    from tests.test_oracle_vae_train_golden import SHAPE
    vae, sd = _tiny(pkg, 8, 50)
    try:
        x = formula_input(SHAPE, 41).clamp(-1, 1)
        prof = CS.SliceProfile(2, SHAPE[2])
        xd = x.to(DEV)
        recon, _ = vae(xd)
        loss = F.mse_loss(recon.float(), xd) + 0.5 * F.mse_loss(prof.measure(recon), prof.measure(xd))
        loss.backward()
        torch.cuda.synchronize()
        W = torch.from_numpy(prof.W).float()
        ref_loss, ref_g = _vae_oracle(sd, x, W, autocast=False)
        _, ac_g = _vae_oracle(sd, x, W, autocast=True)
        print(f"\nloss hip {loss.item():.6f} oracle {ref_loss:.6f}")
        assert abs(loss.item() - ref_loss) <= 2e-2 * ref_loss
        for name, p in vae.named_parameters():
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, name
        _judge(vae, ref_g, ac_g, "measure-term")
        # the term contributes: the gradients differ from those of the plain MSE
        g_with = vae.decoder.conv_out.weight.grad.clone()
        vae.zero_grad(set_to_none=True)
        recon, _ = vae(xd)
        F.mse_loss(recon.float(), xd).backward()
        assert rel_l2(g_with, vae.decoder.conv_out.weight.grad) > 1e-3
    finally:
        vae.invalidate_engine_cache()


def test_measurement_residual():
    prof = CS.SliceProfile(3, 8, kind="gaussian", fwhm=1.0)
    vol = torch.tanh(formula_input((2, 1, 8, 9, 11), 51))
    thick = (mv(torch.from_numpy(prof.W), vol.double()) + 0.05 * formula_noise(5, (2, 1, 3, 9, 11)).double()).float()
    got = MT.measurement_residual(vol.to(DEV), thick.to(DEV), prof)
    d = mv(torch.from_numpy(prof.W), vol.double()) - thick.double()
    rmse = d.pow(2).mean(dim=(0, 1, 3, 4)).sqrt()
    psnr = 20.0 * torch.log10(2.0 / rmse)
    print("\nrmse", got["rmse"], "psnr", got["psnr"])
    assert len(got["rmse"]) == len(got["psnr"]) == 3
    # W vol in fp32: an error of a few 1e-7 on differences of about 0.05 -- 1e-5 relative on the RMSE, 1e-4 dB on the PSNR
    for k in range(3):
        assert abs(got["rmse"][k] - float(rmse[k])) <= 1e-5 * float(rmse[k])
        assert abs(got["psnr"][k] - float(psnr[k])) <= 1e-4
    exact = MT.measurement_residual(vol.to(DEV), prof.measure(vol.to(DEV)), prof)
    assert exact["rmse"] == [0.0] * 3 and all(p == float("inf") for p in exact["psnr"])
    from utils.metrics import measurement_residual
    assert measurement_residual is MT.measurement_residual
    with pytest.raises(ValueError, match="expected"):
        MT.measurement_residual(vol.to(DEV), thick[:, :, :2].to(DEV), prof)


def test_sharded_generation_is_refused(tiny):
    v_in = formula_input((1, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    tiny.data_consistency = CS.DataConsistency()
    tiny.unet.depth_shard_comm = object()
    try:
        with recorded_calls() as calls:
            with pytest.raises(L.CtsiError, match="depth sharding"):
                tiny.generate(v_in, "ddim", num_inference_steps=2, target_depth=4, noise_fn=formula_noise)
        assert calls == []
    finally:
        del tiny.unet.depth_shard_comm
        tiny.data_consistency = None
