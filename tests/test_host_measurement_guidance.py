"""CPU: the host side of measurement guidance (video-to-video-diffusion_amd/measurement_guidance.py) --
argument validation, which evaluations are guided, kappa per sampler against a float64 restatement on both schedules, the z0
rows, the config section, the plain attribute, and every refusal that needs no device."""
import importlib
import inspect
import logging
import math

import numpy as np
import pytest
import torch

from tests import measurement_guidance_restatement as MR
from tests.helpers import TINY_CFG, TINY_UNET

MG = importlib.import_module("video-to-video-diffusion_amd.measurement_guidance")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")


def test_argument_validation():
    g = MG.MeasurementGuidance()
    assert (g.kind, g.fwhm, g.scale, g.start, g.every, g.normalize) == ("box", None, 1.0, 0.5, 1, "residual")
    assert g.last_stats is None and g.profile(2, 12) is g.profile(2, 12) and g.profile(2, 12).W.shape == (2, 12)
    g = MG.MeasurementGuidance(kind="gaussian", fwhm=1.5, scale=0, start=1, every=3, normalize="none")
    assert (g.fwhm, g.scale, g.start, g.every, g.normalize) == (1.5, 0.0, 1.0, 3, "none")
    M = np.zeros((2, 6))
    M[0, :4], M[1, 2:] = 2.0, 1.0
    assert MG.MeasurementGuidance(matrix=M).profile(2, 6).kind == "matrix"
    for kw in (dict(kind="nope"), dict(kind="gaussian"), dict(kind="box", fwhm=1.0), dict(kind="gaussian", fwhm=-1.0),
               dict(scale=-0.5), dict(scale=float("inf")), dict(scale=float("nan")), dict(scale=True), dict(scale="1"),
               dict(start=-0.1), dict(start=1.5), dict(start=float("nan")), dict(start=True), dict(start=None),
               dict(every=0), dict(every=1.5), dict(every=True), dict(normalize="l2"), dict(normalize=None)):
        with pytest.raises(ValueError):
            MG.MeasurementGuidance(**kw)
    with pytest.raises(ValueError, match="nothing to project"):
        MG.MeasurementGuidance().profile(4, 4)
    with pytest.raises(L.CtsiError, match="d_in=65"):
        MG.MeasurementGuidance().profile(65, 130)


def test_guided_evaluations():
    for E in (1, 2, 3, 4, 7, 21, 51, 1000):
        for start in (0.0, 0.25, 0.5, 0.9, 1.0):
            for every in (1, 2, 5, 50):
                got = MG.MeasurementGuidance(start=start, every=every).guided_evaluations(E)
                assert got == MR.guided_evaluations(E, 1.0, start, every), (E, start, every)
                assert got[-1] == E - 1 and list(got) == sorted(set(got)) and got[0] >= math.ceil(start * (E - 1))
                assert all(b - a == every for a, b in zip(got, got[1:]))
                assert got[0] - every < math.ceil(start * (E - 1))          # no eligible evaluation is left out in front
                assert MG.MeasurementGuidance(scale=0.0, start=start, every=every).guided_evaluations(E) == ()
        assert MG.MeasurementGuidance(start=1.0).guided_evaluations(E) == (E - 1,)
        assert MG.MeasurementGuidance(start=0.0).guided_evaluations(E) == tuple(range(E))
    assert MG.MeasurementGuidance().guided_evaluations(51) == tuple(range(25, 51))
    assert MG.MeasurementGuidance(every=5).guided_evaluations(51) == (25, 30, 35, 40, 45, 50)
    assert MG.MeasurementGuidance(start=0.5, every=4).guided_evaluations(4) == (3,) and \
        MG.MeasurementGuidance(start=0.5, every=4).guided_evaluations(8) == (7,)
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            MG.MeasurementGuidance().guided_evaluations(bad)


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_kappa_rows(pkg, schedule):
    df = pkg.GaussianDiffusion(schedule, 1000)
    ac = df.alphas_cumprod.double().numpy()
    ddim_t = [int(t) for t in S.DDIMSampler(df, None)._get_timesteps(10)]
    for kind, t_desc in (("ddim", ddim_t), ("ddim", [999, 500, 0]), ("ddpm", list(range(999, 989, -1))), ("ddpm", [3, 2, 1, 0]),
                         ("dpmpp", ddim_t), ("dpmpp", [999, 666, 333, 0])):
        got, want = MG.kappa_rows(df, kind, t_desc), MR.kappa(ac, kind, t_desc, df.betas.double().numpy())
        assert got.dtype == np.float64 and got.shape == (len(t_desc),)
        # float64 on both sides from the same fp32 schedule.  'ddpm' reads the registered fp32 buffer posterior_mean_coef1, what
        # the update's own row holds: a product, a square root, a quotient and the stored value, each rounded to fp32 -- at most
        # 4 x 2^-24 = 2.4e-7 from the float64 value of the same expression
        tol = 2.5e-7 if kind == "ddpm" else 1e-12
        rel = np.abs(got - want) / np.abs(want)
        print(f"{schedule} {kind} {len(t_desc)} steps: kappa {got[0]:.6g} .. {got[-1]:.6g}  max rel err {rel.max():.2e}")
        assert rel.max() <= tol, (kind, got, want)
    assert MG.kappa_rows(df, "ddim", ddim_t)[-1] == 1.0 and MG.kappa_rows(df, "dpmpp", ddim_t)[-1] == 1.0
    # the last ancestral step returns the data prediction: beta_0 / (1 - abar_0) = 1, up to the rounding of abar_0 = 1 - beta_0
    # to fp32 (half an ulp of 1, 3e-8, on beta_0 = 1e-4 .. 4e-5)
    assert abs(MG.kappa_rows(df, "ddpm", [0])[0] - 1.0) <= 1e-3
    # the update form does not enter
    dv = pkg.GaussianDiffusion(schedule, 1000, prediction_type="v_prediction")
    dv.update_form = "x0"
    for kind in ("ddim", "ddpm", "dpmpp"):
        assert np.array_equal(MG.kappa_rows(dv, kind, ddim_t), MG.kappa_rows(df, kind, ddim_t))
    # kappa is the data prediction's weight in the rows the update reads: b of the x0 rows, with eps held fixed for ddim
    from importlib import import_module
    X0 = import_module("video-to-video-diffusion_amd.x0_form")
    rows = X0.x0_coef_rows(dv, "dpmpp", ddim_t, dtype=torch.float64).numpy()
    assert np.abs(rows[:, 3] - MG.kappa_rows(df, "dpmpp", ddim_t)).max() <= 1e-15
    rows = X0.x0_coef_rows(dv, "ddim", ddim_t, dtype=torch.float64).numpy()      # z' = a z + b X, z = alpha X + sigma eps
    assert np.abs(rows[:, 2] * rows[:, 0] + rows[:, 3] - MG.kappa_rows(df, "ddim", ddim_t)).max() <= 1e-12
    with pytest.raises(L.CtsiError, match="heun"):
        MG.kappa_rows(df, "heun", ddim_t)


def test_z0_rows(pkg):
    """{alpha, sigma, mode, clip} come from the coefficient rows the update itself reads."""
    df = pkg.GaussianDiffusion("cosine", 1000)
    t = [999, 666, 333, 0]
    for kind, mode, clip in (("ddim", 0, 10.0), ("ddpm", 0, 1.0), ("dpmpp", 1, 10.0)):
        plan = S._step_plan(df, kind, t, 0.0, 2, None)
        rows, coef = MG.z0_rows(plan), plan.coef.numpy()
        assert rows.dtype == np.float32 and rows.shape == (4, 4)
        assert (rows[:, 2] == mode).all() and (rows[:, 3] == clip).all()
        if mode == 0:
            assert np.array_equal(rows[:, 0], coef[:, 1]) and np.array_equal(rows[:, 1], coef[:, 0])
        else:
            assert np.array_equal(rows[:, 0], coef[:, 0]) and np.array_equal(rows[:, 1], coef[:, 1])
    dv = pkg.GaussianDiffusion("cosine", 1000, prediction_type="v_prediction")
    dv.update_form = "x0"
    for kind, clip in (("ddim", 10.0), ("ddpm", 1.0), ("dpmpp", 10.0)):
        plan = S._step_plan(dv, kind, t, 0.0, 2, None)
        rows = MG.z0_rows(plan)
        assert plan.x0 and (rows[:, 2] == 1).all() and (rows[:, 3] == clip).all()
        assert np.array_equal(rows[:, :2], plan.coef.numpy()[:, :2])


def test_config_section(pkg):
    assert pkg.VideoToVideoDiffusion(TINY_CFG).measurement_guidance is None
    for sec in ({"enabled": False, "kind": "nope"}, {"enabled": "true", "kind": "nope"}, {"kind": "nope"}, "box"):
        assert pkg.VideoToVideoDiffusion(dict(TINY_CFG, measurement_guidance=sec)).measurement_guidance is None
    m = pkg.VideoToVideoDiffusion(dict(TINY_CFG, measurement_guidance={
        "enabled": True, "kind": "gaussian", "fwhm": 1.5, "scale": 2.0, "start": 0.25, "every": 5, "normalize": "none"}))
    g = m.measurement_guidance
    assert isinstance(g, MG.MeasurementGuidance)
    assert (g.kind, g.fwhm, g.scale, g.start, g.every, g.normalize) == ("gaussian", 1.5, 2.0, 0.25, 5, "none")
    g = pkg.VideoToVideoDiffusion(dict(TINY_CFG, measurement_guidance={"enabled": True})).measurement_guidance
    assert (g.kind, g.scale, g.start, g.every, g.normalize) == ("box", 1.0, 0.5, 1, "residual")
    for bad in ({"kind": "nope"}, {"kind": "gaussian"}, {"scale": -1}, {"start": 2}, {"every": 0}, {"normalize": "x"},
                {"fwhm": 2.0}, {"colour": "red"}, {"iterations": 2}):
        with pytest.raises(ValueError):
            pkg.VideoToVideoDiffusion(dict(TINY_CFG, measurement_guidance=dict(bad, enabled=True)))


def test_attribute_is_plain(pkg):
    model = pkg.VideoToVideoDiffusion(TINY_CFG)
    keys, mods = set(model.state_dict()), [n for n, _ in model.named_modules()]
    model.measurement_guidance = MG.MeasurementGuidance(scale=2.0)
    assert isinstance(model.measurement_guidance, MG.MeasurementGuidance)
    assert set(model.state_dict()) == keys and [n for n, _ in model.named_modules()] == mods
    assert not any("guidance" in k for k in keys) and "measurement_guidance" not in dict(model.named_children())
    model.measurement_guidance = None
    assert model.measurement_guidance is None
    CS = importlib.import_module("video-to-video-diffusion_amd.consistency")
    for bad in ("box", 1, lambda v, t: v, torch.nn.Identity(), CS.DataConsistency()):
        with pytest.raises(ValueError, match="measurement_guidance must be None or a MeasurementGuidance"):
            model.measurement_guidance = bad
    assert model.measurement_guidance is None
    # the samplers take the guidance per call (`measurement=`), never as an attribute; stitching does not take it at all
    g, un = pkg.GaussianDiffusion("cosine", 1000), pkg.UNet3D(**TINY_UNET)
    for sm in (S.DDIMSampler(g, un), S.DDPMSampler(g, un), S.DPMSolverSampler(g, un)):
        assert not hasattr(sm, "measurement_guidance")
        assert inspect.signature(sm.sample).parameters["measurement"].default is None
        assert "measurement" not in inspect.signature(sm.sample_with_stitching).parameters
    # run_sampler keeps its pinned parameter list: the bound measurement reaches it through sampler.measurement_scope
    assert "measurement" not in inspect.signature(S.run_sampler).parameters and callable(S.measurement_scope)
    assert "measurement" not in inspect.signature(S.HeunSampler.sample).parameters
    inf = importlib.import_module("inference.measurement_guidance")
    assert inf.MeasurementGuidance is MG.MeasurementGuidance and inf.kappa_rows is MG.kappa_rows


V_IN = torch.zeros(1, 1, 2, 16, 16)


def _refused(model, match, sampler="ddim", exc=None, **kw):
    with pytest.raises(exc or L.CtsiError, match=match) as info:
        model.generate(V_IN, sampler, num_inference_steps=2, **dict(dict(target_depth=4), **kw))
    if exc is None:       # every refusal names the feature and an alternative
        assert "measurement_guidance" in str(info.value) and ("; " in str(info.value) or ", or " in str(info.value))


def test_refusals_before_any_device_work(pkg):
    """On a CPU input: each of these is raised before generate() reaches its own 'move the input to a ROCm device'."""
    model = pkg.VideoToVideoDiffusion(TINY_CFG)
    model.measurement_guidance = MG.MeasurementGuidance()
    _refused(model, "'heun'", sampler="heun")
    _refused(model, "ddpm_spaced", sampler="ddpm_spaced")
    _refused(model, "fp32 inference precision", precision="fp32")
    _refused(model, "bf16x3 inference precision", precision="bf16x3")
    model.vae.inference_precision = "fp32"
    try:
        _refused(model, "fp32 inference precision")
    finally:
        model.vae.inference_precision = "bf16"
    for part in (model.unet, model.vae):
        part.depth_shard_comm = object()
        try:
            _refused(model, "depth sharding")
        finally:
            del part.depth_shard_comm
    _refused(model, "target_depth=1 is below the 2 input slices", exc=ValueError, target_depth=1)
    with pytest.raises(L.CtsiError, match="generate_ensemble does not support measurement_guidance"):
        model.generate_ensemble(V_IN, "ddim", num_inference_steps=2, num_members=2, target_depth=4)
    # scale 0 and None are "off": the call gets as far as the device check
    for off in (MG.MeasurementGuidance(scale=0.0), None):
        model.measurement_guidance = off
        with pytest.raises(L.CtsiError, match="move the input to a ROCm device"):
            model.generate(V_IN, "heun", num_inference_steps=2, target_depth=4)
        with pytest.raises(L.CtsiError, match="generate_ensemble runs on the HIP engine"):
            model.generate_ensemble(V_IN, "ddim", num_inference_steps=2, num_members=2, target_depth=4)
    # a learned reverse variance
    lv = pkg.VideoToVideoDiffusion(dict(TINY_CFG, unet_learn_sigma=True, var_type="learned_range"))
    lv.measurement_guidance = MG.MeasurementGuidance()
    _refused(lv, "learned reverse variance")
    _refused(lv, "learned reverse variance", sampler="ddpm")
    # a latent_dim the decoder's gradient tape does not take
    l4 = pkg.VideoToVideoDiffusion(dict(TINY_CFG, latent_dim=4))
    l4.measurement_guidance = MG.MeasurementGuidance()
    _refused(l4, "latent_dim=4")


def test_run_sampler_refusals(pkg):
    """A direct caller of the samplers gets the same refusals, before anything is drawn or built."""
    model = pkg.VideoToVideoDiffusion(TINY_CFG)
    df, un, vae = model.diffusion, model.unet, model.vae
    bound = MG.MeasurementGuidance().bind(V_IN, vae)
    shape, cond = (1, 8, 4, 4, 4), torch.zeros(1, 8, 4, 4, 4)
    drawn = []

    def noise_fn(i, shp):
        drawn.append(i)
        return torch.zeros(shp)

    with pytest.raises(L.CtsiError, match="generic model"):
        S.DDIMSampler(df, lambda z, t, c: z).sample(shape, cond, 2, "cuda", progress=False, noise_fn=noise_fn,
                                                    measurement=bound)
    with pytest.raises(L.CtsiError, match="'ddpm_lv'"):
        S.DDPMSampler(df, un).sample(shape, cond, "cuda", progress=False, noise_fn=noise_fn, num_inference_steps=4,
                                     measurement=bound)
    with pytest.raises(L.CtsiError, match="'heun'"):
        rows = S.HeunSampler(df, un).coef_rows(3)
        with S.measurement_scope(bound):
            S.run_sampler(df, un, shape, cond, "cuda", kind="heun", t_desc=list(rows.t), progress=False, heun=rows,
                          noise_fn=noise_fn)
    assert S._take_measurement() is None          # the scope does not outlive the call
    un.inference_precision = "bf16x3"
    try:
        with pytest.raises(L.CtsiError, match="bf16x3 inference precision"):
            S.DPMSolverSampler(df, un).sample(shape, cond, 2, "cuda", progress=False, noise_fn=noise_fn, measurement=bound)
    finally:
        un.inference_precision = "bf16"
    un.depth_shard_comm = object()
    try:
        with pytest.raises(L.CtsiError, match="depth sharding"):
            S.DDIMSampler(df, un).sample(shape, cond, 2, "cuda", progress=False, noise_fn=noise_fn, measurement=bound)
    finally:
        del un.depth_shard_comm
    assert drawn == []


def test_unchanged_depth_warns_once_and_is_off(pkg, caplog):
    model = pkg.VideoToVideoDiffusion(TINY_CFG)
    model.measurement_guidance = MG.MeasurementGuidance()
    with caplog.at_level(logging.WARNING, logger="video-to-video-diffusion_amd.model"):
        for kw in (dict(), dict(target_depth=2), dict()):
            # the guidance is switched off for the call, which then gets as far as the device check
            with pytest.raises(L.CtsiError, match="move the input to a ROCm device"):
                model.generate(V_IN, "ddim", num_inference_steps=2, **kw)
    assert sum("measurement_guidance" in r.getMessage() for r in caplog.records) == 1
