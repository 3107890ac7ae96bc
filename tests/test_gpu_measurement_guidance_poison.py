"""GPU: measurement guidance under the poison-and-guard harness (tests/poison.py; DESIGN sections 16 and 31): a guided tiny
generate() and the three kernels of csrc/measure_guide.hip on their own are bit-identical whatever byte their buffers held
before -- the saved state, the latent the decoder reads, g_x, the partial slots and the per-sample sums included: every slot is
written by exactly one block, none is accumulated into -- with every guard band intact, again after the programs' scratch was
refilled, and with buffer reuse switched off."""
import importlib

import pytest
import torch

from tests import poison as PZ
from tests.helpers import formula_input, formula_noise, tiny_model_sd
from tests.test_gpu_measurement_guidance_ops import launch_apply, launch_residual_adj, launch_z0, to_ndhwc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = 0xFF
MG = importlib.import_module("video-to-video-diffusion_amd.measurement_guidance")
CS = importlib.import_module("video-to-video-diffusion_amd.consistency")


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_guided_generate(pkg, sampler):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    mg = MG.MeasurementGuidance(scale=1.0, start=0.0)
    model.measurement_guidance = mg
    v_in = formula_input((2, 1, 3, 8, 24), 21).clamp(-1, 1).to(DEV)          # latents (2, 8, 8, 2, 6): planes the U-Net halves

    def f():
        out = model.generate(v_in, sampler, num_inference_steps=3, target_depth=8, noise_fn=formula_noise, guidance_scale=3.0)
        torch.cuda.synchronize()
        return dict(out=out, stats=mg.last_stats)

    try:
        ref = PZ.run_scenario(f, name=f"generate-measurement-guidance[{sampler}]", modules=[model], ragged=True,
                              inside=PZ.reevaluate(f), no_reuse_fills=(NAN,))
    finally:
        model.measurement_guidance = None
        model.invalidate_engine_cache()
    assert torch.isfinite(ref["out"]).all() and torch.isfinite(ref["stats"]).all()
    assert ref["stats"].shape == (4, 2) and bool((ref["stats"] > 0).all())


@pytest.mark.parametrize("shape,depths,kw", [((3, 1, 1, 37), (2, 6), dict(kind="box")),
                                             ((2, 3, 4, 67), (3, 8), dict(kind="gaussian", fwhm=1.0)),
                                             ((1, 1, 8, 12), (50, 300), dict(kind="box"))],
                         ids=["scalar-2to6", "ragged-vec-3to8", "deep-50to300"])
def test_bare_residual_adj(shape, depths, kw):
    n, c, h, w = shape
    d_in, d_out = depths
    prof = CS.SliceProfile(d_in, d_out, **kw)
    x0 = torch.tanh(formula_input((n, c, d_out, h, w), 71)).to(DEV)
    y = (0.8 * torch.tanh(formula_input((n, c, d_in, h, w), 72))).to(DEV)

    def f():
        x = torch.empty_like(x0)          # a guarded buffer: the kernel must not write its input
        x.copy_(x0)
        g, sumsq, partials = launch_residual_adj(prof, x, y)
        return dict(g=g, sumsq=sumsq, partials=partials, x=x)

    ref = PZ.run_scenario(f, name=f"residual_adj[{d_in}to{d_out}]", ragged=True, expect_programs=False, inside=PZ.reevaluate(f),
                          no_reuse_fills=(NAN,))
    assert torch.isfinite(ref["g"]).all() and bool((ref["sumsq"] > 0).all()) and torch.equal(ref["x"], x0.cpu())


@pytest.mark.parametrize("shape", [(2, 8, 8, 3, 5), (2, 3, 2, 3, 5)], ids=["vec", "scalar"])
def test_bare_z0_and_apply(shape):
    n, c, d, h, w = shape
    z, eps = to_ndhwc(formula_input(shape, 81)).to(DEV), to_ndhwc(formula_input(shape, 82)).to(DEV)
    g = (0.3 * formula_input(shape, 93)).to(DEV)
    sumsq0 = torch.tensor([198.81, 0.0], dtype=torch.float64, device=DEV)
    zin0 = formula_input((n, d, h, w, 2 * c), 94).to(torch.bfloat16).to(DEV)

    def f():
        z0 = launch_z0(z, eps, 0.3, 0.95, 0, 1.0, shape)
        z_nd, hist, zin, sumsq = torch.empty_like(z), torch.empty_like(z), torch.empty_like(zin0), torch.empty_like(sumsq0)
        z_nd.copy_(z), hist.copy_(eps), zin.copy_(zin0), sumsq.copy_(sumsq0)
        launch_apply(z_nd, hist, g, sumsq, -1.5, -2.0, 1, zin, 2 * c, shape)
        return dict(z0=z0, z=z_nd, hist=hist, zin=zin)

    ref = PZ.run_scenario(f, name=f"guide_z0+apply{shape}", ragged=True, expect_programs=False, inside=PZ.reevaluate(f),
                          no_reuse_fills=(NAN,))
    assert all(torch.isfinite(v.float()).all() for v in ref.values())
