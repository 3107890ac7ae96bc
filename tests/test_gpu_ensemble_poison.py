"""GPU: ensemble statistics under the poison-and-guard harness (tests/poison.py; DESIGN sections 16 and 29): a bare accumulate /
finalize / calibration sequence at a ragged shape and generate_ensemble on the tiny model are bit-identical whatever byte their
buffers held before -- the running state (never read before the first member), the partial slots and the tables included:
every slot is written by exactly one block -- with every guard band intact, again on a second evaluation, and with buffer
reuse switched off."""
import importlib

import pytest
import torch

from tests import poison as PZ
from tests.helpers import formula_input, formula_noise, tiny_model_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = 0xFF
EN = importlib.import_module("video-to-video-diffusion_amd.ensemble")
MT = importlib.import_module("video-to-video-diffusion_amd.metrics")


@pytest.mark.parametrize("shape", [(2, 1, 3, 5, 7), (1, 1, 2, 65, 67), (1, 2, 2, 16, 16)],
                         ids=["ragged-5x7", "two-slots-65x67", "vec-16x16"])
def test_bare_statistics(shape):
    src = torch.tanh(formula_input((5,) + shape, 81)).to(DEV)
    target = torch.tanh(formula_input(shape, 82)).to(DEV)

    def f():
        x = torch.empty_like(src)          # guarded buffers: the kernels must stay inside them
        x.copy_(src)
        acc = EN.EnsembleAccumulator()
        acc.add(x[:2])
        acc.add(x[2])
        mid = acc.result()
        acc.add(x[3:])
        res = acc.result(unbiased=False)
        cal = MT.ensemble_calibration(res.mean, res.std, target)
        torch.cuda.synchronize()
        return dict(mean=res.mean, std=res.std, profile=res.slice_std, mid_mean=mid.mean, mid_std=mid.std,
                    mid_profile=mid.slice_std, rmse=cal["rmse"], rms_std=cal["rms_std"], c1=cal["coverage_1sigma"],
                    c2=cal["coverage_2sigma"], per_slice=cal["per_slice"]["rmse"])

    ref = PZ.run_scenario(f, name=f"ensemble-statistics{list(shape)}", ragged=True, expect_programs=False,
                          inside=PZ.reevaluate(f), no_reuse_fills=(NAN,))
    assert torch.isfinite(ref["mean"]).all() and torch.isfinite(ref["std"]).all() and float(ref["std"].max()) > 0.0
    assert torch.isfinite(ref["profile"]).all() and 0.0 < ref["c1"] <= ref["c2"] <= 1.0


def test_generate_ensemble(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    v_in = formula_input((1, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)

    def f():
        res = model.generate_ensemble(v_in, "ddim", num_inference_steps=3, num_members=3, member_batch=2, target_depth=4,
                                      member_noise_fn=lambda k, i, s: formula_noise(i + 50 * k, s), keep_members=True)
        torch.cuda.synchronize()
        return dict(mean=res.mean, std=res.std, profile=res.slice_std, members=res.members)

    try:
        ref = PZ.run_scenario(f, name="generate-ensemble", modules=[model], ragged=True, inside=PZ.reevaluate(f),
                              no_reuse_fills=(NAN,))
    finally:
        model.invalidate_engine_cache()
    assert torch.isfinite(ref["members"]).all() and torch.isfinite(ref["mean"]).all() and float(ref["std"].max()) > 0.0
