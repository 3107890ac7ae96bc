"""GPU: the bf16x3 inference mode under the poison-and-guard harness (tests/poison.py), as tests/test_gpu_poison.py runs the
bf16 and fp32 modes: every torch.empty buffer of the engine inside guard bands and pre-filled with 0x00, 0xFF (NaN) and 0x7F
(3.4e38).  Results must not change by a bit, no guard byte may change, a second evaluation on refilled scratch must give the same
bits, and so must a run in which no activation buffer is reused.  Odd shapes: ragged row tiles in every conv geometry."""
import pytest
import torch

from tests import poison as PZ
from tests.helpers import formula_input, formula_noise, tiny_model_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, BIG = 0xFF, 0x7F


def _noise_fn(i, shape):
    return formula_noise(i, shape).to(DEV)


@pytest.fixture(scope="module")
def tiny(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    yield model
    model.invalidate_engine_cache()


def _assert_covered(scenario, suffixes):
    """The scenario's guarded programs launched the bf16x3 kernel in its plain, strided (d) and transposed (t) geometry."""
    for sfx in suffixes:
        hit = [k for k, names in PZ.COVERAGE.items() if k.startswith("conv_bf16x3_mfma_128x") and scenario in names
               and (k[-1] == sfx if sfx else k[-1].isdigit())]
        assert hit, (scenario, sfx, sorted(k for k in PZ.COVERAGE if k.startswith("conv_")))


def test_tiny_generate_bf16x3_odd_volume(tiny):
    """encode -> depth upsample -> DDIM -> decode on (1,1,3,24,40) -> 5 slices with every conv on conv_bf16x3_kernel."""
    v_in = formula_input((1, 1, 3, 24, 40), 16).clamp(-1, 1).to(DEV)

    def f():
        out = tiny.generate(v_in, "ddim", num_inference_steps=3, target_depth=5, noise_fn=_noise_fn, precision="bf16x3")
        torch.cuda.synchronize()
        return out

    out = PZ.run_scenario(f, name="tiny-generate[bf16x3]", modules=[tiny], ragged=True, inside=PZ.reevaluate(f),
                          no_reuse_fills=(NAN, BIG))
    assert bool(torch.isfinite(out).all())
    _assert_covered("tiny-generate[bf16x3]", ("", "d", "t"))


def test_tiny_vae_encode_decode_bf16x3_odd_volume(tiny):
    v = formula_input((2, 1, 3, 20, 28), 18).clamp(-1, 1).to(DEV)

    def f():
        tiny.vae.inference_precision = "bf16x3"
        try:
            z = tiny.vae.encode(v)
            out = tiny.vae.decode(z)
        finally:
            tiny.vae.inference_precision = "bf16"
        torch.cuda.synchronize()
        return {"z": z, "out": out}

    res = PZ.run_scenario(f, name="tiny-vae[bf16x3]", modules=[tiny], ragged=True, inside=PZ.reevaluate(f),
                          no_reuse_fills=(NAN, BIG))
    assert bool(torch.isfinite(res["z"]).all()) and bool(torch.isfinite(res["out"]).all())
    _assert_covered("tiny-vae[bf16x3]", ("", "d", "t"))
