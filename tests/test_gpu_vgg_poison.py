"""GPU: the VGG perceptual loss under the poison-and-guard harness (tests/poison.py), as tests/test_gpu_poison.py runs the
other paths: the first end-to-end case again with every torch.empty / zeros buffer of the engine inside guard bands and
pre-filled with 0x00, 0xFF (NaN) and 0x7F (3.4e38).  Loss, layer means and grad_pred must not change by a bit, no guard byte
may change, a second evaluation on refilled scratch must give the same bits, and so must a run in which no activation buffer is
reused."""
import importlib

import pytest
import torch

from tests import poison as PZ
from tests.test_gpu_vgg_loss import CASES, _inputs
from tests.vgg_restatement import he_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, BIG = 0xFF, 0x7F


@pytest.mark.parametrize("tag", ["2x10x32x48_rate0.2", "2x10x32x48_mse"])
def test_loss_forward_and_backward_poisoned(tag):
    case = CASES[tag]
    losses = importlib.import_module("models.losses")
    m = losses.VGGPerceptualLoss(list(case["layers"]), case["use_l1"], case["rate"], weights=he_state_dict(1234, upto=30)).to(DEV)
    pred, target = _inputs(case["shape"])

    def f():
        p = pred.detach().clone().requires_grad_(True)
        loss = m(p, target)
        loss.backward()
        torch.cuda.synchronize()
        return {"loss": loss.detach(), "means": m.last_layer_means, "grad": p.grad}

    ref = PZ.run_scenario(f, name=f"vgg-loss[{tag}]", modules=[m], ragged=True, inside=PZ.reevaluate(f),
                          no_reuse_fills=(NAN, BIG))
    assert torch.isfinite(ref["loss"]) and float(ref["loss"]) > 0.0 and torch.isfinite(ref["grad"]).all()
    for name in ("maxpool2_fwd", "maxpool2_bwd", "feat_loss", "feat_loss_finalize", "feat_grad_relu_bwd"):
        assert f"vgg-loss[{tag}]" in PZ.COVERAGE.get(name, set()), name
    importlib.import_module("video-to-video-diffusion_amd.engine").invalidate_engine_cache(m)
