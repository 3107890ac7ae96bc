"""GPU: the image-loss path under the poison-and-guard harness (tests/poison.py; DESIGN sections 16 and 27), as
tests/test_gpu_window_fuse_poison.py runs latent window fusion: results bit-identical whatever byte the buffers held before,
every guard band intact, again after the programs' scratch was refilled, and with buffer reuse switched off.  The scenarios
build the U-Net training program with its predicted-latent output and the data-gradient decode program, so ctsi_z0_pred,
ctsi_loss_bwd_z0 and the decoder's backward tape run poisoned."""
import pytest
import torch

from tests import poison as PZ
from tests.helpers import formula_input, load_formula, tiny_model_sd
from tests.test_gpu_image_loss import T_FIX, _l1_half, inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = 0xFF


def test_end_to_end_step(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    model.image_loss = _l1_half
    v_in, v_gt, noise = (x.to(DEV) for x in inputs())

    def f():
        for p in model.parameters():
            p.grad = None
        total, metrics = model(v_in, v_gt, t=T_FIX.to(DEV), noise=noise)
        total.backward()
        torch.cuda.synchronize()
        assert metrics["image_rows"] == 1
        return dict(total=total.detach().clone(), grads=[p.grad.clone() for p in model.unet.parameters()])

    try:
        PZ.run_scenario(f, name="image-loss-step", modules=[model], ragged=True, inside=PZ.reevaluate(f), no_reuse_fills=(NAN,))
    finally:
        model.invalidate_engine_cache()
    assert {"loss.fwd", "loss.bwd", "seam.grad_z", "head.grad"} <= set(PZ.COVERAGE), sorted(PZ.COVERAGE)


def test_decode_with_grad(pkg):
    vae = pkg.VideoVAE(in_channels=1, latent_dim=8, base_channels=16, scaling_factor=0.5)
    load_formula(vae, 50)
    vae.to(DEV)
    z = formula_input((2, 8, 3, 5, 6), 61).to(DEV)
    target = formula_input((2, 1, 3, 20, 24), 62).clamp(-1, 1).to(DEV)

    def f():
        zd = z.clone().requires_grad_(True)
        recon = vae.decode_with_grad(zd)
        (recon - target).pow(2).mean().backward()
        torch.cuda.synchronize()
        return dict(recon=recon.detach().clone(), grad_z=zd.grad.clone())

    try:
        PZ.run_scenario(f, name="decode-with-grad", modules=[vae], ragged=True, inside=PZ.reevaluate(f), no_reuse_fills=(NAN,))
    finally:
        vae.invalidate_engine_cache()
    assert "decode-with-grad" in PZ.COVERAGE.get("seam.grad_z", ())
