"""CPU: autograd through the oracle's VAE (oracle.ref_ops.vae_encode / vae_decode) reproduces the reference's own VAE
training gradients (tests/golden/vae_train_v1.npz, made by tests/golden/make_golden_vae_train.py from the reference's
VideoVAE): the loss, the SSIM-augmented total of its AutoencoderLoss, z and the gradient of every parameter.  This pins the
oracle that the GPU tests of tests/test_gpu_vae_train.py compare the engine with."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R
from tests.grad_sketch import grad_sketch
from tests.helpers import rel_l2

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_train_v1.npz")
CONFIGS = {"l8": (8, 50), "l16": (16, 51)}
SHAPE = (2, 1, 4, 32, 32)


def vae_param_shapes(pkg, latent):
    vae = pkg.VideoVAE(in_channels=1, latent_dim=latent, base_channels=16, scaling_factor=0.5)
    return {k: tuple(v.shape) for k, v in vae.state_dict().items()}


def sketch_errors(gold, tag, grads):
    """rel-L2 of each parameter gradient's sketch (grads: name -> tensor, in named_parameters() order) against the golden one"""
    return {name: rel_l2(grad_sketch(g, i), gold[f"{tag}.grad.{name}"]) for i, (name, g) in enumerate(grads.items())}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_oracle_autograd_reproduces_reference_vae_gradients(gold, pkg, tag):
    latent, seed = CONFIGS[tag]
    shapes = vae_param_shapes(pkg, latent)
    sd = {k: v.clone().requires_grad_(True) for k, v in R.formula_state_dict(shapes, seed).items()}
    x = torch.from_numpy(gold["x"])
    assert torch.equal(x, R.formula_input(SHAPE, 41).clamp(-1, 1))
    z = R.vae_encode(sd, x, 0.5)
    recon = R.vae_decode(sd, z, 0.5)
    loss = F.mse_loss(recon, x)
    loss.backward()
    assert abs(loss.item() - float(gold[f"{tag}.loss_mse"])) <= 1e-5 * float(gold[f"{tag}.loss_mse"])
    assert rel_l2(z.detach(), gold[f"{tag}.z"]) < 1e-5
    # the SSIM term is a constant: the total differs from the MSE by exactly 0.1 * (1 - ssim)
    tot = float(gold[f"{tag}.loss_total"])
    assert abs(tot - (float(gold[f"{tag}.loss_mse"]) + 0.1 * (1 - float(gold[f"{tag}.ssim"])))) < 1e-9
    assert len(shapes) == sum(1 for k in gold.files if k.startswith(f"{tag}.grad."))
    errs = sketch_errors(gold, tag, {name: sd[name].grad for name in shapes})
    worst = max(errs.items(), key=lambda kv: kv[1])
    assert worst[1] < 1e-4, worst
