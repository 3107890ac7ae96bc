"""Golden-vector generator for VAE training (the backward of VideoVAE.forward) -- runs ONLY where the reference is present.

Runs the reference's own VideoVAE with formula weights (as make_golden.py does) on a fixed (2,1,4,32,32) batch, forms the
reference's autoencoder loss -- F.mse_loss(recon, x), and the total that its AutoencoderLoss builds with the mid-slice SSIM
term switched on (lambda_recon 1.0, lambda_ssim 0.1, the SSIM from utils.metrics.calculate_ssim: a Python float) -- and
stores the loss values and the gradient of every parameter after mse.backward() in tests/golden/vae_train_v1.npz.
Gradients are stored as their tests/grad_sketch.py fingerprints (small tensors whole, large ones as fixed projections + norm).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vae_train.py <root of the reference checkout>
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = os.path.abspath(sys.argv[1])
sys.dont_write_bytecode = True
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
sys.path.insert(0, REF)

spec = importlib.util.spec_from_file_location("ref_ops", os.path.join(REPO, "oracle", "ref_ops.py"))
R = importlib.util.module_from_spec(spec)
spec.loader.exec_module(R)
spec = importlib.util.spec_from_file_location("grad_sketch", os.path.join(REPO, "tests", "grad_sketch.py"))
S = importlib.util.module_from_spec(spec)
spec.loader.exec_module(S)

import models.vae as ref_vae                # noqa: E402
import utils.metrics as ref_metrics         # noqa: E402

assert ref_vae.__file__.startswith(REF), ref_vae.__file__
torch.set_num_threads(8)

SHAPE, INPUT_KEY, LAMBDA_SSIM = (2, 1, 4, 32, 32), 41, 0.1
CONFIGS = {"l8": dict(latent_dim=8, seed=50), "l16": dict(latent_dim=16, seed=51)}
out = {"x": R.formula_input(SHAPE, INPUT_KEY).clamp(-1, 1).numpy()}
for tag, cfg in CONFIGS.items():
    vae = ref_vae.VideoVAE(in_channels=1, latent_dim=cfg["latent_dim"], base_channels=16, scaling_factor=0.5)
    shapes = {k: tuple(v.shape) for k, v in vae.state_dict().items()}
    vae.load_state_dict(R.formula_state_dict(shapes, cfg["seed"]), strict=True)
    vae.train()
    x = torch.from_numpy(out["x"])
    recon, z = vae(x)
    mse = F.mse_loss(recon.float(), x.float())
    mid = SHAPE[2] // 2
    ssim = ref_metrics.calculate_ssim((recon[:, :, mid].detach().float() + 1) / 2, (x[:, :, mid].float() + 1) / 2,
                                      max_val=1.0)
    ssim = float(ssim)
    out[f"{tag}.loss_mse"] = np.float64(mse.item())
    out[f"{tag}.ssim"] = np.float64(ssim)
    out[f"{tag}.loss_total"] = np.float64(mse.item() + LAMBDA_SSIM * (1.0 - ssim))
    out[f"{tag}.z"] = z.detach().numpy()
    mse.backward()
    for i, (name, p) in enumerate(vae.named_parameters()):
        out[f"{tag}.grad.{name}"] = S.grad_sketch(p.grad, i).numpy()
    print(tag, "mse", mse.item(), "ssim", ssim, "params", len(list(vae.parameters())))

np.savez(os.path.join(REPO, "tests", "golden", "vae_train_v1.npz"), **out)
print("wrote", len(out), "arrays")
