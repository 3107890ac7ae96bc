"""GPU: one VAE training step at the size of the reference's config/vae_training.yaml -- base 128, thin (1,1,48,192,192) and
thick (1,1,8,192,192) patches, latent 16 and 8 -- against the fp32 oracle's autograd evaluated on the device, under the
criterion of tests/test_gpu_vae_train.py (err_hip <= 2 * err_autocast + 2e-2 per parameter tensor, loss within 2 %).  The
oracle's ConvTranspose3d runs in its CONVT_AS_CONV form (MIOpen's fp32 ConvTranspose backward-data path takes minutes here)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R
from tests.helpers import formula_input, load_formula, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _oracle_grads(sd, x, autocast):
    sdg = {k: v.detach().to(DEV).clone().requires_grad_(True) for k, v in sd.items()}
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        recon = R.vae_decode(sdg, R.vae_encode(sdg, x, 1.0), 1.0)
    loss = F.mse_loss(recon.float(), x)
    loss.backward()
    out = {k: v.grad.detach().float() for k, v in sdg.items()}
    del sdg, recon
    return loss.item(), out


@pytest.mark.parametrize("latent,depth", [(16, 48), (16, 8), (8, 48), (8, 8)])
def test_vae_training_step_full_size(pkg, monkeypatch, latent, depth):
    monkeypatch.setattr(R, "CONVT_AS_CONV", True)
    vae = pkg.VideoVAE(in_channels=1, latent_dim=latent, base_channels=128, scaling_factor=1.0)
    sd = load_formula(vae, 60 + latent)
    vae.train().to(DEV)
    x = formula_input((1, 1, depth, 192, 192), 45).clamp(-1, 1).to(DEV)
    recon, _ = vae(x)
    loss = F.mse_loss(recon, x)
    loss.backward()
    torch.cuda.synchronize()
    hip = {k: p.grad.float() for k, p in vae.named_parameters()}
    sd = {k: v.to(DEV) for k, v in sd.items()}
    ref_loss, ref_g = _oracle_grads(sd, x, False)
    torch.cuda.empty_cache()
    _, ac_g = _oracle_grads(sd, x, True)
    print(f"[latent {latent}, depth {depth}] loss hip {loss.item():.6f} oracle {ref_loss:.6f}")
    assert abs(loss.item() - ref_loss) <= 2e-2 * ref_loss
    worst = []
    for name in hip:
        e_h, e_a = rel_l2(hip[name].cpu(), ref_g[name].cpu()), rel_l2(ac_g[name].cpu(), ref_g[name].cpu())
        worst.append((e_h / (2 * e_a + 2e-2), e_h, e_a, name))
    worst.sort(reverse=True)
    for w in worst[:6]:
        print(f"  {w[3]:45s} hip {w[1]:.3e}  autocast {w[2]:.3e}  ratio {w[0]:.2f}")
    for w in worst:
        assert w[1] <= 2 * w[2] + 2e-2, w
