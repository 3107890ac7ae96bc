"""GPU: every backward launch of the training programs against a float64 reference computed from that launch's own operands.

The end-to-end gradient tests (test_gpu_train.py, test_gpu_vae_train*.py, test_gpu_fullsize.py) compare parameter gradients with
the fp32 oracle under `err_hip <= 2 err_autocast + 2e-2`, and the unit tests (test_gpu_train_ops.py) run small shapes at rel-L2
<= 3e-3.  Neither can see one lost or doubled tile partial of a config-3 weight gradient (~1e-3 rel-L2).  Here each backward op
of a training program runs on its own, with copies of exactly the operands it read (tests/train_audit.py), so the bound can be
the arithmetic of the launch itself:

  fp32 outputs (weight / bias gradients, dgamma / dbeta, the batched pointwise-layer gradients, the VAE thin wgrad, the time
  embedding): rel-L2 <= 1e-4 and max |err| <= 1e-3 max |ref|.  bf16 operands make every product exact in fp32; what is left is
  fp32 accumulation (measured worst values are in profiles/train_bwd_audit.log).  The max-abs term catches a single wrong tile.
  bf16 outputs (data gradients, GroupNorm dx, depth sums, loss and head gradients): every element within one bf16 ulp of the
  float64 reference (+ 1e-5 rms(ref); GroupNorm dx also rstd |gamma| ulp(g), see train_audit.py), and rel-L2 <= 4e-3 against bf16(ref).
  grad.add: bit for bit bf16(fp32(a) + fp32(b)).

Every backward op must carry an audit record (or be on train_audit.SKIP with a reason), so a backward launch added later cannot go
unchecked.  The programs: the production U-Net at config 3 (what tools/profile_train.py builds), two small U-Nets that reach the
remaining branches (batch 1 + a mask + a 6x6 level; latent 4 padded to 8 channels, 3 levels, 8 heads, odd coarse planes) and the
VAE training program at the thin and thick patches of the VAE training config."""
import gc
import importlib

import pytest
import torch

from tests import train_audit as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E = importlib.import_module("video-to-video-diffusion_amd.engine")
T = importlib.import_module("video-to-video-diffusion_amd.train_engine")
V = importlib.import_module("video-to-video-diffusion_amd.vae_train_engine")


def _free():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _report(title, rows, missing):
    print()
    print(A.format_table(title, rows))
    bad = [r for r in rows if not r["ok"]]
    assert not missing, f"backward ops without an audit record: {sorted(set(missing))}"
    assert rows, "no backward op was audited"
    assert not bad, "%d audited outputs out of bounds, first: %s" % (len(bad), bad[:3])


def _audit_unet(pkg, unet_kw, n, d, h, w, mask=False, seed=0):
    torch.manual_seed(seed)
    un = pkg.UNet3D(**unet_kw).to(DEV)
    diff = pkg.GaussianDiffusion("cosine", 1000).to(DEV)
    L = un.latent_dim
    g = torch.Generator().manual_seed(seed + 1)
    shape = (n, L, d, h, w)
    z0, cond, noise = (torch.randn(shape, generator=g).to(DEV) for _ in range(3))
    t = torch.randint(0, 1000, (n,), generator=g).to(DEV)
    ac = diff.alphas_cumprod[t]
    snr = ac / (1 - ac + 1e-8)
    norm = (snr.clamp(max=5.0) / (snr + 1e-8)) / float(n * L * d * h * w)
    m = None
    if mask:
        m = (torch.rand((n, L, d), generator=g) > 0.3).float().to(DEV)
    ctx = E.Ctx.get(DEV)
    with ctx.scope():
        prog = T.UNetTrainProgram(ctx, un, n, d, h, w)
        prog.set_diffusion(diff)
        prog.run_forward(z0, cond, t, noise, norm, m)
        prog.gscale.fill_(1.0)
    rows, missing = A.audit_backward(prog, prog.n_fwd)
    del prog
    _free()
    return rows, missing


def test_unet_config3_backward_audit(pkg):
    """The production U-Net (UNet3D(latent_dim=8), default init, seed 0) at config 3: batch 4, latent 48^3."""
    rows, missing = _audit_unet(pkg, dict(latent_dim=8), 4, 48, 48, 48)
    _report("U-Net config 3 (4, 8, 48, 48, 48): backward ops against float64 from their own operands", rows, missing)


@pytest.mark.parametrize("case", ["b1_mask_6x6", "latent4_three_levels"])
def test_unet_small_backward_audit(pkg, case):
    if case == "b1_mask_6x6":      # batch 1, a loss mask, levels 24 -> 12 -> 6 with attention on both coarse levels
        kw = dict(latent_dim=8, model_channels=32, num_res_blocks=1, attention_levels=[1, 2], channel_mult=(1, 2, 4),
                  num_heads=4, time_embed_dim=64)
        rows, missing = _audit_unet(pkg, kw, 1, 5, 24, 24, mask=True, seed=3)
    else:                          # the shape family of test_training_loss_latent4_three_levels
        kw = dict(latent_dim=4, model_channels=32, num_res_blocks=2, attention_levels=[1, 2], channel_mult=(1, 2, 4),
                  num_heads=8, time_embed_dim=128)
        rows, missing = _audit_unet(pkg, kw, 3, 5, 12, 8, seed=9)
    _report(f"U-Net {case}: backward ops against float64 from their own operands", rows, missing)


@pytest.mark.parametrize("depth", [48, 8])
def test_vae_backward_audit(pkg, depth):
    """The VAE training program at the VAE training config's patches: base 128, latent 16, (1, 1, depth, 192, 192), with an
    output gradient on both the reconstruction and z (so the seam's grad_z launch is active)."""
    torch.manual_seed(0)
    sf = 1.0 if depth == 48 else 0.5
    vae = pkg.VideoVAE(in_channels=1, latent_dim=16, base_channels=128, scaling_factor=sf).train().to(DEV)
    g = torch.Generator().manual_seed(depth)
    x = (torch.rand((1, 1, depth, 192, 192), generator=g) * 2 - 1).to(DEV)
    ctx = E.Ctx.get(DEV)
    with ctx.scope():
        prog = V.VAETrainProgram(ctx, vae, 1, depth, 192, 192)
        prog.run_forward(x)
        prog.g_recon.copy_(torch.randn(tuple(prog.g_recon.shape), generator=g).to(DEV) * 1e-3)
        prog.g_z.copy_(torch.randn(tuple(prog.g_z.shape), generator=g).to(DEV) * 1e-3)
        prog.use_gz = True
    rows, missing = A.audit_backward(prog, prog.n_fwd)
    del prog
    _free()
    _report(f"VAE (1, 1, {depth}, 192, 192), base 128, latent 16: backward ops against float64", rows, missing)
