"""GPU: VAE training through the drop-in API -- `recon, z = vae(x)` in grad mode -> a torch loss -> `backward()` -> `.grad` of
every VAE parameter (vae_train_engine.VAETrainProgram), as the reference's training/train_vae.py uses it.

Yardstick (as tests/test_gpu_train.py): gradients against the fp32 oracle's autograd (pinned to the reference by
tests/test_oracle_vae_train_golden.py), with the error held against the oracle's own under bf16 autocast:
   err_hip(param) <= 2 * err_autocast(param) + 2e-2   (rel-L2 per parameter tensor), loss within 2 %.
"""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R
from tests.helpers import formula_input, load_formula, rel_l2
from tests.test_oracle_vae_train_golden import CONFIGS, GOLD, SHAPE, sketch_errors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAMBDA_SSIM = 0.1


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


def _tiny(pkg, latent, seed):
    vae = pkg.VideoVAE(in_channels=1, latent_dim=latent, base_channels=16, scaling_factor=0.5)
    sd = load_formula(vae, seed)
    vae.train()
    return vae.to(DEV), sd


def _oracle(sd, x, *, autocast=None, z_weight=0.0, dev="cpu"):
    """fp32 (or autocast bf16) oracle loss = mse(recon, x) [+ z_weight * mean(z^2)] and its parameter gradients."""
    sdg = {k: v.detach().to(dev).clone().requires_grad_(True) for k, v in sd.items()}
    x = x.to(dev)
    if autocast:
        with torch.autocast(dev.split(":")[0], dtype=torch.bfloat16):
            z = R.vae_encode(sdg, x, 0.5)
            recon = R.vae_decode(sdg, z, 0.5)
    else:
        z = R.vae_encode(sdg, x, 0.5)
        recon = R.vae_decode(sdg, z, 0.5)
    loss = F.mse_loss(recon.float(), x.float())
    if z_weight:
        loss = loss + z_weight * z.float().pow(2).mean()
    loss.backward()
    return loss.item(), {k: v.grad.detach().float().cpu() for k, v in sdg.items()}


def _judge(vae, ref_g, ac_g, tag, extra=None):
    worst = []
    for name, p in vae.named_parameters():
        g = p.grad.float().cpu()
        e_h, e_a = rel_l2(g, ref_g[name]), rel_l2(ac_g[name], ref_g[name])
        worst.append((e_h / (2 * e_a + 2e-2), e_h, e_a, name))
        if extra is not None:
            worst[-1] += (rel_l2(g, extra[name]),)
    worst.sort(reverse=True)
    for w in worst[:5]:
        print(f"  [{tag}] {w[3]:45s} hip {w[1]:.3e}  autocast {w[2]:.3e}  ratio {w[0]:.2f}")
    for w in worst:
        assert w[1] <= 2 * w[2] + 2e-2, w
    return worst


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_tiny_vae_gradients_vs_oracle_and_goldens(gold, pkg, tag):
    """recon, z = vae(x); MSE; backward: every gradient against the fp32 oracle and the reference goldens; z / recon
    bit for bit equal to encode / decode."""
    latent, seed = CONFIGS[tag]
    vae, sd = _tiny(pkg, latent, seed)
    x = torch.from_numpy(gold["x"]).to(DEV)
    recon, z = vae(x)
    assert recon.grad_fn is not None and z.grad_fn is not None
    loss = F.mse_loss(recon.float(), x.float())
    loss.backward()
    torch.cuda.synchronize()
    gl = float(gold[f"{tag}.loss_mse"])
    ref_loss, ref_g = _oracle(sd, x.cpu())
    _, ac_g = _oracle(sd, x.cpu(), autocast=True)
    print(f"[{tag}] loss hip {loss.item():.6f} reference {gl:.6f} oracle {ref_loss:.6f}")
    assert abs(loss.item() - gl) <= 2e-2 * gl
    # the fp32 oracle reproduces the reference's gradients (their golden sketches); the engine is judged against it
    assert max(sketch_errors(gold, tag, {name: ref_g[name] for name, _ in vae.named_parameters()}).values()) < 1e-4
    _judge(vae, ref_g, ac_g, tag)
    # forward equality with the inference legs, bit for bit
    with torch.no_grad():
        assert torch.equal(z.detach(), vae.encode(x))
        assert torch.equal(recon.detach(), vae.decode(z.detach()))
    assert x.grad is None


def test_grad_z_path(pkg):
    """A loss with a term on z as well: grad_z enters at the seam (scaled by scaling_factor) and reaches the encoder."""
    vae, sd = _tiny(pkg, 16, 51)
    x = formula_input(SHAPE, 41).clamp(-1, 1)
    recon, z = vae(x.to(DEV))
    loss = F.mse_loss(recon, x.to(DEV)) + 0.5 * z.pow(2).mean()
    loss.backward()
    ref_loss, ref_g = _oracle(sd, x, z_weight=0.5)
    _, ac_g = _oracle(sd, x, autocast=True, z_weight=0.5)
    assert abs(loss.item() - ref_loss) <= 2e-2 * ref_loss
    _judge(vae, ref_g, ac_g, "grad_z")
    # z alone: the decoder gets exactly zero, the encoder a gradient
    vae.zero_grad(set_to_none=True)
    _, z = vae(x.to(DEV))
    z.pow(2).mean().backward()
    assert float(vae.decoder.conv_out.weight.grad.abs().max()) == 0.0
    assert float(vae.encoder.conv_in.conv.weight.grad.abs().max()) > 0.0


def test_ssim_term_is_a_constant(gold, pkg):
    """The reference's AutoencoderLoss adds lambda_ssim * (1 - calculate_ssim(mid slice)): a float.  The loss matches the
    golden total, the gradients equal (bit for bit) those of the MSE-only loss."""
    from utils.metrics import calculate_ssim
    vae, _ = _tiny(pkg, 8, 50)
    x = torch.from_numpy(gold["x"]).to(DEV)
    recon, _ = vae(x)
    mse = F.mse_loss(recon.float(), x.float())
    mse.backward()
    g_mse = [p.grad.clone() for p in vae.parameters()]
    vae.zero_grad(set_to_none=True)
    recon, _ = vae(x)
    mid = x.shape[2] // 2
    ssim = calculate_ssim((recon[:, :, mid].detach() + 1) / 2, (x[:, :, mid] + 1) / 2, max_val=1.0)
    total = F.mse_loss(recon.float(), x.float()) + LAMBDA_SSIM * (1.0 - ssim)
    total.backward()
    gt = float(gold["l8.loss_total"])
    print(f"total hip {total.item():.6f} reference {gt:.6f} (ssim hip {float(ssim):.4f} reference {float(gold['l8.ssim']):.4f})")
    assert abs(total.item() - gt) <= 2e-2 * gt
    for a, p in zip(g_mse, vae.parameters()):
        assert torch.equal(a, p.grad)


def test_backward_is_deterministic(pkg):
    vae, _ = _tiny(pkg, 8, 50)
    x = formula_input(SHAPE, 41).clamp(-1, 1).to(DEV)
    grads = []
    for _ in range(2):
        vae.zero_grad(set_to_none=True)
        recon, z = vae(x)
        (F.mse_loss(recon, x) + 0.1 * z.abs().mean()).backward()
        grads.append([p.grad.clone() for p in vae.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


@pytest.mark.parametrize("fused", [False, True])
def test_optimizer_loop(pkg, fused):
    """Reference-style loop: AdamW / FusedAdamW lower the loss on a fixed batch (the engine picks the new weights up); two
    backward calls accumulate; a scaled loss scales the gradients; clip_grad_norm_ clips them; thick (8-slice) and thin
    batches alternate on their cached programs without a rebuild."""
    vae, _ = _tiny(pkg, 16, 51)
    params = list(vae.parameters())
    if fused:
        opt = pkg.FusedAdamW(params, lr=2e-3, weight_decay=0.0, engine_modules=[vae])
    else:
        opt = torch.optim.AdamW(params, lr=2e-3, weight_decay=0.0)
    thin = formula_input((1, 1, 8, 32, 32), 43).clamp(-1, 1).to(DEV)
    thick = formula_input((1, 1, 4, 32, 32), 44).clamp(-1, 1).to(DEV)
    losses, progs = [], {}
    for step in range(8):
        x = thick if step % 2 else thin
        opt.zero_grad(set_to_none=True)
        recon, _ = vae(x)
        loss = F.mse_loss(recon.float(), x.float())
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        if step % 2 == 0:
            losses.append(loss.item())
        cache = vae.__dict__["_ctsi_programs"]
        for key, prog in cache.items():
            if key[0] == "train":
                assert progs.setdefault(key, prog) is prog, "training program rebuilt"
    print("thin-batch losses:", ["%.5f" % v for v in losses])
    assert len(progs) == 2 and losses[-1] < losses[0]
    # accumulation and scaling
    opt.zero_grad(set_to_none=True)
    recon, _ = vae(thin)
    F.mse_loss(recon, thin).backward()
    g1 = [p.grad.clone() for p in params]
    recon, _ = vae(thin)
    (F.mse_loss(recon, thin) * 2.0).backward()      # (a power of two: the bf16 gradients scale exactly)
    for a, p in zip(g1, params):
        assert rel_l2(p.grad, 3.0 * a) <= 1e-5
    # GradScaler-style: scale, unscale, clip
    opt.zero_grad(set_to_none=True)
    recon, _ = vae(thin)
    (F.mse_loss(recon, thin) * 1024.0).backward()
    for a, p in zip(g1, params):
        p.grad.div_(1024.0)
        assert rel_l2(p.grad, a) <= 1e-5
    total = torch.nn.utils.clip_grad_norm_(params, 1e-3)
    norm = torch.norm(torch.stack([p.grad.norm() for p in params]))
    assert float(total) > 1e-3 and abs(float(norm) - 1e-3) <= 1e-5


def test_kernels_vs_torch(pkg):
    """Unit parity of the new kernels on ragged planes and channel paddings: the head gradient against autograd of tanh (and
    its add mode), the thin weight gradient against torch.nn.grad.conv3d_weight for cin = 1 and cout = 1."""
    import ctypes as C
    lib = pkg.get_lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    gen = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    # head gradient: n=2, c=3 (padded to 8), a 3 x 5 x 7 plane
    n, c, d, h, w = 2, 3, 3, 5, 7
    a = rnd(n, c, d, h, w).requires_grad_(True)
    y = torch.tanh(a)
    g = rnd(n, c, d, h, w)
    y.backward(g)
    dst = torch.full((n, d, h, w, 8), 7.0, dtype=torch.bfloat16, device=DEV)
    yd, gd = y.detach().to(DEV).contiguous(), g.to(DEV)
    lib.vae_head_grad(ptr(gd), ptr(yd), n, c, d, h, w, 2.0, 0, ptr(dst), 8, None)
    torch.cuda.synchronize()
    got = dst.float().cpu()
    assert rel_l2(got[..., :c].permute(0, 4, 1, 2, 3), 2.0 * a.grad) < 1e-2 and float(got[..., c:].abs().max()) == 0.0
    base = rnd(n, d, h, w, 8).to(torch.bfloat16)
    dst = base.to(DEV)
    lib.vae_head_grad(ptr(gd), None, n, c, d, h, w, 0.5, 1, ptr(dst), 8, None)
    torch.cuda.synchronize()
    got = dst.float().cpu()
    assert rel_l2(got[..., :c], base.float()[..., :c] + 0.5 * g.permute(0, 2, 3, 4, 1)) < 1e-2
    assert torch.equal(got[..., c:], base.float()[..., c:])
    # thin weight gradient, stem (cin = 1) and head (cout = 1), ragged planes; padded channels of the thin tensor hold junk
    for (n, cw, d, h, w) in ((2, 16, 3, 6, 10), (1, 32, 4, 9, 13), (1, 128, 2, 5, 36)):
        thin = rnd(n, d, h, w, 8).to(torch.bfloat16)
        wide = rnd(n, d, h, w, cw).to(torch.bfloat16)
        t_ncdhw = thin.float()[..., :1].permute(0, 4, 1, 2, 3)
        w_ncdhw = wide.float().permute(0, 4, 1, 2, 3)
        ws = torch.empty(lib.thin_wgrad_workspace_bytes(n, cw, d, h, w), dtype=torch.uint8, device=DEV)
        thin_d, wide_d = thin.to(DEV), wide.to(DEV)
        for head in (0, 1):
            dw = torch.full((cw * 27,), 5.0, device=DEV)
            lib.thin_wgrad(ptr(wide_d), cw, cw, ptr(thin_d), 8, head, n, d, h, w, 3, 3, 3, ptr(ws), ws.numel(), ptr(dw), 1.5,
                           None)
            torch.cuda.synchronize()
            if head:    # weight (1, cw, 3,3,3): input = wide, output gradient = thin
                ref = torch.nn.grad.conv3d_weight(w_ncdhw.double(), (1, cw, 3, 3, 3), t_ncdhw.double(), padding=1)
            else:       # weight (cw, 1, 3,3,3): input = thin, output gradient = wide
                ref = torch.nn.grad.conv3d_weight(t_ncdhw.double(), (cw, 1, 3, 3, 3), w_ncdhw.double(), padding=1)
            e = rel_l2(dw.cpu().double(), 1.5 * ref.reshape(-1))
            assert e < 1e-5, ((n, cw, d, h, w), head, e)


def test_errors(pkg):
    vae, _ = _tiny(pkg, 8, 50)
    with pytest.raises(pkg.CtsiError, match="multiples of 4"):
        vae(formula_input((1, 1, 3, 18, 22), 14).to(DEV))
    with torch.no_grad():                      # inference on the same shape still works
        vae(formula_input((1, 1, 3, 18, 22), 14).to(DEV))
    x = formula_input(SHAPE, 41).clamp(-1, 1).to(DEV)
    r1, _ = vae(x)
    r2, _ = vae(x * 0.5)
    with pytest.raises(pkg.CtsiError, match="overwritten"):
        F.mse_loss(r1, x).backward()
    F.mse_loss(r2, x).backward()              # the newest forward's backward is fine
