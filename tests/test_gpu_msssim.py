"""GPU: the differentiable MS-SSIM loss of models.losses (csrc/msssim.hip) -- forward and backward.

Yardsticks.  The truth is the float64 torch restatement (tests/msssim_restatement.py, pinned to the reference's class by
tests/test_oracle_msssim_golden.py); the yardstick is an fp32 evaluation of the same arithmetic -- the reference's own stored
result on the golden cases, the fp32 restatement on the device at real sizes -- never the engine's own output:
    |loss_hip - loss_64|      <= 2 |loss_32 - loss_64| + 2^-22
    relL2(grad_hip, grad_64)  <= 2 relL2(grad_32, grad_64) + 1e-6
The kernels evaluate the same fp32 formula (with the cancelling E[a^2] - mu^2) and differ only in summation order (separable
11 + 11 taps instead of 121, fp64 instead of fp32 means), so they should sit at the yardstick's own error; the factor 2 is this
suite's convention for "as good as the torch path", the additive terms a quarter-ulp-scale floor for a result of size <= 1,
because the yardstick can land on the truth by luck.
The five level means (an output for logs and tests; the issue sets no bar for them) are held to the same rule with the floor
    |mean_hip - mean_64|      <= 2 |mean_32 - mean_64| + 2^-24 / C2        (C2 = 9e-4: 6.6e-5)
one half-ulp rounding of a second moment of size <= 1 divided by the smallest value the denominator sigma1^2 + sigma2^2 + C2
can take.  Any fp32 evaluation stores E[a^2] and mu in fp32 before it subtracts, and on smooth inputs neighbouring pixels
round alike, so this part of the error is systematic and does not average out over the pixels of a level: the fp32
restatement itself lands anywhere between 1e-7 and 1e-6 depending on its summation order.  A wrong or swapped level is off
by 1e-3 or more.
The VAE cases use tests/test_gpu_vae_train.py's criterion unchanged (err_hip <= 2 err_autocast + 2e-2, loss within 2 %).
"""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R
from tests.helpers import formula_input, load_formula, rel_l2
from tests.msssim_restatement import msssim_loss, smooth_pair
from tests.test_gpu_vae_train import _judge, _tiny
from tests.test_oracle_msssim_golden import CASES, GOLD
from tests.test_oracle_vae_train_golden import CONFIGS, SHAPE
from tests.test_oracle_vae_train_golden import GOLD as VAE_GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_FLOOR, GRAD_FLOOR, MEAN_FLOOR = 2.0 ** -22, 1e-6, 2.0 ** -24 / 9e-4


@pytest.fixture(scope="module")
def losses():
    return importlib.import_module("models.losses")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


def _hip(losses, pred, target, channel=1):
    """loss, level means, grad of the device loss for fp32 device tensors"""
    m = losses.MS_SSIM_Loss(channel=channel)
    p = pred.detach().clone().requires_grad_(True)
    loss = m(p, target)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), m.last_level_means.double().cpu(), p.grad


def _restated(pred, target, dtype):
    p = pred.detach().clone().requires_grad_(True)
    loss, means = msssim_loss(p, target, dtype, return_means=True)
    loss.backward()
    return loss.detach().double().item(), means.detach().double().cpu(), p.grad.double()


def _report(tag, hip, y32, t64):
    """(loss, means, grad) triples of the engine, the fp32 yardstick and the fp64 truth: print, then assert the bars"""
    el_h, el_y = abs(float(hip[0]) - t64[0]), abs(y32[0] - t64[0])
    em_h, em_y = (hip[1] - t64[1]).abs().max().item(), (y32[1] - t64[1]).abs().max().item()
    eg_h, eg_y = rel_l2(hip[2].double().cpu(), t64[2].cpu()), rel_l2(y32[2].cpu(), t64[2].cpu())
    print(f"[{tag}] loss {t64[0]:.7f}  means {' '.join('%.4f' % v for v in t64[1])}")
    print(f"[{tag}]   loss err hip {el_h:.3e} fp32 {el_y:.3e} ratio {el_h / (2 * el_y + LOSS_FLOOR):.2f} | "
          f"means err hip {em_h:.3e} fp32 {em_y:.3e} | "
          f"grad relL2 hip {eg_h:.3e} fp32 {eg_y:.3e} ratio {eg_h / (2 * eg_y + GRAD_FLOOR):.2f}")
    assert el_h <= 2 * el_y + LOSS_FLOOR
    assert em_h <= 2 * em_y + MEAN_FLOOR
    assert eg_h <= 2 * eg_y + GRAD_FLOOR


@pytest.mark.parametrize("tag", CASES)
def test_golden_cases(losses, gold, tag):
    """The reference's own stored loss, level means and gradient are the fp32 yardstick; truth = fp64 restatement."""
    pred, target = torch.from_numpy(gold[f"{tag}.pred"]), torch.from_numpy(gold[f"{tag}.target"])
    hip = _hip(losses, pred.to(DEV), target.to(DEV), int(gold[f"{tag}.channel"]))
    assert hip[0].dtype == torch.float32 and hip[0].dim() == 0 and hip[0].is_cuda and hip[2].shape == pred.shape
    t64 = _restated(pred, target, torch.float64)
    y32 = (float(gold[f"{tag}.loss"]), torch.from_numpy(gold[f"{tag}.means"]), torch.from_numpy(gold[f"{tag}.grad"]).double())
    if tag == "nan":          # loss and every gradient element NaN, as the reference; the level means are finite numbers
        assert torch.isnan(hip[0]) and torch.isnan(hip[2]).all()
        em_h, em_y = (hip[1] - t64[1]).abs().max().item(), (y32[1] - t64[1]).abs().max().item()
        print(f"[nan] level means {hip[1].numpy()}  err hip {em_h:.3e} fp32 {em_y:.3e}")
        assert (t64[1] < 0).any() and em_h <= 2 * em_y + MEAN_FLOOR
        return
    _report(tag, hip, y32, t64)


REAL = [((1, 1, 48, 192, 192), 201), ((4, 1, 8, 192, 192), 202), ((1, 1, 8, 512, 512), 203), ((1, 1, 3, 50, 70), 204)]


@pytest.mark.parametrize("shape,seed", REAL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_real_sizes_vs_float64(losses, shape, seed):
    pred, target = smooth_pair(shape, 0.1, seed, DEV)        # generated once, handed to all three
    t64 = _restated(pred, target, torch.float64)
    assert (t64[1] >= 0.85).all(), f"the input recipe left a level mean below 0.85: {t64[1]}"
    y32 = _restated(pred, target, torch.float32)
    hip = _hip(losses, pred, target)
    _report("x".join(map(str, shape)), hip, y32, t64)


def test_bit_stability(losses):
    pred, target = smooth_pair((1, 1, 6, 80, 112), 0.1, 301, DEV)
    a, b = _hip(losses, pred, target), _hip(losses, pred, target)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_autograd_contract(losses):
    eng = importlib.import_module("video-to-video-diffusion_amd.losses")
    m = losses.MS_SSIM_Loss()
    pred, target = smooth_pair((2, 1, 3, 48, 64), 0.1, 302, DEV)
    _, _, g1 = _hip(losses, pred, target)
    # the upstream scalar enters the level-0 backward once
    p = pred.clone().requires_grad_(True)
    loss = m(p, target)
    assert loss.grad_fn is not None and loss.dtype == torch.float32 and loss.dim() == 0
    (3 * loss).backward()
    assert torch.equal(p.grad, 3 * g1)
    # accumulation next to another loss
    p = pred.clone().requires_grad_(True)
    (F.mse_loss(p, target) + 0.1 * m(p, target)).backward()
    q = pred.clone().requires_grad_(True)
    F.mse_loss(q, target).backward()
    assert rel_l2(p.grad.cpu(), (q.grad + 0.1 * g1).cpu()) <= 1e-6
    # two losses of one shape in one graph own their workspaces
    p1, p2 = pred.clone().requires_grad_(True), (pred * 0.5).clone().requires_grad_(True)
    (m(p1, target) + m(p2, target)).backward()
    assert torch.equal(p1.grad, g1) and not torch.equal(p2.grad, g1)
    # validation: the same loss bits, no graph, and a workspace without the coefficient maps
    with torch.no_grad():
        v = m(p, target)
    assert v.grad_fn is None and not v.requires_grad and torch.equal(v, loss.detach())
    v2 = m(pred, target)                     # grad mode, but nothing requires grad
    assert v2.grad_fn is None and torch.equal(v2, v)
    planes, h, w = 6, 48, 64
    lib = importlib.import_module("video-to-video-diffusion_amd").get_lib()
    free = eng._WORKSPACES[(0, planes, h, w, 11, 0)]
    assert len(free) == 1 and free[0].numel() * 8 < lib.msssim_workspace_bytes(planes, h, w, 11, 0) + 16
    assert lib.msssim_workspace_bytes(planes, h, w, 11, 1) > 4 * lib.msssim_workspace_bytes(planes, h, w, 11, 0)
    # dtype and layout conversions are autograd's: a bf16 pred gets a bf16 gradient, a permuted one a gradient of its own
    pb = pred.to(torch.bfloat16).requires_grad_(True)
    m(pb, target).backward()
    _, _, gb = _hip(losses, pb.detach().float(), target)
    assert pb.grad.dtype == torch.bfloat16 and torch.equal(pb.grad, gb.to(torch.bfloat16))
    pt = pred.transpose(3, 4).contiguous().transpose(3, 4).requires_grad_(True)
    assert not pt.is_contiguous()
    m(pt, target).backward()
    assert torch.equal(pt.grad, g1)
    # the gradient is pred's only, never silently
    with pytest.raises(eng.CtsiError, match="pred. only"):
        m(pred, target.clone().requires_grad_(True))
    # backward twice on one forward is refused (the maps are gone), not answered from stale memory
    p = pred.clone().requires_grad_(True)
    loss = m(p, target)
    loss.backward(retain_graph=True)
    with pytest.raises(eng.CtsiError, match="backward ran twice"):
        loss.backward()


def test_other_windows(losses):
    """Odd windows other than 11 against the fp64 restatement under the same bars."""
    pred, target = smooth_pair((1, 1, 2, 40, 56), 0.1, 303, DEV)
    for window in (1, 3, 7, 15):
        m = losses.MS_SSIM_Loss(window_size=window)
        p = pred.clone().requires_grad_(True)
        loss = m(p, target)
        loss.backward()
        res = {}
        for dtype in (torch.float64, torch.float32):
            q = pred.clone().requires_grad_(True)
            l_, means = msssim_loss(q, target, dtype, window_size=window, return_means=True)
            l_.backward()
            res[dtype] = (l_.detach().double().item(), means.detach().double().cpu(), q.grad.double())
        _report(f"window {window}", (loss.detach(), m.last_level_means.double().cpu(), p.grad), res[torch.float32],
                res[torch.float64])


def _oracle_vae(sd, x, lam, autocast=False, dev="cpu"):
    """tests/test_gpu_vae_train.py's `_oracle` (fp32 or bf16-autocast oracle VAE, on the CPU as there) with
    loss = mse + lam * the fp32 restatement of the MS-SSIM loss"""
    sdg = {k: v.detach().to(dev).clone().requires_grad_(True) for k, v in sd.items()}
    x = x.to(dev)
    with torch.autocast(dev.split(":")[0], dtype=torch.bfloat16, enabled=autocast):
        recon = R.vae_decode(sdg, R.vae_encode(sdg, x, 0.5), 0.5)
    loss = F.mse_loss(recon.float(), x.float())
    if lam:
        loss = loss + lam * msssim_loss(recon.float(), x.float(), torch.float32)
    loss.backward()
    return loss.item(), {k: v.grad.detach().float().cpu() for k, v in sdg.items()}


@pytest.mark.parametrize("tag", sorted(CONFIGS))
def test_tiny_vae_trains_with_the_term(pkg, losses, tag):
    """One step of mse + 1.0 * MS_SSIM_Loss()(recon, x): every parameter gradient against the fp32 oracle with the fp32
    restatement as its loss term."""
    lam = 1.0
    latent, seed = CONFIGS[tag]
    vae, sd = _tiny(pkg, latent, seed)
    x = torch.from_numpy(np.load(VAE_GOLD, allow_pickle=False)["x"]).to(DEV)
    assert tuple(x.shape) == SHAPE
    ref_loss, ref_g = _oracle_vae(sd, x, lam)
    _, ac_g = _oracle_vae(sd, x, lam, autocast=True)
    _, mse_g = _oracle_vae(sd, x, 0.0)
    # the condition, on the oracle alone: the term moves most gradients by more than the criterion would forgive
    moved = [rel_l2(mse_g[k], ref_g[k]) > 2 * rel_l2(ac_g[k], ref_g[k]) + 2e-2 for k, _ in vae.named_parameters()]
    print(f"[{tag}] the term moves {sum(moved)} of {len(moved)} parameter gradients beyond the criterion")
    assert sum(moved) * 2 >= len(moved)
    m = losses.MS_SSIM_Loss()
    recon, _ = vae(x)
    loss = F.mse_loss(recon.float(), x.float()) + lam * m(recon, x)
    loss.backward()
    torch.cuda.synchronize()
    means = m.last_level_means.cpu().numpy()
    print(f"[{tag}] loss hip {loss.item():.6f} oracle {ref_loss:.6f}  level means {means}")
    assert (means > 0).all()
    assert abs(loss.item() - ref_loss) <= 2e-2 * ref_loss
    _judge(vae, ref_g, ac_g, f"{tag} + ms-ssim")


def test_production_size_step(pkg, losses):
    """Base-128 VAE on the thin training patch: the loss runs next to the VAE program without touching it."""
    vae = pkg.VideoVAE(in_channels=1, latent_dim=16, base_channels=128, scaling_factor=1.0)
    load_formula(vae, 76)
    vae.train().to(DEV)
    x = formula_input((1, 1, 48, 192, 192), 45).clamp(-1, 1).to(DEV)
    recon, _ = vae(x)
    F.mse_loss(recon, x).backward()
    recon0 = recon.detach().clone()
    g0 = [p.grad.clone() for p in vae.parameters()]
    vae.zero_grad(set_to_none=True)
    m = losses.MS_SSIM_Loss()
    recon, _ = vae(x)
    loss = F.mse_loss(recon, x) + 1.0 * m(recon, x)
    loss.backward()
    torch.cuda.synchronize()
    print(f"loss {loss.item():.6f}  level means {m.last_level_means.cpu().numpy()}")
    assert torch.equal(recon.detach(), recon0)
    assert torch.isfinite(loss)
    changed = 0
    for a, p in zip(g0, vae.parameters()):
        assert torch.isfinite(p.grad).all()
        changed += int(not torch.equal(a, p.grad))
    assert changed * 2 >= len(g0)
