"""GPU: models.losses.VGGPerceptualLoss end to end -- loss and grad_pred of the HIP engine (vgg_loss_engine.VGGLossProgram).

Truth: the float64 restatement (tests/vgg_restatement.py, checked on the CPU by tests/test_host_vgg_loss.py), evaluated on
the device.  Yardstick: the SAME restatement run as torch ops under bf16 autocast on the device, measured in the test -- never
the engine's own output:
    relL2(grad_hip, grad_64)            <= 2 relL2(grad_autocast, grad_64) + 2e-2     (the training criterion, tests/test_gpu_train.py)
    |loss_hip - loss_64| / |loss_64|    <= 2 |loss_autocast - loss_64| / |loss_64| + 2^-8   (one bf16 ulp)
Weights are He-normal (std = sqrt(2 / fan_in)) with 0.05 * randn biases, so activations stay O(1) through the 14 layers; no
trained VGG weights exist here and nothing below depends on any.  Inputs are smooth random volumes in [-1, 1]; their clamped
plateaus make neighbouring activations EQUAL, so max pooling meets real ties.
"""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R
from tests.helpers import rel_l2
from tests.test_gpu_vae_train import _tiny
from tests.test_oracle_vae_train_golden import GOLD as VAE_GOLD
from tests.test_oracle_vae_train_golden import SHAPE
from tests.vgg_restatement import DEFAULT_LAYERS, Restatement, he_state_dict, slice_indices, smooth_volume

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR, LOSS_FLOOR = 2e-2, 2.0 ** -8

CASES = {
    "2x10x32x48_rate0.2": dict(shape=(2, 1, 10, 32, 48), rate=0.2, use_l1=True, layers=DEFAULT_LAYERS),   # 2 slices per sample
    "1x5x64x64_rate1.0": dict(shape=(1, 1, 5, 64, 64), rate=1.0, use_l1=True, layers=DEFAULT_LAYERS),
    "2x10x32x48_mse": dict(shape=(2, 1, 10, 32, 48), rate=0.2, use_l1=False, layers=DEFAULT_LAYERS),
    "1x5x64x64_layers_3_8_17": dict(shape=(1, 1, 5, 64, 64), rate=1.0, use_l1=True, layers=(3, 8, 17)),  # ReLU-ended, ends early
}
_CACHE = {}


@pytest.fixture(scope="module")
def losses():
    return importlib.import_module("models.losses")


@pytest.fixture(scope="module")
def sd():
    return he_state_dict(1234, upto=30)


def _inputs(shape):
    return smooth_volume(shape, 101).to(DEV), smooth_volume(shape, 102).to(DEV)


def _module(losses, sd, case):
    return losses.VGGPerceptualLoss(list(case["layers"]), case["use_l1"], case["rate"], weights=sd).to(DEV)


def _hip(m, pred, target):
    p = pred.detach().clone().requires_grad_(True)
    loss = m(p, target)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), p.grad


def _restated(sd, case, pred, target, autocast):
    r = Restatement(sd, case["layers"], case["use_l1"], case["rate"], torch.float32 if autocast else torch.float64, DEV)
    p = pred.detach().clone().requires_grad_(True)
    loss = r(p, target, autocast=autocast)
    loss.backward()
    return float(loss.detach().double()), p.grad.double().cpu()


def _reference(sd, tag):
    """(pred, target, truth, autocast yardstick) of a case: computed once, shared, never changed"""
    if tag not in _CACHE:
        case = CASES[tag]
        pred, target = _inputs(case["shape"])
        _CACHE[tag] = (pred, target, _restated(sd, case, pred, target, False), _restated(sd, case, pred, target, True))
    return _CACHE[tag]


def _errors(loss, grad, t64):
    return abs(float(loss) - t64[0]) / abs(t64[0]), rel_l2(grad.double().cpu(), t64[1])


@pytest.mark.parametrize("tag", list(CASES))
def test_loss_and_gradient_against_float64(losses, sd, tag):
    case = CASES[tag]
    pred, target, t64, ac = _reference(sd, tag)
    m = _module(losses, sd, case)
    loss, grad = _hip(m, pred, target)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    assert grad.shape == pred.shape and grad.dtype == torch.float32 and torch.isfinite(grad).all()
    (el_h, eg_h), (el_a, eg_a) = _errors(loss, grad, t64), _errors(ac[0], ac[1], t64)
    print(f"[{tag}] loss {t64[0]:.6f}  layer means {m.last_layer_means.cpu().numpy()}")
    print(f"[{tag}]   loss rel err hip {el_h:.3e} autocast {el_a:.3e} ratio {el_h / (2 * el_a + LOSS_FLOOR):.2f} | "
          f"grad relL2 hip {eg_h:.3e} autocast {eg_a:.3e} ratio {eg_h / (2 * eg_a + GRAD_FLOOR):.2f}")
    assert t64[0] > 0.05 and float(t64[1].abs().max()) > 0.0
    assert el_h <= 2 * el_a + LOSS_FLOOR
    assert eg_h <= 2 * eg_a + GRAD_FLOOR
    # exactly zero on the slices that were not sampled, a gradient on every sampled one
    d = case["shape"][2]
    idx = slice_indices(d, case["rate"]).tolist()
    rest = [s for s in range(d) if s not in idx]
    if rest:
        assert float(grad[:, :, rest].abs().max()) == 0.0
    assert all(float(grad[:, :, s].abs().max()) > 0.0 for s in idx)
    # run to run: the same bits, from a program that is reused
    loss2, grad2 = _hip(m, pred, target)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    progs = [p for v in m._ctsi_programs.values() for p in v]
    assert len(progs) == 1
    kernels = [k for _, _, k in progs[0].op_meta]
    assert any(k.endswith("m9p") for k in kernels) and "relu_bf16" in kernels      # planar launches, and the stem's ReLU pass
    print(f"[{tag}]   conv launches: {sorted(set(k for k in kernels if k.startswith('conv_')))}")


@pytest.mark.parametrize("tag", ["2x10x32x48_rate0.2", "1x5x64x64_layers_3_8_17"])
def test_gather_kernel_override_stays_within_the_criterion(losses, sd, monkeypatch, tag):
    """CTSI_CONV_PLANAR=0: every conv on the gather kernel (another summation order, ReLU as a pass of its own).  The result may
    differ from the planar form's in the last bits only: it is held to the same criterion against float64, and it is
    bit-identical run to run as well."""
    case = CASES[tag]
    pred, target, t64, ac = _reference(sd, tag)
    loss_p, grad_p = _hip(_module(losses, sd, case), pred, target)
    monkeypatch.setenv("CTSI_CONV_PLANAR", "0")
    m = _module(losses, sd, case)
    loss, grad = _hip(m, pred, target)
    kernels = [k for v in m._ctsi_programs.values() for p in v for _, _, k in p.op_meta]
    assert not any(k.endswith("m9p") for k in kernels)
    (el_h, eg_h), (el_a, eg_a) = _errors(loss, grad, t64), _errors(ac[0], ac[1], t64)
    print(f"[{tag} gather] loss rel err {el_h:.3e} (autocast {el_a:.3e}) grad relL2 {eg_h:.3e} (autocast {eg_a:.3e}); against the "
          f"planar form: loss {abs(float(loss) - float(loss_p)) / float(loss_p):.3e} grad relL2 {rel_l2(grad.cpu(), grad_p.cpu()):.3e}")
    assert el_h <= 2 * el_a + LOSS_FLOOR and eg_h <= 2 * eg_a + GRAD_FLOOR
    loss2, grad2 = _hip(m, pred, target)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_autograd_contract(losses, sd):
    tag = "2x10x32x48_rate0.2"
    case = CASES[tag]
    pred, target, _, _ = _reference(sd, tag)
    m = _module(losses, sd, case)
    loss1, g1 = _hip(m, pred, target)
    # the upstream scalar enters the deepest layer's pass once and travels linearly (exact for a power of two)
    p = pred.clone().requires_grad_(True)
    (4 * m(p, target)).backward()
    assert torch.equal(p.grad, 4 * g1)
    # accumulation next to another loss
    p = pred.clone().requires_grad_(True)
    (F.mse_loss(p, target) + 0.1 * m(p, target)).backward()
    q = pred.clone().requires_grad_(True)
    F.mse_loss(q, target).backward()
    assert rel_l2(p.grad.cpu(), (q.grad + 0.1 * g1).cpu()) <= 1e-3        # (0.1 is not exact in the bf16 gradient chain)
    # two losses of one shape in one graph own their programs
    p1, p2 = pred.clone().requires_grad_(True), (pred * 0.5).clone().requires_grad_(True)
    (m(p1, target) + m(p2, target)).backward()
    assert torch.equal(p1.grad, g1) and not torch.equal(p2.grad, g1)
    assert sum(len(v) for v in m._ctsi_programs.values()) == 2
    # no graph: the same loss bits; the target never gets a gradient (the reference computes its features under no_grad)
    with torch.no_grad():
        v = m(pred, target)
    assert v.grad_fn is None and torch.equal(v, loss1)
    t = target.clone().requires_grad_(True)
    p = pred.clone().requires_grad_(True)
    m(p, t).backward()
    assert t.grad is None and torch.equal(p.grad, g1)
    # identical volumes: the loss is exactly zero and so is the L1 gradient (sign(0) = 0)
    p = target.clone().requires_grad_(True)
    zero = m(p, target)
    zero.backward()
    assert float(zero) == 0.0 and float(p.grad.abs().max()) == 0.0
    # backward twice on one forward is refused, not answered from overwritten activations
    p = pred.clone().requires_grad_(True)
    loss = m(p, target)
    loss.backward(retain_graph=True)
    with pytest.raises(importlib.import_module("video-to-video-diffusion_amd").CtsiError, match="backward ran twice"):
        loss.backward()


def _oracle_vae(sd_vae, x, vgg, lam, autocast):
    """tests/test_gpu_vae_train.py's oracle VAE (fp32 or bf16 autocast, on the CPU as there) with
    loss = mse + lam * the restatement of the perceptual loss (float64 / under the same autocast)"""
    sdg = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in sd_vae.items()}
    x = x.cpu()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        recon = R.vae_decode(sdg, R.vae_encode(sdg, x, 0.5), 0.5)
    loss = F.mse_loss(recon.float(), x.float()) + lam * vgg(recon.float(), x.float(), autocast=autocast).float()
    loss.backward()
    return loss.item(), {k: v.grad.detach().float().cpu() for k, v in sdg.items()}


def test_tiny_vae_trains_with_the_term(pkg, losses, sd):
    """One VAE training step with mse + 0.1 * VGGPerceptualLoss(weights=...)(recon, x) at the smallest shape of
    tests/test_gpu_vae_train.py: three parameter gradients (first encoder conv, last decoder conv, the latent seam) under the
    training criterion."""
    lam = 0.1
    vae, sd_vae = _tiny(pkg, 8, 50)
    x = torch.from_numpy(np.load(VAE_GOLD, allow_pickle=False)["x"]).to(DEV)
    assert tuple(x.shape) == SHAPE
    ref_loss, ref_g = _oracle_vae(sd_vae, x, Restatement(sd, dtype=torch.float64), lam, False)
    _, ac_g = _oracle_vae(sd_vae, x, Restatement(sd, dtype=torch.float32), lam, True)
    m = losses.VGGPerceptualLoss(weights=sd).to(DEV)
    recon, _ = vae(x)
    perceptual = m(recon, x)
    loss = F.mse_loss(recon.float(), x.float()) + lam * perceptual
    loss.backward()
    torch.cuda.synchronize()
    print(f"loss hip {loss.item():.6f} oracle {ref_loss:.6f} (perceptual term {perceptual.item():.6f})")
    assert abs(loss.item() - ref_loss) <= 2e-2 * ref_loss
    params = dict(vae.named_parameters())
    for name in ("encoder.conv_in.conv.weight", "decoder.conv_out.weight", "encoder.quant_conv.weight"):
        e_h, e_a = rel_l2(params[name].grad.float().cpu(), ref_g[name]), rel_l2(ac_g[name], ref_g[name])
        print(f"  {name:32s} hip {e_h:.3e}  autocast {e_a:.3e}  ratio {e_h / (2 * e_a + GRAD_FLOOR):.2f}")
        assert e_h <= 2 * e_a + GRAD_FLOOR, name
