"""GPU: models.losses.LPIPS end to end -- per-image values and the gradient of in0 from the HIP engine (VGGLossProgram with the
VGG-16 module table and the LPIPS distance) -- and utils.metrics.calculate_lpips.

Truth: the float64 restatement (tests/lpips_restatement.py, checked on the CPU by tests/test_host_lpips.py), evaluated on the
device.  Yardstick, as in tests/test_gpu_vgg_loss.py: the SAME restatement run as torch ops under bf16 autocast on the device,
measured in the test -- never the engine's own output:
    |v_hip - v_64| / |v_64|             <= 2 |v_autocast - v_64| / |v_64| + 2^-8      (every per-image value and every scalar loss)
    relL2(grad_hip, grad_64)            <= 2 relL2(grad_autocast, grad_64) + 2e-2
Weights are He-normal, heads random and non-negative (fixed seeds); inputs are target in [-1, 1] and pred = target + 0.3 noise,
for which every float64 value exceeds 0.05 (asserted), so the relative error means something.
"""
import importlib

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import formula_input, formula_noise, rel_l2, tiny_model_sd
from tests.lpips_restatement import Restatement, he_state_dict, lpips_state_dict, make_pair, random_heads, volume_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR, LOSS_FLOOR = 2e-2, 2.0 ** -8
UP = (1.0, 2.0, 0.5)          # the per-image upstream gradient of the 4-D cases: distinct, exact in bf16

CASES = {
    "1x3x16x16": dict(shape=(1, 3, 16, 16), seed=21),                       # the smallest: the last tap is one position
    "3x1x32x48": dict(shape=(3, 1, 32, 48), seed=22),                       # odd batch, non-square, grey input
    "2x1x5x32x32_middle": dict(shape=(2, 1, 5, 32, 32), seed=23, slices="middle"),
    "2x1x5x32x32_rate0.5": dict(shape=(2, 1, 5, 32, 32), seed=23, slices=0.5),
}
_CACHE = {}


@pytest.fixture(scope="module")
def losses():
    return importlib.import_module("models.losses")


@pytest.fixture(scope="module")
def sd():
    return he_state_dict(1234)


@pytest.fixture(scope="module")
def heads():
    return random_heads(77)


def _module(losses, sd, heads, **kw):
    return losses.LPIPS(weights=sd, lin_weights=heads, **kw).to(DEV)


def _scalar(out, shape):
    """what the tests differentiate: the volume loss itself, or the per-image values under the distinct upstream UP"""
    if len(shape) == 5:
        return out
    return (out.reshape(-1) * torch.tensor(UP[:shape[0]], dtype=out.dtype, device=out.device)).sum()


def _hip(m, pred, target, **kw):
    p = pred.detach().clone().requires_grad_(True)
    out = m(p, target, **kw)
    _scalar(out, pred.shape).backward()
    torch.cuda.synchronize()
    return out.detach(), p.grad


def _restated(sd, heads, case, pred, target, autocast):
    r = Restatement(sd, heads, torch.float32 if autocast else torch.float64, DEV)
    p = pred.detach().clone().requires_grad_(True)
    if len(case["shape"]) == 5:
        m = importlib.import_module("models.losses").LPIPS(weights=sd, lin_weights=heads, slices=case["slices"])
        out = volume_loss(r, p, target, m.slice_indices(case["shape"][2]), autocast=autocast)
    else:
        out = r(p, target, autocast=autocast)
    _scalar(out, case["shape"]).backward()
    return out.detach().double().reshape(-1).cpu(), p.grad.double().cpu()


def _reference(sd, heads, tag):
    """(pred, target, truth, autocast yardstick) of a case: computed once, shared, never changed"""
    if tag not in _CACHE:
        case = CASES[tag]
        pred, target = (x.to(DEV) for x in make_pair(case["shape"], case["seed"]))
        _CACHE[tag] = (pred, target, _restated(sd, heads, case, pred, target, False), _restated(sd, heads, case, pred, target, True))
    return _CACHE[tag]


def _judge(tag, vals, grad, t64, ac):
    vals = vals.double().reshape(-1).cpu()
    assert float(t64[0].min()) > 0.05 and float(t64[1].abs().max()) > 0.0
    for i in range(vals.numel()):
        e_h, e_a = abs(float(vals[i] - t64[0][i])) / float(t64[0][i]), abs(float(ac[0][i] - t64[0][i])) / float(t64[0][i])
        print(f"[{tag}] value {i}: float64 {float(t64[0][i]):.6f} hip rel err {e_h:.3e} autocast {e_a:.3e} ratio {e_h / (2 * e_a + LOSS_FLOOR):.2f}")
        assert e_h <= 2 * e_a + LOSS_FLOOR, (tag, i)
    eg_h, eg_a = rel_l2(grad.double().cpu(), t64[1]), rel_l2(ac[1], t64[1])
    print(f"[{tag}] grad relL2 hip {eg_h:.3e} autocast {eg_a:.3e} ratio {eg_h / (2 * eg_a + GRAD_FLOOR):.2f}")
    assert eg_h <= 2 * eg_a + GRAD_FLOOR, tag


@pytest.mark.parametrize("tag", list(CASES))
def test_values_and_gradient_against_float64(losses, sd, heads, tag):
    case = CASES[tag]
    pred, target, t64, ac = _reference(sd, heads, tag)
    m = _module(losses, sd, heads, **({"slices": case["slices"]} if "slices" in case else {}))
    out, grad = _hip(m, pred, target)
    if len(case["shape"]) == 4:
        assert out.shape == (case["shape"][0], 1, 1, 1)
    else:
        assert out.dim() == 0
    assert out.dtype == torch.float32 and out.is_cuda
    assert grad.shape == pred.shape and grad.dtype == torch.float32 and torch.isfinite(grad).all()
    print(f"[{tag}] tap means {m.last_layer_means.cpu().numpy()}")
    assert m.last_layer_means.shape == (5,)
    _judge(tag, out, grad, t64, ac)
    if len(case["shape"]) == 5:         # exactly zero on the slices that were not selected, a gradient on every selected one
        d = case["shape"][2]
        idx = m.slice_indices(d).tolist()
        rest = [s for s in range(d) if s not in idx]
        assert rest and float(grad[:, :, rest].abs().max()) == 0.0
        assert all(float(grad[:, :, s].abs().max()) > 0.0 for s in idx)
    out2, grad2 = _hip(m, pred, target)          # run to run: the same bits, from a program that is reused
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    progs = [p for v in m._ctsi_programs.values() for p in v]
    assert len(progs) == 1
    kernels = [k for _, _, k in progs[0].op_meta]
    assert kernels.count("lpips_dist") == 5 and kernels.count("lpips_grad_relu_bwd") == 5 and "lpips_finalize" in kernels
    assert "feat_loss" not in kernels


def test_baseline_heads_and_normalize(losses, sd, heads):
    tag = "3x1x32x48"
    pred, target, _, _ = _reference(sd, heads, tag)
    # lpips=False: all-ones heads, against the restatement with ones
    ones = [torch.ones_like(h) for h in heads]
    m1 = losses.LPIPS(weights=sd, lpips=False).to(DEV)
    out, grad = _hip(m1, pred, target)
    case = CASES[tag]
    _judge(tag + " lpips=False", out, grad, _restated(sd, ones, case, pred, target, False), _restated(sd, ones, case, pred, target, True))
    # normalize=True on [0, 1] inputs is the call on 2 x - 1, bit for bit (values that are exact under x -> 2 x - 1)
    m = _module(losses, sd, heads)
    p01 = (torch.randint(0, 257, pred.shape, generator=torch.Generator().manual_seed(3)).float() / 256).to(DEV)
    t01 = (torch.randint(0, 257, pred.shape, generator=torch.Generator().manual_seed(4)).float() / 256).to(DEV)
    a, ga = _hip(m, p01, t01, normalize=True)
    b, gb = _hip(m, 2 * p01 - 1, 2 * t01 - 1)
    assert torch.equal(a, b) and torch.equal(ga, 2 * gb)


def test_autograd_contract(pkg, losses, sd, heads):
    tag = "3x1x32x48"
    pred, target, _, _ = _reference(sd, heads, tag)
    m = _module(losses, sd, heads)
    out1, g1 = _hip(m, pred, target)
    # the upstream gradient enters each tap's pass once and travels linearly (exact for a power of two)
    p = pred.clone().requires_grad_(True)
    (4 * _scalar(m(p, target), pred.shape)).backward()
    assert torch.equal(p.grad, 4 * g1)
    # accumulation into .grad next to another loss
    p = pred.clone().requires_grad_(True)
    F.mse_loss(p, target).backward()
    q = p.grad.clone()
    _scalar(m(p, target), pred.shape).backward()
    assert torch.equal(p.grad, q + g1)
    # two distances of one shape in one graph own their programs
    p1, p2 = pred.clone().requires_grad_(True), (pred * 0.5).clone().requires_grad_(True)
    (_scalar(m(p1, target), pred.shape) + _scalar(m(p2, target), pred.shape)).backward()
    assert torch.equal(p1.grad, g1) and not torch.equal(p2.grad, g1)
    assert sum(len(v) for v in m._ctsi_programs.values()) == 2
    # no graph: the same bits
    with torch.no_grad():
        v = m(pred, target)
    assert v.grad_fn is None and torch.equal(v, out1)
    # identical inputs: exactly zero, and a zero gradient
    p = target.clone().requires_grad_(True)
    zero = m(p, target)
    zero.sum().backward()
    assert float(zero.abs().max()) == 0.0 and float(p.grad.abs().max()) == 0.0
    # the gradient exists for in0 only
    t = target.clone().requires_grad_(True)
    with pytest.raises(pkg.CtsiError, match="detach it"):
        m(pred.clone().requires_grad_(True), t)
    with torch.no_grad():
        assert torch.equal(m(pred, t), out1)
    # backward twice on one forward is refused, not answered from overwritten activations
    p = pred.clone().requires_grad_(True)
    loss = m(p, target).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(pkg.CtsiError, match="backward ran twice"):
        loss.backward()


def test_the_three_lines_of_the_reference_trainer(losses, sd, heads):
    """AutoencoderLoss.perceptual_loss: the middle slice of recon and x, repeated to three channels, the net, .mean() --
    with perceptual_net = LPIPS(weights=...) built from an lpips.LPIPS state dict"""
    tag = "2x1x5x32x32_middle"
    pred, target, t64, ac = _reference(sd, heads, tag)
    perceptual_net = losses.LPIPS(weights=lpips_state_dict(sd, heads)).to(DEV)
    recon = pred.clone().requires_grad_(True)
    mid = recon.shape[2] // 2
    pred_slice = recon[:, :, mid, :, :].repeat(1, 3, 1, 1)
    target_slice = target[:, :, mid, :, :].repeat(1, 3, 1, 1)
    loss = perceptual_net(pred_slice, target_slice).mean()
    loss.backward()
    torch.cuda.synchronize()
    _judge("trainer lines", loss.detach(), recon.grad, t64, ac)
    assert float(recon.grad[:, :, [s for s in range(recon.shape[2]) if s != mid]].abs().max()) == 0.0


def test_combined_loss_takes_the_module(losses, sd, heads):
    tag = "2x1x5x32x32_middle"
    pred, target, t64, ac = _reference(sd, heads, tag)
    c = losses.CombinedLoss(lambda_perceptual=0.1, lambda_ssim=0.0, perceptual_every_n_steps=1).to(DEV)
    c.perceptual_loss = _module(losses, sd, heads)
    p = pred.clone().requires_grad_(True)
    dl = F.mse_loss(p, target)
    total, parts = c(p, target, dl)
    total.backward()
    torch.cuda.synchronize()
    direct, g_direct = _hip(c.perceptual_loss, pred, target)
    assert parts["perceptual"] == float(direct) and int(c.step) == 1
    assert abs(parts["total"] - (parts["diffusion"] + 0.1 * parts["perceptual"])) <= 1e-6 * parts["total"]
    q = pred.clone().requires_grad_(True)
    F.mse_loss(q, target).backward()
    assert rel_l2(p.grad.cpu(), (q.grad + 0.1 * g_direct).cpu()) <= 1e-3        # (0.1 is not exact in the bf16 gradient chain)


def test_image_loss_of_the_diffusion_stage_takes_the_module(pkg, losses, sd, heads):
    """model.image_loss = a term built on LPIPS: one step of the tiny model, the U-Net gets a gradient
    through the frozen decoder and the VAE none.  32 x 16 volumes: the tiny configuration with H, W multiples of 16."""
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    m = _module(losses, sd, heads)
    seen = {}

    def term(p, y, dl, compute_auxiliary=True):
        v = m(p, y)
        seen["lpips"] = v.detach()
        return dl + 0.1 * v, {"lpips": float(v)}

    v_in = formula_input((2, 1, 2, 32, 16), 18).clamp(-1, 1).to(DEV)
    v_gt = formula_input((2, 1, 6, 32, 16), 19).clamp(-1, 1).to(DEV)
    noise = formula_noise(-1, (2, 8, 6, 8, 4)).to(DEV)
    try:
        model.image_loss = term
        total, metrics = model(v_in, v_gt, t=torch.tensor([100, 100], device=DEV), noise=noise)
        total.backward()
        torch.cuda.synchronize()
    finally:
        model.image_loss = None
    assert metrics["image_rows"] >= 1 and float(seen["lpips"]) > 0.0 and torch.isfinite(total)
    assert abs(float(total) - (metrics["loss"] + 0.1 * float(seen["lpips"]))) <= 1e-5 * abs(float(total))
    g = model.unet.conv_in.weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0.0
    assert all(p.grad is None for p in model.vae.parameters())
    model.invalidate_engine_cache()


def test_calculate_lpips(losses, sd, heads):
    """5 slices in groups of 2: the last group is filled up and its repeat dropped; every per-slice value is the module's on
    the same group of images bit for bit, and within the criterion's floor of the module's value on the slice alone (another
    batch size may plan its convolutions differently)."""
    metrics = importlib.import_module("utils.metrics")
    m = _module(losses, sd, heads)
    g = torch.Generator().manual_seed(31)
    v2 = torch.rand(1, 1, 5, 32, 32, generator=g)
    v1 = (v2 + 0.15 * torch.randn(v2.shape, generator=g)).clamp(0, 1)
    v1, v2 = v1.to(DEV), v2.to(DEV)
    res = metrics.calculate_lpips(v1, v2, m, group=2)
    assert set(res) == {"lpips", "per_slice"} and len(res["per_slice"]) == 5
    assert abs(res["lpips"] - sum(res["per_slice"]) / 5) <= 1e-12
    a, b = v1[0].transpose(0, 1), v2[0].transpose(0, 1)            # (5, 1, 32, 32)
    with torch.no_grad():
        for idx in ([0, 1], [2, 3], [4, 4]):
            want = m(a[idx], b[idx], normalize=True).reshape(-1).double().cpu().tolist()
            for j, s in enumerate(idx):
                assert res["per_slice"][s] == want[j], s
        for s in range(5):
            alone = float(m(a[s:s + 1], b[s:s + 1], normalize=True))
            assert abs(res["per_slice"][s] - alone) <= 2 * LOSS_FLOOR * alone
    # (D, H, W) volumes in [0, max_val]
    res3 = metrics.calculate_lpips(255 * v1[0, 0], 255 * v2[0, 0], m, max_val=255.0, group=2)
    assert max(abs(x - y) for x, y in zip(res3["per_slice"], res["per_slice"])) <= 2 * LOSS_FLOOR * max(res["per_slice"])
    assert sum(len(v) for v in m._ctsi_programs.values()) == 2          # one program for the groups, one for the single slices
    with pytest.raises(ValueError, match="expected two"):
        metrics.calculate_lpips(v1, v2[:, :, :4], m)
