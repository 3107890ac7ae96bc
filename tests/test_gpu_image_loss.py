"""GPU: image-space loss terms of the diffusion stage end to end: `model.image_loss = fn`, then
`total, metrics = model(v_in, v_gt)` -> `total.backward()` -> U-Net gradients that came through the frozen decoder.

Yardstick (as tests/test_gpu_train.py): U-Net parameter gradients against the fp32 oracle's autograd of the same composite --
U-Net -> predicted clean latent -> decoder -> loss -- with the error held against the oracle's own under bf16 autocast:
   err_hip(param) <= 2 * err_autocast(param) + 2e-2   (rel-L2 per parameter tensor).
t = [100, 900] on the cosine schedule: exactly one row passes the default gate (SNR >= 1)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R
from tests import image_loss_restatement as IR
from tests.helpers import formula_input, formula_noise, rel_l2, tiny_model_sd
from tests.msssim_restatement import msssim_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_FIX = torch.tensor([100, 900])
LAMBDA_SSIM = 0.1


def inputs():
    # (24 x 16: a 6 x 4 latent.  A 24 x 20 volume has a 6 x 5 latent, which the two-level tiny U-Net cannot halve and restore.)
    v_in = formula_input((2, 1, 2, 24, 16), 18).clamp(-1, 1)
    v_gt = formula_input((2, 1, 6, 24, 16), 19).clamp(-1, 1)
    noise = formula_noise(-1, (2, 8, 6, 6, 4))
    return v_in, v_gt, noise


# the three configurations: (what the model gets, the same term for the oracle)
def _l1_only(p, y, dl, compute_auxiliary=True):      # (a) the diffusion gradient is zeroed: the image path cannot hide behind it
    return 0.0 * dl + F.l1_loss(p, y), {}


def _l1_half(p, y, dl, compute_auxiliary=True):      # (b)
    return dl + 0.5 * F.l1_loss(p, y), {}


def _ssim_ref(p, y, dl, compute_auxiliary=True):     # (c) on the oracle's side: CombinedLoss(0, 0.1, ssim_every_n_steps=1)
    return dl + LAMBDA_SSIM * msssim_loss(p, y), {}


def oracle(sd, cfg, fn, v_pred=False, autocast=False, t=T_FIX):
    """(total, {U-Net parameter name: gradient}) of the composite in torch autograd on the CPU."""
    sd = {k: v.clone() for k, v in sd.items()}
    names = [k for k in sd if k.startswith("unet.")]
    for k in names:
        sd[k].requires_grad_(True)
    v_in, v_gt, noise = inputs()
    bufs = {k[len("diffusion."):]: v for k, v in sd.items() if k.startswith("diffusion.")}
    sf = cfg["scaling_factor"]

    def run():
        with torch.no_grad():
            z_in, z_gt = R.vae_encode(sd, v_in, sf, "vae."), R.vae_encode(sd, v_gt, sf, "vae.")
            z_c = F.interpolate(z_in, size=z_gt.shape[2:], mode="trilinear", align_corners=False).float()
            z_gt = z_gt.float()
        a = bufs["sqrt_alphas_cumprod"][t].float().view(-1, 1, 1, 1, 1)
        s = bufs["sqrt_one_minus_alphas_cumprod"][t].float().view(-1, 1, 1, 1, 1)
        z_t = a * z_gt + s * noise
        pred = R.unet_forward(sd, cfg, z_t, t, z_c, "unet.").float()
        ac = bufs["alphas_cumprod"][t]
        snr = ac / (1 - ac + 1e-8)
        if v_pred:
            target, w, z0h = a * noise - s * z_gt, torch.clamp(snr, max=5.0) / (snr + 1.0), a * z_t - s * pred
        else:
            target, w, z0h = noise, torch.clamp(snr, max=5.0) / (snr + 1e-8), (z_t - s * pred) / a
        dl = (F.mse_loss(pred, target, reduction="none").reshape(t.shape[0], -1).mean(dim=1) * w).mean()
        rows = IR.rows_f64(bufs["alphas_cumprod"], t, 1.0)
        img = R.vae_decode(sd, z0h[rows], sf, "vae.").float()
        return fn(img, v_gt[rows], dl)[0]

    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            total = run()
    else:
        total = run()
    total.float().backward()
    return float(total.detach()), {k[len("unet."):]: sd[k].grad.float() for k in names}


def judge(unet, ref_g, ac_g, tag):
    """Every U-Net gradient tensor under the project's criterion (tests/test_gpu_train.py); returns the worst ratio."""
    worst = []
    gmax = max(float(g.norm()) for g in ref_g.values())
    for name, p in unet.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        g = p.grad.float().cpu()
        assert bool(torch.isfinite(g).all()), name
        if float(ref_g[name].norm()) < 1e-5 * gmax:     # q / k thirds of qkv etc.: (numerically) zero in the reference
            assert float(g.norm()) <= 1e-3 * gmax, name
            continue
        if ".qkv." in name:                              # compare the V third only; q, k are exactly zero here
            c = p.shape[0] // 3
            assert float(g[:2 * c].abs().max()) == 0.0
            e_h, e_a = rel_l2(g[2 * c:], ref_g[name][2 * c:]), rel_l2(ac_g[name][2 * c:], ref_g[name][2 * c:])
        else:
            e_h, e_a = rel_l2(g, ref_g[name]), rel_l2(ac_g[name], ref_g[name])
        worst.append((e_h / (2 * e_a + 2e-2), e_h, e_a, name))
    worst.sort(reverse=True)
    for ratio, e_h, e_a, name in worst[:5]:
        print(f"  [{tag}] {name:50s} hip {e_h:.3e}  autocast {e_a:.3e}  ratio {ratio:.2f}")
    assert worst[0][0] <= 1.0, worst[0]
    return worst[0][0]


@pytest.fixture(scope="module")
def tiny(pkg):
    model, sd, cfg = tiny_model_sd(pkg)
    model.to(DEV)
    yield model, sd, cfg
    model.image_loss = None
    model.diffusion.prediction_type = "epsilon"
    model.invalidate_engine_cache()


def run_model(model, fn, t=T_FIX, grad=True):
    v_in, v_gt, noise = (x.to(DEV) for x in inputs())
    for p in model.parameters():
        p.grad = None
    model.image_loss = fn
    total, metrics = model(v_in, v_gt, t=t.to(DEV), noise=noise)
    if grad:
        total.backward()
        torch.cuda.synchronize()
    return total, metrics


def _dec_grad_programs(model):
    return [k for k in model.vae.decoder.__dict__.get("_ctsi_programs", {}) if k[0] == "dec-grad"]


@pytest.mark.parametrize("tag,v_pred", [("a", False), ("b", False), ("c", False), ("b", True)],
                         ids=["l1-only", "dl+l1", "dl+ms-ssim", "dl+l1-v"])
def test_unet_gradients_through_the_decoder(pkg, tiny, tag, v_pred):
    model, sd, cfg = tiny
    losses = importlib_losses()
    fn_hip = {"a": _l1_only, "b": _l1_half,
              "c": losses.CombinedLoss(lambda_perceptual=0.0, lambda_ssim=LAMBDA_SSIM, ssim_every_n_steps=1)}[tag]
    fn_ref = {"a": _l1_only, "b": _l1_half, "c": _ssim_ref}[tag]
    model.diffusion.prediction_type = "v_prediction" if v_pred else "epsilon"
    try:
        total, metrics = run_model(model, fn_hip)
    finally:
        model.diffusion.prediction_type = "epsilon"
    assert metrics["image_rows"] == 1 and {"loss", "mse"} <= set(metrics)
    assert all(p.grad is None for p in model.vae.parameters())
    ref_total, ref_g = oracle(sd, cfg, fn_ref, v_pred)
    ac_total, ac_g = oracle(sd, cfg, fn_ref, v_pred, autocast=True)
    print(f"[{tag}{'-v' if v_pred else ''}] total: hip {total.item():.6f}  oracle {ref_total:.6f}  oracle/bf16-autocast {ac_total:.6f}")
    assert abs(total.item() - ref_total) <= 2 * abs(ac_total - ref_total) + 2e-2 * abs(ref_total)
    judge(model.unet, ref_g, ac_g, tag + ("-v" if v_pred else ""))
    if tag == "c":
        assert "ssim" in metrics and int(fn_hip.step) == 1


def importlib_losses():
    import importlib
    return importlib.import_module("models.losses")


def test_without_a_term_the_step_is_the_plain_one(pkg, tiny):
    """image_loss = None, and a callable that ignores the prediction: loss and gradients of training_loss, bit for bit."""
    model, _, _ = tiny
    total0, m0 = run_model(model, None)
    g0 = [p.grad.clone() for p in model.unet.parameters()]
    assert "image_rows" not in m0
    # the same through diffusion.training_loss by hand
    v_in, v_gt, noise = (x.to(DEV) for x in inputs())
    for p in model.parameters():
        p.grad = None
    with torch.no_grad():
        z_in, z_gt = model.vae._encode(v_in, "bf16"), model.vae._encode(v_gt, "bf16")
        z_c = F.interpolate(z_in, size=z_gt.shape[2:], mode="trilinear", align_corners=False)
    loss, _ = model.diffusion.training_loss(model.unet, z_gt, z_c, t=T_FIX.to(DEV), noise=noise)
    assert float(loss.detach()) == float(total0.detach())
    # the predicted latent is produced and decoded, its gradient is None: ctsi_mse_loss_bwd's path
    total1, m1 = run_model(model, lambda p, y, dl, compute_auxiliary=True: (dl, {}))
    assert m1["image_rows"] == 1 and float(total1.detach()) == float(total0.detach())
    for a, p in zip(g0, model.unet.parameters()):
        assert torch.equal(a, p.grad)


def test_skipped_terms_build_nothing(pkg, tiny):
    model, _, _ = tiny
    losses = importlib_losses()
    total0, _ = run_model(model, None)
    model.invalidate_engine_cache()
    # a CombinedLoss with nothing due at its step: no decode program, no predicted latent, the step still counts
    c = losses.CombinedLoss(lambda_perceptual=0.0, lambda_ssim=LAMBDA_SSIM, ssim_every_n_steps=10)
    c.step.fill_(1)
    assert not losses.auxiliary_due(c)
    total, m = run_model(model, c)
    assert m["image_rows"] == 1 and "ssim" not in m and int(c.step) == 2 and float(total) == float(total0)
    assert not _dec_grad_programs(model)
    progs = [p for k, p in model.unet.__dict__["_ctsi_programs"].items() if k[0] == "unet-train"]
    assert progs and all(p.z0_hat is None for p in progs)
    # no row passes the gate: the plain loss (values of t = [900, 950], not of total0), nothing built
    c.step.fill_(0)
    total, m = run_model(model, c, t=torch.tensor([900, 950]))
    assert m["image_rows"] == 0 and "ssim" not in m and not _dec_grad_programs(model)
    assert float(total) == m["mse"] and all(p.z0_hat is None for p in progs)


def test_forward_under_no_grad_returns_the_term_and_keeps_no_tape(pkg, tiny):
    model, _, _ = tiny
    losses = importlib_losses()
    model.invalidate_engine_cache()
    c = losses.CombinedLoss(lambda_perceptual=0.0, lambda_ssim=LAMBDA_SSIM, ssim_every_n_steps=1)
    with torch.no_grad():
        total, m = run_model(model, c, grad=False)
    assert total.grad_fn is None and not total.requires_grad
    assert m["image_rows"] == 1 and 0.0 < m["ssim"] <= 2.0 and m["total"] == pytest.approx(m["mse"] + LAMBDA_SSIM * m["ssim"], rel=1e-5)
    assert not _dec_grad_programs(model)          # the plain decode: no tape
    assert any(k[0] == "dec" for k in model.vae.__dict__["_ctsi_programs"])
