"""GPU: the EMA / global-norm-clipping part of the optimizer step (optim.FusedAdamW(ema=, max_grad_norm=), optim.clip_grad_norm_,
ema.EMAWeights; csrc/optim.hip).

Yardsticks: the plain FusedAdamW step (bit for bit where nothing may change), torch's lerp_ on the same values (1e-6 of the
tensor's largest magnitude: the same arithmetic in the same precision), the float64 norm of the concatenated gradients (1e-6
relative: an fp64 sum rounded once to fp32 is 2^-24 off, the margin covers the scale and the square root), and
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW with test_gpu_optim.py's bounds (parameters 1e-6, moments 2e-6)."""
import copy
import importlib

import pytest
import torch

from tests.helpers import formula_input, formula_noise, tiny_model_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(128, 64, 3, 3, 3), (128,), (7,), (33, 5), (1,), (512, 257), (64, 32, 3, 4, 4), (3, 3)]
KW = dict(betas=(0.9, 0.98), eps=1e-7, weight_decay=0.05)


def _params(seed):
    """test_gpu_optim.py's parameter set (sizes that are no multiples of 4), with one deliberately misaligned view: the (33, 5)
    parameter starts one float into its storage, so its rows take the scalar path."""
    ps = []
    for i, s in enumerate(SHAPES):
        v = formula_input(s, seed + i).to(DEV) * (0.5 + 0.1 * i)
        if s == (33, 5):
            buf = torch.empty(v.numel() + 1, device=DEV)
            buf[1:].copy_(v.reshape(-1))
            v = buf[1:].view(s)
            assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        ps.append(torch.nn.Parameter(v))
    return ps


def _named(ps):
    return [(f"p{i}", p) for i, p in enumerate(ps)]


def _groups(ps):
    return [dict(params=ps[:3], lr=3e-3, name="a"), dict(params=ps[3:], lr=1e-3 * 0.1, name="b")]


def _set_grads(step, *param_sets, scale=0.3, skip=None):
    for i, group in enumerate(zip(*param_sets)):
        g = formula_input(tuple(group[0].shape), 500 + 10 * step + i).to(DEV) * scale
        for p in group:
            p.grad = None if i == skip else g.clone()


def _norm64(params):
    gs = [p.grad.detach().double().reshape(-1) for p in params if p.grad is not None]
    return torch.linalg.vector_norm(torch.cat(gs))


def _close(a, b, rel, what):
    scale = float(b.detach().abs().max())
    err = float((a.detach() - b.detach()).abs().max())
    print(f"{what}: max error {err:.3e}, bound {rel * scale:.3e}")
    assert err <= rel * scale + 1e-30, what


def test_fused_ema_step_changes_nothing_it_should_not_and_averages(pkg):
    """(1) FusedAdamW(ema=...) leaves p, exp_avg, exp_avg_sq bit-identical to plain FusedAdamW over 3 steps (the third with a
    parameter that has no gradient); (2) the shadows are torch's lerp_ of the post-step parameters, and the fused shadows and
    the stand-alone update() shadows are the same bits."""
    ours, twin = _params(100), _params(100)
    ema = pkg.EMAWeights(_named(ours), decay=0.99)
    ema_alone = pkg.EMAWeights(_named(twin), decay=0.99)              # stand-alone: twin stepped by plain FusedAdamW
    ref = [p.detach().clone() for p in twin]                          # torch.lerp_ on the twin's post-step parameters
    o1 = pkg.FusedAdamW(_groups(ours), ema=ema, max_grad_norm=None, **KW)
    o2 = pkg.FusedAdamW(_groups(twin), **KW)
    assert o1.last_grad_norm is None
    for step in range(3):
        _set_grads(step, ours, twin, skip=4 if step == 2 else None)
        o1.step()
        o2.step()
        ema_alone.update()
        w = 1.0 - ema.decay_at(step)
        for r, p in zip(ref, twin):
            r.lerp_(p.detach(), w)
        o1.zero_grad(set_to_none=True)
        o2.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert ema.num_updates == ema_alone.num_updates == 3
    for i, (a, b) in enumerate(zip(ours, twin)):
        assert torch.equal(a.detach(), b.detach()), SHAPES[i]
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(o1.state[a][k], o2.state[b][k]), (k, SHAPES[i])
        assert float(o1.state[a]["step"]) == float(o2.state[b]["step"])
    for i, (s, s_alone, r) in enumerate(zip(ema.shadows, ema_alone.shadows, ref)):
        assert torch.equal(s, s_alone), f"fused and stand-alone shadows differ: {SHAPES[i]}"
        _close(s, r, 1e-6, f"shadow {SHAPES[i]} vs lerp_")
    assert not torch.equal(ema.shadows[4], ours[4].detach())          # the parameter that sat step 3 out was still averaged
    with pytest.raises(pkg.CtsiError, match="attached"):              # no silent double average
        ema.update()
    with ema.applied():
        _set_grads(9, ours)
        with pytest.raises(pkg.CtsiError, match="applied"):
            o1.step()
    assert float(o1.state[ours[0]]["step"]) == 3.0                    # the refused step counted nothing


def test_grad_norm_against_float64_and_run_to_run(pkg):
    ours = _params(200)
    _set_grads(0, ours, scale=0.3, skip=4)
    want = float(_norm64(ours))
    unclipped = [None if p.grad is None else p.grad.clone() for p in ours]
    n1 = pkg.clip_grad_norm_(ours, 1e9)                               # far above the norm: coefficient exactly 1
    n2 = pkg.clip_grad_norm_(ours, 1e9)
    assert n1.device.type == "cuda" and n1.dim() == 0
    print(f"norm {float(n1):.9g}, float64 {want:.9g}, rel {abs(float(n1) - want) / want:.3e}")
    assert abs(float(n1) - want) <= 1e-6 * want
    assert torch.equal(n1, n2), "the norm is not bit-identical from run to run"
    for p, g in zip(ours, unclipped):
        assert g is None or torch.equal(p.grad, g)                    # coefficient 1: the gradients are untouched
    with pytest.raises(pkg.CtsiError, match="norm_type"):
        pkg.clip_grad_norm_(ours, 1.0, norm_type=1.0)
    # below max_norm the fused clipped step IS the unclipped step
    a, b = _params(210), _params(210)
    o1, o2 = pkg.FusedAdamW(_groups(a), max_grad_norm=1e9, **KW), pkg.FusedAdamW(_groups(b), **KW)
    for step in range(2):
        _set_grads(step, a, b)
        o1.step()
        o2.step()
        assert abs(float(o1.last_grad_norm) - float(_norm64(a))) <= 1e-6 * float(_norm64(a))
    for x, y in zip(a, b):
        assert torch.equal(x.detach(), y.detach())
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(o1.state[x][k], o2.state[y][k])


def test_nonfinite_gradient_gives_torchs_nonfiniteness(pkg):
    ours, ref = _params(220), _params(220)
    _set_grads(0, ours, ref)
    for ps in (ours, ref):
        ps[5].grad[17, 3] = float("inf")
    n_ref = torch.nn.utils.clip_grad_norm_(ref, 1.0)
    n = pkg.clip_grad_norm_(ours, 1.0)
    assert not bool(torch.isfinite(n)) and not bool(torch.isfinite(n_ref))
    assert bool(torch.isinf(n)) == bool(torch.isinf(n_ref)) and bool(torch.isnan(n)) == bool(torch.isnan(n_ref))
    for a, b in zip(ours, ref):                                       # and the gradients end up non-finite where torch's do
        assert torch.equal(torch.isfinite(a.grad), torch.isfinite(b.grad))
    with pytest.raises(RuntimeError, match="non-finite"):
        pkg.clip_grad_norm_(ours, 1.0, error_if_nonfinite=True)
    ours[5].grad[17, 3] = float("nan")
    assert bool(torch.isnan(pkg.clip_grad_norm_(ours, 1.0)))


def test_clipped_step_matches_torch_clip_then_adamw(pkg):
    """FusedAdamW(max_grad_norm=c) against clip_grad_norm_(params, c) + torch.optim.AdamW.step() over 3 steps.  torch's norm is
    an fp32 reduction and the yardstick is float64: on a step where torch's coefficient is further than 4 fp32 ulps (2.5e-7)
    from the float64 one, the twin's gradients are scaled by the float64 coefficient instead (and the step says so)."""
    c = 0.5
    ours, ref = _params(300), _params(300)
    o1, o2 = pkg.FusedAdamW(_groups(ours), max_grad_norm=c, **KW), torch.optim.AdamW(_groups(ref), **KW)
    for step in range(3):
        _set_grads(step, ours, ref, skip=4 if step == 2 else None)
        unclipped = [None if p.grad is None else p.grad.clone() for p in ours]
        want = float(_norm64(ref))
        assert want > 2 * c                                           # these steps really clip
        n_ref = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in ref if p.grad is not None]))
        coef64, coef_torch = c / (want + 1e-6), c / (float(n_ref) + 1e-6)      # (torch's clip_grad_norm_ norm, not yet applied)
        fair = abs(coef_torch - coef64) <= 2.5e-7 * coef64
        print(f"step {step}: float64 norm {want:.9g}, torch fp32 {float(n_ref):.9g}, coefficient rel diff "
              f"{abs(coef_torch - coef64) / coef64:.3e} -> twin clipped by {'torch' if fair else 'the float64 coefficient'}")
        if fair:
            torch.nn.utils.clip_grad_norm_(ref, c)
        else:
            for p in ref:
                if p.grad is not None:
                    p.grad.mul_(min(1.0, coef64))
        o1.step()
        o2.step()
        assert abs(float(o1.last_grad_norm) - want) <= 1e-6 * want
        for p, g in zip(ours, unclipped):                             # .grad keeps its unclipped values
            assert g is None or torch.equal(p.grad, g)
        o1.zero_grad(set_to_none=True)
        o2.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(ours, ref)):
        _close(a, b, 1e-6, f"param {SHAPES[i]}")
        for k in ("exp_avg", "exp_avg_sq"):
            _close(o1.state[a][k], o2.state[b][k], 2e-6, f"{k} {SHAPES[i]}")
        assert float(o1.state[a]["step"]) == float(o2.state[b]["step"])


def test_clipped_step_under_gradscaler(pkg):
    """Under a GradScaler the gradients are unscaled by the time step() runs (scaler.step unscales if the loop did not), so
    max_grad_norm clips the true gradients: same parameters as unscale_ + torch's clip_grad_norm_ + torch.optim.AdamW."""
    c = 0.5
    ours, ref = _params(600)[:4], _params(600)[:4]
    o1 = pkg.FusedAdamW(ours, lr=1e-2, weight_decay=0.02, max_grad_norm=c)
    o2 = torch.optim.AdamW(ref, lr=1e-2, weight_decay=0.02)
    g1, g2 = torch.amp.GradScaler("cuda", init_scale=1024.0), torch.amp.GradScaler("cuda", init_scale=1024.0)
    for step in range(3):
        for ps, opt, sc in ((ours, o1, g1), (ref, o2, g2)):
            loss = sum((p * formula_input(tuple(p.shape), 700 + 10 * step + i).to(DEV)).sum() for i, p in enumerate(ps))
            opt.zero_grad(set_to_none=True)
            sc.scale(loss).backward()
            if opt is o2:
                sc.unscale_(opt)
                torch.nn.utils.clip_grad_norm_(ps, c)
            sc.step(opt)
            sc.update()
        want = float(_norm64(ours))                                   # (unscaled in place by scaler.step; never clipped)
        assert want > 2 * c and abs(float(o1.last_grad_norm) - want) <= 1e-6 * want
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(ours, ref)):
        _close(a, b, 2e-6, f"param {SHAPES[i]} under GradScaler")     # (test_gpu_optim.py's bound under a GradScaler)


def test_standalone_clip_grad_norm_matches_torch(pkg):
    ours, ref = _params(400), _params(400)
    _set_grads(1, ours, ref, skip=2)
    want = float(_norm64(ref))
    n_ref = torch.nn.utils.clip_grad_norm_(ref, 0.25)
    n = pkg.clip_grad_norm_(ours, 0.25)
    torch.cuda.synchronize()
    assert abs(float(n) - want) <= 1e-6 * want and abs(float(n) - float(n_ref)) <= 1e-6 * want
    assert ours[2].grad is None
    for i, (a, b) in enumerate(zip(ours, ref)):
        if b.grad is not None:
            _close(a.grad, b.grad, 2e-6, f"clipped grad {SHAPES[i]}")
    after = float(_norm64(ours))
    assert abs(after - 0.25) <= 1e-5 * 0.25


def test_sampling_with_the_averaged_weights(pkg):
    """generate() inside ema.applied() is generate() of a twin model holding the shadows, bit for bit; after the block it is
    what it was before; and training goes on as if the block had never been entered (version bump, re-pack and the weight
    cache together)."""
    model, sd, cfg = tiny_model_sd(pkg)
    plain, _, _ = tiny_model_sd(pkg)                                  # never enters the block
    model.to(DEV)
    plain.to(DEV)
    v_in = formula_input((2, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    v_gt = formula_input((2, 1, 4, 16, 16), 19).clamp(-1, 1).to(DEV)
    t, nz = torch.tensor([612, 77], device=DEV), formula_noise(-1, (2, 8, 4, 4, 4)).to(DEV)
    opts, emas = [], []
    for m in (model, plain):
        for p in m.vae.parameters():
            p.requires_grad_(False)
        emas.append(pkg.EMAWeights(m.unet, decay=0.9, prefix="unet."))
        opts.append(pkg.FusedAdamW(m.unet.parameters(), lr=2e-3, weight_decay=0.01, engine_modules=[m.unet], ema=emas[-1],
                                   max_grad_norm=1.0))

    def train_step():
        losses = []
        for m, o in zip((model, plain), opts):
            loss, _ = m(v_in, v_gt, t=t, noise=nz)
            loss.backward()
            o.step()
            o.zero_grad(set_to_none=True)
            losses.append(float(loss.detach()))
        return losses

    for _ in range(3):
        l_model, l_plain = train_step()
        assert l_model == pytest.approx(l_plain, rel=1e-6)
    ema = emas[0]
    assert set(ema.names) <= set(model.state_dict())
    gen = lambda m: m.generate(v_in[:1], "ddim", num_inference_steps=4, target_depth=4, noise_fn=formula_noise)
    before = gen(model).clone()
    twin, _, _ = tiny_model_sd(pkg)
    twin.load_state_dict(copy.deepcopy(model.state_dict()))
    missing, unexpected = twin.load_state_dict({k: v.clone() for k, v in ema.state_dict()["shadow"].items()}, strict=False)
    assert not unexpected and all(k.startswith(("vae.", "diffusion.")) for k in missing)
    twin.to(DEV).eval()
    want = gen(twin).clone()
    raw = [p.detach().clone() for p in model.unet.parameters()]
    ptrs = [p.data_ptr() for p in model.unet.parameters()]
    with ema.applied():
        inside = gen(model).clone()
    after = gen(model).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(inside).all()
    assert not torch.equal(want, before), "the averaged weights should sample something else than the raw ones"
    assert torch.equal(inside, want), f"max diff {float((inside - want).abs().max()):.3e}"
    assert torch.equal(after, before), f"max diff {float((after - before).abs().max()):.3e}"
    assert all(torch.equal(p.detach(), r) for p, r in zip(model.unet.parameters(), raw))
    assert [p.data_ptr() for p in model.unet.parameters()] == ptrs
    l_model, l_plain = train_step()
    print("loss after the block / of the twin that never entered it:", l_model, l_plain)
    assert l_model == pytest.approx(l_plain, rel=1e-6)
    for a, b in zip(emas[0].shadows, emas[1].shadows):
        assert torch.equal(a, b)


def test_full_size_fused_step_with_both_options(pkg):
    """The config-3 U-Net's parameter list (264.66 M parameters, random fp32 gradients, no forward) through ONE fused step with
    clipping and the EMA: finite results, the norm against float64, the shadows against lerp_ of the new parameters."""
    unet = pkg.UNet3D(latent_dim=8).to(DEV)
    params = [p for p in unet.parameters() if p.requires_grad]
    assert sum(p.numel() for p in params) > 264e6
    gen = torch.Generator(device=DEV).manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, device=DEV, generator=gen) * 1e-3
    want = float(_norm64(params))
    ema = pkg.EMAWeights(unet, decay=0.9999)
    old_shadow = [s.clone() for s in ema.shadows]
    assert all(torch.equal(s, p.detach()) for s, p in zip(old_shadow, params))
    c = 0.5 * want
    opt = pkg.FusedAdamW(params, lr=1e-3, weight_decay=0.01, ema=ema, max_grad_norm=c)
    opt.step()
    torch.cuda.synchronize()
    norm = float(opt.last_grad_norm)
    print(f"full size: norm {norm:.9g}, float64 {want:.9g}, rel {abs(norm - want) / want:.3e}")
    assert abs(norm - want) <= 1e-6 * want
    w = 1.0 - ema.decay_at(0)
    worst = 0.0
    for p, s, s0 in zip(params, ema.shadows, old_shadow):
        assert torch.isfinite(p).all() and torch.isfinite(s).all()
        assert torch.isfinite(opt.state[p]["exp_avg"]).all() and torch.isfinite(opt.state[p]["exp_avg_sq"]).all()
        r = s0.lerp_(p.detach(), w)
        scale = float(r.abs().max())
        err = float((s - r).abs().max())
        worst = max(worst, err / (scale + 1e-30))
        assert err <= 1e-6 * scale + 1e-30, tuple(p.shape)
    print(f"full size: worst shadow error vs lerp_ {worst:.3e} of the tensor's largest magnitude")
