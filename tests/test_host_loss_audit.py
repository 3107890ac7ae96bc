"""CPU: the float64 references of tests/loss_audit.py against torch (autograd or plain ops in float64) on random data, what the
per-launch comparison sees that the end-to-end bounds do not, and that every launch of vgg_loss_engine.py carries a record whose
kind has a reference.

The gap.  tests/test_gpu_vgg_loss.py holds the VGG loss to
    |v - v_64| / |v_64| <= 2 |v_autocast - v_64| / |v_64| + 2^-8        relL2(grad) <= 2 relL2(grad_autocast) + 2e-2
against its float64 restatement.  Here that restatement runs with a tap on each of VGG-19's 16 convs (MSE, 2 images at 32 x 32)
and two plumbing errors are put into it:
  A  the coefficient of ONE tap's gradient term counts the tap twice (coef = 2 / (nl half) on a node with one tap);
  B  ONE tap's distance launch reads the pred half as its own target (that tap contributes neither value nor gradient).
Both stay inside the end-to-end bounds -- the bf16-autocast gradient is itself ~0.14 rel-L2 off, so the gradient bound is ~0.3,
while one of 16 taps carries at most 0.16 of the gradient; the deepest tap carries 0.0014 of the MSE value, below 2^-8 -- and
both fail the comparison of the launch they sit in.  (Under L1 the smallest tap carries 0.011 of the value: B would be visible
there, so MSE is what the demonstration uses; A is invisible under either.)
"""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from tests import loss_audit as A
from tests import train_audit as T
from tests.lpips_restatement import tap_distance
from tests.vgg_restatement import CONV_INDICES, Restatement, he_state_dict, smooth_volume, to_rgb

F64 = torch.float64
SRC = Path(__file__).resolve().parents[1] / "video-to-video-diffusion_amd"


def _bf16(t):
    return t.to(torch.bfloat16)


# ---- selections ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(6, 10), (3, 5), (5, 4), (2, 2)])
def test_max_pool_references_route_like_torch_with_ties(h, w):
    """half-integer values: most windows hold equal maxima; forward = torch's values, backward = torch's routing (the first
    maximum in (h, w) row-major order), an odd last row / column left out and given a zero gradient"""
    g = torch.Generator().manual_seed(3 + h * w)
    n, c = 3, 16
    x = (torch.randint(-3, 4, (n, c, h, w), generator=g).to(F64) / 2)
    gy = torch.randn((n, c, h // 2, w // 2), generator=g, dtype=F64)
    xr = x.clone().requires_grad_(True)
    ref = F.max_pool2d(xr, kernel_size=2, stride=2)
    ref.backward(gy)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    assert A.tie_fraction(nhwc(x)) > 0.2
    assert torch.equal(A.ref_maxpool2_fwd(nhwc(x)), nhwc(ref.detach()))
    assert torch.equal(A.ref_maxpool2_bwd(nhwc(x), nhwc(gy)), nhwc(xr.grad))
    # in bf16, as the audit uses them: the same selection, bit for bit
    xb, gb = _bf16(nhwc(x)), _bf16(nhwc(gy))
    assert A.cmp_same(A.ref_maxpool2_fwd(xb), _bf16(nhwc(ref.detach())))["ok"]
    xq = xb.to(F64).permute(0, 3, 1, 2).requires_grad_(True)
    F.max_pool2d(xq, kernel_size=2, stride=2).backward(gb.to(F64).permute(0, 3, 1, 2))
    assert A.cmp_same(A.ref_maxpool2_bwd(xb, gb), _bf16(nhwc(xq.grad)))["ok"]


def test_max_pool_reference_keeps_the_first_of_two_zeros():
    """+0 before -0 and -0 before +0: equal values, different bits -- the first one's bits are the result"""
    x = torch.tensor([[0.0, -0.0], [-0.0, 0.0]], dtype=torch.bfloat16).view(1, 2, 2, 1)
    y = A.ref_maxpool2_fwd(x)
    assert y.view(torch.int16).item() == 0
    y = A.ref_maxpool2_fwd(-x)
    assert y.view(torch.int16).item() == torch.tensor(-0.0, dtype=torch.bfloat16).view(torch.int16).item()


def test_relu_reference_is_the_sign_bit_rule():
    x = torch.tensor([1.5, -1.5, 0.0, -0.0, float("inf"), float("-inf")], dtype=torch.bfloat16)
    y = A.ref_relu(x)
    assert A.cmp_same(y, torch.tensor([1.5, 0.0, 0.0, 0.0, float("inf"), 0.0], dtype=torch.bfloat16))["ok"]


# ---- distances -----------------------------------------------------------------------------------------------------------------
def test_distance_references_against_torch():
    g = torch.Generator().manual_seed(5)
    p, t = torch.randn((3, 6, 10, 64), generator=g, dtype=F64), torch.randn((3, 6, 10, 64), generator=g, dtype=F64)
    assert torch.allclose(A.ref_feat_sum(p, t, 0), F.l1_loss(p, t) * p.numel(), rtol=1e-13)
    assert torch.allclose(A.ref_feat_sum(p, t, 1), F.mse_loss(p, t) * p.numel(), rtol=1e-13)
    y, tt = torch.relu(p), torch.relu(t)
    w = torch.rand(64, generator=g, dtype=F64)
    w[::7] = 0.0
    sums, kappa = A.ref_lpips_sums(y.reshape(3, 60, 64), tt.reshape(3, 60, 64), w)
    want = tap_distance(y.permute(0, 3, 1, 2), tt.permute(0, 3, 1, 2), w.view(1, 64, 1, 1)) * 60
    assert torch.allclose(sums, want, rtol=1e-13)
    assert float(kappa.min()) >= 1.0 - 1e-12            # |u| + |v| >= |u - v|
    # the finalizes from partial sums laid out as the kernels lay them out
    blocks = 4
    counts = torch.tensor([640, 160], dtype=torch.int64)
    parts = torch.rand(2 * blocks, generator=g, dtype=F64)
    out = A.ref_feat_finalize(parts, counts, blocks)
    means = torch.stack([parts[:4].sum() / 640, parts[4:].sum() / 160])
    assert torch.allclose(out, torch.cat([means.mean().view(1), means]), rtol=1e-15)
    parts = torch.rand(2 * 3 * blocks, generator=g, dtype=F64)           # [tap][image][block]
    out = A.ref_lpips_finalize(parts, counts, 3, blocks)
    d = parts.view(2, 3, blocks).sum(2) / counts.to(F64).view(2, 1)
    assert torch.allclose(out[:3], d.sum(0), rtol=1e-15) and torch.allclose(out[3:], d.mean(1), rtol=1e-15)


# ---- the gradient passes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_kind,relu,with_g", [(1, 1, True), (2, 1, True), (0, 1, True), (1, 0, False), (2, 0, True), (2, 1, False)])
def test_feature_gradient_reference_against_autograd(loss_kind, relu, with_g):
    g = torch.Generator().manual_seed(7 + loss_kind)
    shape = (3, 5, 4, 16)
    z = torch.randn(shape, generator=g, dtype=F64).requires_grad_(True)
    t = torch.randn(shape, generator=g, dtype=F64)
    gin = torch.randn(shape, generator=g, dtype=F64) * 1e-3 if with_g else None
    nl, gl = 5, 0.75
    y = torch.relu(z) if relu else z
    loss = {0: 0.0 * y.sum(), 1: F.l1_loss(y, t), 2: F.mse_loss(y, t)}[loss_kind] / nl * gl
    if with_g:
        loss = loss + (gin * y).sum()
    loss.backward()
    ref, need = A.ref_feat_grad(gin, y.detach(), t, 1.0 / (nl * t.numel()), gl, loss_kind, relu)
    assert torch.allclose(ref, z.grad, rtol=1e-12, atol=1e-18)
    assert float(need.max()) <= 1e-6 * float((ref.abs() + (gin.abs() if with_g else 0)).max() + 1.0)


@pytest.mark.parametrize("c,with_g", [(64, True), (128, False)])
def test_lpips_gradient_reference_against_autograd(c, with_g):
    g = torch.Generator().manual_seed(c)
    n, pos = 3, 12
    z = torch.randn((n, pos, c), generator=g, dtype=F64)
    z[1, 3] = -1.0                                                  # a row that the ReLU zeroes entirely: a = 0
    z = z.requires_grad_(True)
    t = torch.relu(torch.randn((n, pos, c), generator=g, dtype=F64))
    w = torch.rand(c, generator=g, dtype=F64) * (4.0 / c)
    w[::7] = 0.0
    gl = torch.tensor([0.75, 0.0, -1.25], dtype=F64)
    gin = torch.randn((n, pos, c), generator=g, dtype=F64) * 1e-3 if with_g else None
    y = torch.relu(z)
    nchw = lambda v: v.permute(0, 2, 1).unsqueeze(-1)
    loss = (tap_distance(nchw(y), nchw(t), w.view(1, c, 1, 1)) * gl).sum()
    if with_g:
        loss = loss + (gin * y).sum()
    loss.backward()
    ref, need = A.ref_lpips_grad(gin, y.detach(), t, w, gl, pos)
    assert torch.isfinite(ref).all() and torch.isfinite(need).all()
    assert torch.allclose(ref, z.grad, rtol=1e-9, atol=1e-16)
    assert float(ref[1, 3].abs().max()) == 0.0 and (float(ref[1].abs().max()) == 0.0 or with_g)
    # the fp32 chain is far below one bf16 ulp of the result's scale: the plain one-ulp bound applies on operands like these
    assert float(need.max()) <= T.BF16_FLOOR * float(ref.pow(2).mean().sqrt()) * 10


def test_elementwise_bound_takes_the_fp32_chain_only_outside_the_operand_range():
    """_bf16_elem: inside the range -- need below the rms floor everywhere -- it is cmp_bf16 itself; a term far above the
    result's rms (g_in and the loss term cancelling) brings `need` in as the per-element extra"""
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(4096, generator=g, dtype=F64)
    out = _bf16(ref)
    small = torch.full_like(ref, 1e-9)
    r = A._bf16_elem(out, ref, small)
    assert r["ok"] and r["extra"] == "-" and r["ulps"] == T.cmp_bf16(out, ref)["ulps"]
    big = small.clone()
    big[7] = 1e-3
    r = A._bf16_elem(out, ref, big)
    assert r["ok"] and r["extra"] == "fp32 chain"
    off = out.clone()
    off[9] = (off[9].double() * (1 + 2.0 ** -6)).to(torch.bfloat16)
    assert not A._bf16_elem(off, ref, small)["ok"] and not A._bf16_elem(off, ref, big)["ok"]


# ---- what the end-to-end bounds cannot see -------------------------------------------------------------------------------------
def test_planted_plumbing_errors_pass_end_to_end_and_fail_their_launch():
    torch.manual_seed(0)
    layers, nl = tuple(CONV_INDICES), len(CONV_INDICES)
    sd = he_state_dict(1234, upto=36)
    shape = (1, 1, 2, 32, 32)
    pred, target = smooth_volume(shape, 101), smooth_volume(shape, 102)
    r64 = Restatement(sd, layers, False, 1.0, F64)
    p = pred.double().clone().requires_grad_(True)
    with torch.no_grad():
        tf = r64.features(to_rgb(target.double(), 1.0))
    pf = r64.features(to_rgb(p, 1.0))
    terms = [F.mse_loss(a, b) for a, b in zip(pf, tf)]
    v64 = sum(terms) / nl
    g64 = torch.autograd.grad(v64, p, retain_graph=True)[0]
    g_tap = [torch.autograd.grad(t / nl, p, retain_graph=True)[0] for t in terms]
    # the yardstick: the same restatement under bf16 autocast
    rac = Restatement(sd, layers, False, 1.0, torch.float32)
    q = pred.clone().requires_grad_(True)
    vac = rac(q, target, autocast=True)
    vac.backward()
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())
    v64, vac = v64.detach(), vac.detach()
    v_bound = 2 * abs(float(vac) - float(v64)) / float(v64) + 2.0 ** -8
    g_bound = 2 * rel(q.grad, g64) + 2e-2
    # A: tap kA counted twice in its gradient coefficient (the value is untouched)
    kA = 4
    gA = g64 + g_tap[kA]
    # B: the deepest tap reads pred as its own target
    kB = nl - 1
    gB, share_b = g64 - g_tap[kB], float((terms[kB] / nl / v64).detach())           # the value drops by the tap's share
    print(f"bounds: value {v_bound:.3e} gradient {g_bound:.3e}; A: gradient off by {rel(gA, g64):.3e}; "
          f"B: value off by {share_b:.3e}, gradient by {rel(gB, g64):.3e}")
    assert rel(gA, g64) > 0.05 and rel(gA, g64) <= g_bound                                   # a real error, unseen
    assert 1e-3 < share_b <= v_bound and rel(gB, g64) <= g_bound
    # ... and at their launches: the operands are the bf16 features the launches would read (images, h, w, c)
    feat = lambda k: (_bf16(pf[k].detach().permute(0, 2, 3, 1)), _bf16(tf[k].permute(0, 2, 3, 1)))
    y, t = feat(kA)
    half = y.numel()
    good, need = A.ref_feat_grad(None, torch.relu(y), torch.relu(t), 1.0 / (nl * half), 1.0, 2, 1)
    twice, _ = A.ref_feat_grad(None, torch.relu(y), torch.relu(t), 2.0 / (nl * half), 1.0, 2, 1)
    assert A._bf16_elem(_bf16(good), good, need)["ok"] and not A._bf16_elem(_bf16(twice), good, need)["ok"]
    y, t = feat(kB)
    assert A.cmp_rel(A.ref_feat_sum(y, t, 1), A.ref_feat_sum(y, t, 1), A.SUM_REL)["ok"]
    assert not A.cmp_rel(A.ref_feat_sum(y, y, 1), A.ref_feat_sum(y, t, 1), A.SUM_REL)["ok"]
    none, _ = A.ref_feat_grad(None, y, y, 1.0 / (nl * y.numel()), 1.0, 2, 0)
    good, need = A.ref_feat_grad(None, y, t, 1.0 / (nl * y.numel()), 1.0, 2, 0)
    assert not A._bf16_elem(_bf16(none), good, need)["ok"]


# ---- every launch has a record, every kind a reference ------------------------------------------------------------------------------
def test_every_loss_program_launch_carries_a_record_with_a_reference():
    assert set(A.REFS) == set(A._INPUTS)
    text = (SRC / "vgg_loss_engine.py").read_text()
    kinds = set(re.findall(r'kind="([a-z0-9_.]+)"', text))
    known = set(A.REFS) | set(T._INPUTS)
    assert kinds and kinds <= known, kinds - known
    assert {"maxpool2_fwd", "relu", "feat_loss", "lpips_dist", "feat_loss_finalize", "lpips_finalize", "feat_grad_relu",
            "lpips_grad_relu", "maxpool2_bwd"} <= kinds
    # every _emit( call passes audit= (the calls end at the first line that closes their parenthesis)
    calls = [m.start() for m in re.finditer(r"self\._emit\(", text)]
    assert len(calls) >= 9
    for at in calls:
        depth, end = 0, at
        for end in range(at + len("self._emit"), len(text)):
            depth += {"(": 1, ")": -1}.get(text[end], 0)
            if depth == 0:
                break
        assert "audit=" in text[at:end], text[at:end][:80]
    # the decode-grad seam: a record of a kind this module knows, and no launch left that says it has none
    vae = (SRC / "vae_train_engine.py").read_text()
    assert '"kind": "seam.grad_z"' in vae and "no audit record" not in vae and "seam.grad_z" in A.REFS
    # the new kinds stay out of the two older tables (tests/test_host_fwd_audit.py pins those to four engine files)
    from tests import fwd_audit as FA
    assert not set(A.REFS) & (set(FA.REFS) | set(T._INPUTS))
