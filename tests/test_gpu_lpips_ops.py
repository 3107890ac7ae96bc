"""GPU: the single ops of the LPIPS distance (csrc/lpips.hip) against float64 from their own bf16 operands.

Operands are made in bf16 and are exactly what the kernels read; the truth is tests/lpips_restatement.tap_distance (steps 3 and
4) and its autograd in float64.  Bounds:

  ctsi_lpips_dist_fwd + ctsi_lpips_finalize: 1e-5 relative per image.  From the source (lpips_dist_kernel): y^2 is exact in
    fp32 (8-bit significands); the row's sum of C squares is 7 sequential fmas and log2(C / 8) butterfly levels, <= 13 roundings
    of 2^-24 relative (all terms positive); sqrt halves that and adds 1/2, + eps, the reciprocal and the product y * ia add
    1/2 each: u and v carry delta <= 8.5 x 2^-24 = 5.1e-7 relative.  d = u - v then has |err| <= delta (|u| + |v|), and
    sum_c w d^2 an error <= 2 delta sum w |d| (|u| + |v|) + 10 x 2^-24 sum w d^2 (the product, the 8-term fma chain; fp64 from
    there on, one rounding to fp32 at the end).  By Cauchy-Schwarz the first term is <= 2 delta kappa sum w d^2 with
    kappa^2 = sum w (|u| + |v|)^2 / sum w d^2, a property of the OPERANDS: the test computes kappa in float64 and checks that
    2 delta kappa + 6e-7 stays below the 1e-5 it asserts (these rows give kappa 1.2 .. 2.7: at most 3.4e-6).
  ctsi_lpips_grad_relu_bwd: every element within tests/train_audit.cmp_bf16 -- one bf16 ulp + BF16_FLOOR x rms -- of float64.
    The kernel evaluates g + s (r ia - u (u . r) / a) in fp32 and rounds once (half an ulp); the fp32 chain leaves <= ~2e-6 of
    the LARGEST of the three terms, which the rms floor covers as long as no term exceeds ~5 rms where the result cancels to
    nothing: u, v <= 1 and w <= 4 / C bound the two loss terms by a few rms, and g is drawn at their rms.
"""
import ctypes as C

import pytest
import torch

from tests.helpers import bf16_round, rel_l2
from tests.lpips_restatement import SCALE, SHIFT, tap_distance
from tests.train_audit import cmp_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = 1e-5
DELTA = 8.5 * 2.0 ** -24
MIX = (0.0, 0.4, 0.7)
SHAPES = [(c, pos, n) for c in (64, 128, 256, 512) for pos in (1, 6, 35, 1024) for n in (1, 3)]


@pytest.fixture(scope="module")
def G():
    from tests import gpu_utils
    return gpu_utils


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _operands(c, pos, n, seed=0):
    """post-ReLU bf16 features (images, positions, c) and a non-negative head.  Image i's target is correlated with its pred
    by MIX[i], so the images' distances differ by construction (independent draws converge to one value at large sizes)."""
    g = torch.Generator().manual_seed(1000 * c + 10 * pos + n + seed)
    raw, noise = torch.randn(n, pos, c, generator=g), torch.randn(n, pos, c, generator=g)
    mix = torch.tensor(MIX[:n]).view(n, 1, 1)
    y = bf16_round(torch.relu(raw))
    t = bf16_round(torch.relu(mix * raw + (1 - mix ** 2).sqrt() * noise))
    w = torch.rand(c, generator=g) * (4.0 / c)
    w[::7] = 0.0
    return y, t, w


def _nchw(x):              # (n, pos, c) -> (n, c, pos, 1)
    return x.permute(0, 2, 1).unsqueeze(-1)


def _dev16(x):
    return x.to(device=DEV, dtype=torch.bfloat16).contiguous()


def _run_dist(G, taps):
    """taps: [(y, t, w)] with one image count -> (out[n], tap_means[taps]) of ctsi_lpips_dist_fwd per tap + one finalize"""
    ctx = G.ctx()
    n = taps[0][0].shape[0]
    blocks = ctx.lib.lpips_blocks()
    partials = torch.full((len(taps) * n * blocks,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    means = torch.full((len(taps),), float("nan"), dtype=torch.float32, device=DEV)
    cnt = torch.tensor([y.shape[1] for y, _, _ in taps], dtype=torch.int64, device=DEV)
    keep = []
    with ctx.scope():
        for l, (y, t, w) in enumerate(taps):
            yb, tb, wb = _dev16(y), _dev16(t), w.to(DEV)
            keep += [yb, tb, wb]
            ctx.lib.lpips_dist_fwd(_ptr(yb), _ptr(tb), _ptr(wb), n, y.shape[1], y.shape[2],
                                   C.c_void_p(partials.data_ptr() + 8 * l * n * blocks), ctx.sptr)
        ctx.lib.lpips_finalize(_ptr(partials), _ptr(cnt), len(taps), n, _ptr(out), _ptr(means), ctx.sptr)
    torch.cuda.synchronize()
    return out.double().cpu(), means.double().cpu()


def _kappa(y, t, w):
    y, t, w = y.double(), t.double(), w.double()
    u = y / (y.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    v = t / (t.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    return float(((w * (u + v) ** 2).sum((1, 2)) / (w * (u - v) ** 2).sum((1, 2))).sqrt().max())


@pytest.mark.parametrize("c,pos,n", SHAPES, ids=[f"c{c}_p{p}_n{n}" for c, p, n in SHAPES])
def test_distance_per_image_against_float64(G, c, pos, n):
    y, t, w = _operands(c, pos, n)
    want = tap_distance(_nchw(y.double()), _nchw(t.double()), w.double().view(1, c, 1, 1))
    got, means = _run_dist(G, [(y, t, w)])
    bound = 2 * DELTA * _kappa(y, t, w) + 6e-7
    err = float(((got - want).abs() / want).max())
    print(f"[c={c} pos={pos} n={n}] rel err {err:.3e}  derived worst case {bound:.3e}  values {want.tolist()}")
    assert bound <= FWD_TOL and float(want.min()) > 0.0
    assert err <= FWD_TOL
    assert abs(float(means[0]) - float(want.mean())) <= FWD_TOL * float(want.mean())
    if n > 1:                  # distinct images: a mix-up would show
        assert float((want - want.roll(1)).abs().min()) > 100 * FWD_TOL * float(want.max())


def test_finalize_sums_taps_per_image(G):
    taps = [_operands(64, 35, 3), _operands(512, 6, 3), _operands(128, 1, 3)]
    want = [tap_distance(_nchw(y.double()), _nchw(t.double()), w.double().view(1, -1, 1, 1)) for y, t, w in taps]
    got, means = _run_dist(G, taps)
    total = sum(want)
    assert float(((got - total).abs() / total).max()) <= FWD_TOL
    for l, v in enumerate(want):
        assert abs(float(means[l]) - float(v.mean())) <= FWD_TOL * float(v.mean())
    again, _ = _run_dist(G, taps)
    assert torch.equal(got, again)


def _grad_truth(y, t, w, go, g):
    z = y.double().clone().requires_grad_(True)           # y is post-ReLU: relu(z) = y, and its backward is the mask [y > 0]
    d = tap_distance(_nchw(torch.relu(z)), _nchw(t.double()), w.double().view(1, -1, 1, 1))
    (d * go.double()).sum().backward()
    return z.grad + (g.double() * (y > 0) if g is not None else 0.0)


def _run_grad(G, y, t, w, go, g, alias=False):
    ctx = G.ctx()
    n, pos, c = y.shape
    yb, tb, wb, gob = _dev16(y), _dev16(t), w.to(DEV), go.to(DEV)
    gb = _dev16(g) if g is not None else None
    out = gb if alias else torch.full((n, pos, c), float("nan"), dtype=torch.bfloat16, device=DEV)
    with ctx.scope():
        ctx.lib.lpips_grad_relu_bwd(_ptr(gb), _ptr(yb), _ptr(tb), _ptr(wb), _ptr(out), n, pos, c, _ptr(gob), ctx.sptr)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("c,pos,n", SHAPES, ids=[f"c{c}_p{p}_n{n}" for c, p, n in SHAPES])
def test_gradient_pass_against_float64(G, c, pos, n):
    """g_in NULL / present / aliased, a distinct upstream gradient per image"""
    y, t, w = _operands(c, pos, n, seed=5)
    go = torch.tensor([0.75, -1.25, 2.5][:n]) * pos
    term = _grad_truth(y, t, w, go, None)
    rms = float(term.pow(2).mean().sqrt())
    gen = torch.Generator().manual_seed(c + pos)
    g = bf16_round(torch.randn(n, pos, c, generator=gen) * rms)
    for mode in ("null", "present", "aliased"):
        gi = None if mode == "null" else g
        want = term if gi is None else _grad_truth(y, t, w, go, gi)
        got = _run_grad(G, y, t, w, go, gi, alias=mode == "aliased")
        r = cmp_bf16(got, want)
        print(f"[c={c} pos={pos} n={n} g_in {mode}] ulps {r['ulps']:.3f} rel-L2 {r['rel_l2']:.3e}")
        assert r["ok"], (mode, r)
        assert float(got.double()[y <= 0].abs().max()) == 0.0
        if mode == "present":
            first = got
        if mode == "aliased":
            assert torch.equal(got, first)


@pytest.mark.parametrize("c", [64, 512])
def test_zero_rows_stay_finite(G, c):
    """one all-zero pred row, one all-zero target row, one row zero in both; with and without an incoming gradient"""
    y, t, w = _operands(c, 6, 2, seed=9)
    y[0, 1] = 0.0
    t[0, 2] = 0.0
    y[1, 4] = 0.0
    t[1, 4] = 0.0
    go = torch.tensor([3.0, -2.0]) * 6
    want_d = tap_distance(_nchw(y.double()), _nchw(t.double()), w.double().view(1, c, 1, 1))
    got_d, _ = _run_dist(G, [(y, t, w)])
    assert torch.isfinite(got_d).all() and float(((got_d - want_d).abs() / want_d).max()) <= FWD_TOL
    g = bf16_round(torch.randn(2, 6, c, generator=torch.Generator().manual_seed(1)) * 1e-3)
    for gi in (None, g):
        want = _grad_truth(y, t, w, go, gi)
        got = _run_grad(G, y, t, w, go, gi)
        assert torch.isfinite(got.float()).all() and torch.isfinite(want).all()
        assert float(got[0, 1].float().abs().max()) == 0.0 and float(got[1, 4].float().abs().max()) == 0.0
        assert float(got[0, 2].float().abs().max()) > 0.0
        assert cmp_bf16(got, want)["ok"]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("normalize", [0, 1])
def test_prep_and_its_backward(G, c, normalize):
    n, h, w = 3, 16, 24
    gen = torch.Generator().manual_seed(5 + c)
    x = torch.rand(n, c, h, w, generator=gen) if normalize else torch.rand(n, c, h, w, generator=gen) * 2 - 1
    g = bf16_round(torch.randn(n, 8, h, w, generator=gen))
    xd = x.to(DEV)
    img = torch.full((n, h, w, 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    grad = torch.full((n, c, h, w), float("nan"), dtype=torch.float32, device=DEV)
    gb = g.permute(0, 2, 3, 1).contiguous().to(device=DEV, dtype=torch.bfloat16)
    ctx = G.ctx()
    with ctx.scope():
        ctx.lib.lpips_prep(_ptr(xd), _ptr(img), n, c, h, w, normalize, ctx.sptr)
        ctx.lib.lpips_prep_bwd(_ptr(gb), _ptr(grad), n, c, h, w, normalize, ctx.sptr)
    torch.cuda.synchronize()

    def formula(v):
        v = 2 * v - 1 if normalize else v
        v = v.repeat(1, 3, 1, 1) if c == 1 else v
        shift = torch.tensor(SHIFT, dtype=v.dtype).view(1, 3, 1, 1)
        scale = torch.tensor(SCALE, dtype=v.dtype).view(1, 3, 1, 1)
        return (v - shift) / scale

    # forward: the fp32 formula rounded to bf16 once, channels 3-7 zero
    got = img.float().cpu().permute(0, 3, 1, 2)
    assert torch.equal(got[:, :3], formula(x).to(torch.bfloat16).float()) and float(got[:, 3:].abs().max()) == 0.0
    # backward: autograd of the same formula in float64 (C = 1: the three channel gradients summed)
    xr = x.double().requires_grad_(True)
    formula(xr).backward(g[:, :3].double())
    assert rel_l2(grad.cpu(), xr.grad) < 1e-6 and float(grad.abs().min()) > 0.0
