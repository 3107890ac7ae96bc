"""GPU: the learned reverse variance and the strided ancestral sampler (csrc/learned_sigma.hip,
learned_sigma.py) -- the kernels against float64, the 2L-channel head through the step programs, the analytic model, one
training step against the fp32 oracle, poison-and-guard, and the three inference precisions.  Every figure is printed before
it is asserted.  None of this exists on the parent: it has no 'ddpm_spaced' sampler and no learn_sigma argument."""
import contextlib
import ctypes as C
import importlib
import json
import math
import os

import pytest
import torch

from oracle import ref_ops as R
from tests import learned_sigma_restatement as LR
from tests import poison as PZ
from tests import train_audit as TA
from tests.helpers import TINY_UNET, formula_input, formula_noise, load_formula, rel_l2, unet_cfg
from tests.x3_restatement import x3_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = importlib.import_module("video-to-video-diffusion_amd.engine")
E32 = importlib.import_module("video-to-video-diffusion_amd.engine_f32")
EX = importlib.import_module("video-to-video-diffusion_amd.engine_x3")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
LS = importlib.import_module("video-to-video-diffusion_amd.learned_sigma")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
U24 = 2.0 ** -24
F64 = torch.float64
V = "v_prediction"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resblock_default_launches.json")
SHAPES = [(2, 8, 4, 8, 8), (1, 3, 5, 7, 9)]          # the second: no 16-byte path


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _nd(x):
    """NCDHW -> contiguous NDHWC."""
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _nc(x):
    """NDHWC -> contiguous NCDHW."""
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _learned(pkg, **kw):
    g = pkg.GaussianDiffusion(**kw)
    g.var_type = "learned_range"
    return g


def _noise_fn(i, shape):
    return _randn(shape, 1000 + i).to(DEV)


@pytest.fixture(scope="module")
def wide_unet(pkg):
    """The tiny U-Net with the 2L-channel head."""
    un = pkg.UNet3D(**TINY_UNET, learn_sigma=True)
    load_formula(un, 8)
    yield un.to(DEV)
    un.invalidate_engine_cache()


class _precision:
    def __init__(self, unet, p):
        self.unet, self.p = unet, p

    def __enter__(self):
        self.prev = self.unet.inference_precision
        self.unet.inference_precision = self.p

    def __exit__(self, *exc):
        self.unet.inference_precision = self.prev


# ---------------------------------------------------------------------------------------------------------------------
# 1. ctsi_sigma_split
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", ["half", "all", "none"])
@pytest.mark.parametrize("shape", SHAPES)
def test_sigma_split_moves_bits(shape, keep):
    """A pure copy: eps holds channels [0, L) of every row, vraw channels [L, 2L) of rows [0, n_keep), bit for bit; what lies
    behind the kept rows is not written, and out2 is read only."""
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    n, Lc, d, h, w = shape
    n = 2 * n                                            # network rows (a guided batch)
    n_keep = dict(half=n // 2, all=n, none=0)[keep]
    out2 = _randn((n, d, h, w, 2 * Lc), 3)
    out2[0, 0, 0, 0, :4] = torch.tensor([0.0, -0.0, float("nan"), float("inf")])[:min(4, 2 * Lc)]
    o2 = out2.to(DEV)
    eps = torch.full((n, d, h, w, Lc), 7.0, device=DEV)
    vraw = None if keep == "none" else torch.full((n, d, h, w, Lc), 9.0, device=DEV)
    with ctx.scope():
        lib.sigma_split(_ptr(o2), _ptr(eps), _ptr(vraw), n, n_keep, Lc, d, h, w, ctx.sptr)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(o2.cpu()), bits(out2))
    assert torch.equal(bits(eps.cpu()), bits(out2[..., :Lc]))
    if vraw is not None:
        assert torch.equal(bits(vraw[:n_keep].cpu()), bits(out2[:n_keep, ..., Lc:]))
        assert bool((vraw[n_keep:] == 9.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 2. ctsi_ddpm_lv_step against float64
# ---------------------------------------------------------------------------------------------------------------------
def _lv_case(shape, with_v, with_noise, clip, last, f32_zin, seed=0):
    """One launch of the step through a non-zero step_ptr past a decoy row; returns what the checks need."""
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    n, Lc, d, h, w = shape
    g = importlib.import_module("video-to-video-diffusion_amd").GaussianDiffusion()
    chain = [999, 700, 300, 0]
    rows = LS.respaced_ddpm_rows(g, chain, clip)
    live = rows[3 if last else 1].clone()
    table = torch.stack([torch.full((8,), 5.0), live]).to(DEV).contiguous()            # row 0: a decoy, never read
    step = torch.ones(1, dtype=torch.int32, device=DEV)
    z = _randn((n, d, h, w, Lc), 11 + seed, 0.8)
    eps = _randn((n, d, h, w, Lc), 12 + seed)
    vraw = (torch.rand((n, d, h, w, Lc), generator=torch.Generator().manual_seed(13 + seed)) * 3.0 - 1.5) if with_v else None
    noise = _randn((n, Lc, d, h, w), 14 + seed) if with_noise else None
    c_total, c_off = (Lc, 0) if f32_zin else (2 * Lc, 0)
    zin = torch.full((n, d, h, w, c_total), 3.0, dtype=torch.float32 if f32_zin else torch.bfloat16, device=DEV)
    zd, ed = z.to(DEV), eps.to(DEV)
    vd, nd = (None if vraw is None else vraw.to(DEV)), (None if noise is None else noise.to(DEV))
    fn = lib.ddpm_lv_step_f32 if f32_zin else lib.ddpm_lv_step
    with ctx.scope():
        fn(_ptr(zd), _ptr(ed), _ptr(vd), _ptr(nd), _ptr(zin), c_total, c_off, _ptr(table), _ptr(step), n, Lc, d, h, w, ctx.sptr)
    torch.cuda.synchronize()
    assert torch.equal(ed.cpu(), eps) and (vd is None or torch.equal(vd.cpu(), vraw))        # read only
    nz_nd = None if noise is None else _nd(noise)
    ref, lv, bound = LR.step(z, eps, vraw, nz_nd, live.double())
    return dict(got=zd.cpu(), zin=zin.cpu(), ref=ref, bound=bound, live=live, c_total=c_total, Lc=Lc, vraw=vraw)


@pytest.mark.parametrize("f32_zin", [False, True])
@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("with_v", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_lv_step_against_float64(shape, with_v, with_noise, clip, last, f32_zin):
    """|got - ref| <= bound elementwise, the bound counted operation by operation in learned_sigma_restatement.step (the rule of
    test_gpu_cfg.test_combine_against_float64): three roundings for z0, three for the mean plus z0's inherited error, and for
    the noise term the relative error of the scale s exp(f (c4 - c5) / 2), s = the row's fixed-small scale -- an absolute error
    delta in the exp argument costs a relative delta in the exp; the argument carries 4 u |f (c4 - c5) / 2|, the device exp 2 ulp,
    the two products and the sum 3 more.  v spans [-1.5, 1.5]: f outside [0, 1] is not clamped.  At the clamp's edges the reference's z0 and the
    kernel's may sit on different sides of +-1 by a rounding: those elements are bounded by the unclamped error, which the bound
    carries (the clamp is 1-Lipschitz).  zin holds the same values (bf16-rounded in the bf16 engine's slice)."""
    r = _lv_case(shape, with_v, with_noise, clip, last, f32_zin)
    err = (r["got"].double() - r["ref"]).abs()
    used = float((err / r["bound"].clamp_min(1e-300)).max())
    print(f"lv_step {shape} v={with_v} noise={with_noise} clip={clip} last={last} f32_zin={f32_zin}: worst |err| / bound = "
          f"{used:.3f}; max |z'| {float(r['ref'].abs().max()):.3f}; row {[round(float(x), 5) for x in r['live']]}")
    assert torch.isfinite(r["got"]).all()
    assert (err <= r["bound"]).all(), used
    if with_v:
        f = (r["vraw"] + 1.0) / 2.0
        assert float(f.min()) < 0.0 and float(f.max()) > 1.0
    Lc = r["Lc"]
    zin = r["zin"]
    want = r["got"] if f32_zin else r["got"].to(torch.bfloat16)
    assert torch.equal(zin[..., :Lc].contiguous().view(torch.int16 if not f32_zin else torch.int32),
                       want.contiguous().view(torch.int16 if not f32_zin else torch.int32))
    if r["c_total"] > Lc:
        assert bool((zin[..., Lc:].float() == 3.0).all())                   # the conditioning half is not touched
    if last and with_noise:        # the last row draws no noise: the update is the mean
        r0 = _lv_case(shape, with_v, False, clip, last, f32_zin)
        assert torch.equal(r0["got"].view(torch.int32), r["got"].view(torch.int32))


@pytest.mark.parametrize("f32_zin", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_lv_step_without_variance_channels_reproduces_ddpm_step_bits(pkg, shape, f32_zin):
    """vraw = NULL on the full-length chain's rows (read from the registered buffers, clip 1): the bits of ctsi_ddpm_step on the
    parent's rows, at EVERY row -- the noise scale in the row is the same fp32 number and the mean is written with the same
    roundings.  All 1000 rows sit in the two tables; the launches walk step_ptr over a spread of them that holds both ends,
    and the rows themselves are compared over the whole chain."""
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    g = pkg.GaussianDiffusion()
    full = list(reversed(range(1000)))
    lv_rows, parent = LS.respaced_ddpm_rows(g, full, True), g.ddpm_coef_rows(full)
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(lv_rows[:, :4]), bits(parent[:, :4])) and torch.equal(bits(lv_rows[:, 6]), bits(parent[:, 4]))
    n, Lc, d, h, w = shape
    c_total = Lc if f32_zin else 2 * Lc
    picks = list(range(0, 1000, 37)) + [1, 998, 999]                              # (row 999 is t = 0: no noise)
    z, eps, noise = _randn((n, d, h, w, Lc), 21, 0.8), _randn((n, d, h, w, Lc), 22), _randn((n, Lc, d, h, w), 23)
    worst = 0
    for j in picks:
        outs = []
        for entry, rows in (("ddpm_step", parent), ("ddpm_lv_step", lv_rows)):
            zd, ed, nd = z.to(DEV), eps.to(DEV), noise.to(DEV)
            zin = torch.zeros((n, d, h, w, c_total), dtype=torch.float32 if f32_zin else torch.bfloat16, device=DEV)
            table, step = rows.to(DEV).contiguous(), torch.full((1,), j, dtype=torch.int32, device=DEV)
            fn = getattr(lib, entry + ("_f32" if f32_zin else ""))
            extra = (None,) if entry == "ddpm_lv_step" else ()
            with ctx.scope():
                fn(_ptr(zd), _ptr(ed), *extra, _ptr(nd), _ptr(zin), c_total, 0, _ptr(table), _ptr(step), n, Lc, d, h, w, ctx.sptr)
            torch.cuda.synchronize()
            outs.append((zd.cpu(), zin.cpu().float()))
        bad = int((bits(outs[0][0]) != bits(outs[1][0])).sum())
        worst = max(worst, bad)
        if bad:
            print(f"  t = {full[j]}: elements whose bits differ from ctsi_ddpm_step's: {bad} of {outs[0][0].numel()}")
        assert torch.equal(outs[0][1], outs[1][1])
    print(f"lv_step vs ddpm_step {shape} f32_zin={f32_zin}: {len(picks)} rows, most differing elements at any row: {worst}")
    assert worst == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. the hybrid loss
# ---------------------------------------------------------------------------------------------------------------------
MASKS = {"nomask": None, "equal": torch.tensor([[[1., 0., 1., 1.]], [[0., 1., 1., 1.]]]),
         "unequal": torch.tensor([[[1., 1., 1., 1.]], [[1., 0., 0., 1.]]])}
T_LOSS = torch.tensor([0, 640])                       # the Gaussian NLL branch and the KL branch in one batch
LOSS_SHAPES = SHAPES + [(2, 3, 5, 7, 9)]              # the third: both branches in one batch where there is no 16-byte path


def _loss_case(pkg, v_pred, tag, shape):
    g = pkg.GaussianDiffusion(prediction_type=V if v_pred else "epsilon")
    g.var_type = "learned_range"
    n, Lc, d, h, w = shape
    t = T_LOSS if n > 1 else T_LOSS[1:]               # (a single sample takes the KL branch)
    z0, noise = formula_input(shape, 31), formula_noise(-1, shape)
    a = g.sqrt_alphas_cumprod[t].view(-1, 1, 1, 1, 1)
    s = g.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1, 1)
    target = a * noise - s * z0 if v_pred else noise
    pred = target + 0.3 * _randn(shape, 41)                                     # a prediction with an error, as in training
    vch = torch.rand(shape, generator=torch.Generator().manual_seed(42)) * 3.0 - 1.5
    pred2 = torch.cat([pred, vch], 1)
    mask = MASKS[tag]
    if mask is not None:
        mask = mask[:n, :, :d] if d <= 4 else torch.cat([mask[:n], mask[:n, :, :d - 4]], 2)
    weight = g._snr_weight(t)
    cn, me, pooled = LR.count_norm(mask, shape)
    norm = ((weight.double().mean().expand(n) if pooled else weight.double()) * cn).float()
    norm_vb = (cn * (g.timesteps / 1000.0) / math.log(2.0)).float()
    return dict(g=g, t=t, z0=z0, noise=noise, pred2=pred2, mask=mask, me=me, weight=weight, norm=norm, norm_vb=norm_vb)


def _run_loss(c, v_pred, shape, bwd_stride=None, gscale=None):
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    n, Lc, d, h, w = shape
    sched = LS.loss_schedule_rows(c["g"]).to(DEV).contiguous()
    p2 = _nd(c["pred2"]).to(DEV)
    z0, nz, t = c["z0"].to(DEV), c["noise"].to(DEV), c["t"].to(torch.int32).to(DEV)
    m = None if c["mask"] is None else c["mask"].expand(n, Lc, d).contiguous().to(DEV)
    norm, nvb = c["norm"].to(DEV), c["norm_vb"].to(DEV)
    head = (_ptr(p2), _ptr(z0), _ptr(nz), _ptr(t), _ptr(sched), int(sched.shape[0]), int(v_pred), _ptr(m), _ptr(norm), _ptr(nvb))
    if bwd_stride is None:
        ws = torch.empty(lib.hybrid_loss_workspace_doubles(n), dtype=torch.float64, device=DEV)
        out = torch.zeros(3 + 2 * n, device=DEV)
        with ctx.scope():
            lib.hybrid_loss_fwd(*head, n, Lc, d, h, w, _ptr(ws), _ptr(out), ctx.sptr)
        torch.cuda.synchronize()
        return out.cpu()
    gs = None if gscale is None else torch.tensor([gscale], device=DEV)
    dp = torch.full((n, d, h, w, bwd_stride), 7.0, dtype=torch.bfloat16, device=DEV)
    with ctx.scope():
        lib.hybrid_loss_bwd(*head, _ptr(gs), n, Lc, d, h, w, _ptr(dp), bwd_stride, ctx.sptr)
    torch.cuda.synchronize()
    return dp.cpu()


@pytest.mark.parametrize("tag", ["nomask", "equal", "unequal"])
@pytest.mark.parametrize("v_pred", [False, True])
@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_hybrid_loss_forward_against_float64(pkg, shape, v_pred, tag):
    """{total, mse, vb} and the per-sample sums against the float64 restatement.  The device adds fp64 partials of fp32 element
    terms, so the error of a sum is the sum of its elements' errors.  Per element, counting fp32 roundings u = 2^-24 on the
    magnitude each acts on, and carrying every inherited error through (twice the count is allowed: fused and unfused
    multiply-adds round differently):
      target (v form) a noise - s z0: 3 u (|a noise| + |s z0|);  dp = p - target: that + u |dp|;  dp^2: 2 |dp| e + e^2 + u dp^2
      z0_pred: 4 u (|z_t| + |s p|) / a  |  4 u (|a z_t| + |s p|)     (z_t itself is two products and a sum of O(1) terms)
      q = c1 (z0 - z0_pred) (t > 0) or z0 - c1 z0_pred - c2 z_t (t = 0): c1 e(z0_pred) + 4 u (|z0| + |c1 z0_pred| + |c2 z_t|)
      lv = f c4 + (1 - f) c5: e_lv = 4 u (|f c4| + |(1 - f) c5|) + u |lv| absolute; an exp of it: relative e_lv + 3 u
      q^2 e^-lv: e^-lv (2 |q| e_q + e_q^2) + q^2 e^-lv (e_lv + 5 u)
      t > 0: (lv - c5): e_lv + u |lv - c5|;  (e^(c5 - lv) - 1): e^(c5 - lv) (e_lv + u |c5 - lv| + 3 u) + u |e^(c5 - lv) - 1|
      t = 0: ln 2 pi + lv: e_lv + u (ln 2 pi + |lv|)
      the three-term sum and the factor 1/2: 3 u of the magnitudes summed
    Added to the sums: u for each fp32 norm factor and the final fp32 store."""
    c = _loss_case(pkg, v_pred, tag, shape)
    n, Lc = shape[0], shape[1]
    out = _run_loss(c, v_pred, shape).double()
    g, t = c["g"], c["t"]
    ref = LR.hybrid_loss(c["pred2"].double(), c["z0"], c["noise"], t, g, c["weight"], c["mask"], v_pred)
    mse_e, vb_e = LR.hybrid_terms(c["pred2"].double(), c["z0"], c["noise"], t, LR.schedule64(g), v_pred)
    mag_mse, mag_vb = LR.hybrid_error_terms(c["pred2"], c["z0"], c["noise"], t, LR.schedule64(g), v_pred)      # the list above
    me = c["me"]
    S_ref, V_ref = (me * mse_e).reshape(n, -1).sum(1), (me * vb_e).reshape(n, -1).sum(1)
    S_b, V_b = (me * mag_mse).reshape(n, -1).sum(1), (me * mag_vb).reshape(n, -1).sum(1)
    norm, nvb = c["norm"].double(), c["norm_vb"].double()
    bd = LR.hybrid_sum_bounds(S_ref, V_ref, S_b, V_b, norm, nvb, ref["mse"], ref["vb"])
    checks = [("S_b", out[3:3 + n], S_ref, bd["S_b"]), ("V_b", out[3 + n:], V_ref, bd["V_b"]), ("mse", out[1], ref["mse"], bd["mse"]),
              ("vb", out[2], ref["vb"], bd["vb"]), ("total", out[0], ref["total"], bd["total"])]
    for name, got, want, bound in checks:
        err = (got - want).abs()
        print(f"hybrid fwd {shape} v_pred={v_pred} {tag} {name}: got {got.reshape(-1).tolist()} float64 {want.reshape(-1).tolist()} "
              f"worst |err| / bound {float((err / bound.clamp_min(1e-300)).max()):.3f} (bound / |value| "
              f"{float((bound / want.abs().clamp_min(1e-300)).max()):.1e})")
    for name, got, want, bound in checks:
        assert ((got - want).abs() <= bound).all(), name
    assert abs(float(out[0]) - float(out[1]) - float(out[2])) <= 2 * U24 * abs(float(out[0]))
    if tag == "unequal":
        nv = c["mask"].expand(n, Lc, shape[2]).reshape(n, -1).sum(1)
        assert n == 1 or not bool((nv == nv[0]).all())


@pytest.mark.parametrize("tag", ["nomask", "equal", "unequal"])
@pytest.mark.parametrize("v_pred", [False, True])
@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_hybrid_loss_backward_against_float64_autograd(pkg, shape, v_pred, tag):
    """d_pred against float64 autograd of the restatement's total, compared after bf16 rounding by the rule of the backward
    audit (tests/train_audit.cmp_bf16: one bf16 ulp per element plus its 1e-5 rms floor, rel-L2 4e-3 against bf16(ref)), each
    channel half on its own.  The padding channels of c_stride are zero; the bound sends nothing to the prediction channels."""
    c = _loss_case(pkg, v_pred, tag, shape)
    n, Lc, d, h, w = shape
    stride = (2 * Lc + 7) // 8 * 8 + 8                       # padded, and more than the next multiple of 8
    gscale = 0.75
    dp = _run_loss(c, v_pred, shape, bwd_stride=stride, gscale=gscale)
    p2 = c["pred2"].double().clone().requires_grad_(True)
    ref = LR.hybrid_loss(p2, c["z0"], c["noise"], c["t"], c["g"], c["weight"], c["mask"], v_pred)
    (gscale * ref["total"]).backward()
    want = p2.grad
    got = _nc(dp.float())                                    # (n, stride, d, h, w)
    assert bool((got[:, 2 * Lc:] == 0).all())                # the padding
    # the restatement uses float64 norm factors; the kernel's are their fp32 roundings: one more 2^-24, far below a bf16 ulp
    for name, lo, hi in (("prediction", 0, Lc), ("variance", Lc, 2 * Lc)):
        r = TA.cmp_bf16(got[:, lo:hi], want[:, lo:hi])
        print(f"hybrid bwd {shape} v_pred={v_pred} {tag} {name} channels: ulps {r['ulps']:.3f} rel-L2 vs bf16(ref) {r['rel_l2']:.2e} "
              f"max/max|ref| {r['max_rel']:.2e}; rms ref {float(want[:, lo:hi].pow(2).mean().sqrt()):.3e}")
        assert r["ok"], (name, r)
    assert float(want[:, Lc:].abs().max()) > 0
    # the MSE half is exactly the parent's expression: 2 norm mask (p - target); the bound adds nothing there
    mse_only = p2.detach().clone().requires_grad_(True)
    (gscale * LR.hybrid_loss(mse_only, c["z0"], c["noise"], c["t"], c["g"], c["weight"], c["mask"], v_pred)["mse"]).backward()
    assert torch.equal(mse_only.grad[:, :Lc], want[:, :Lc])
    if c["mask"] is not None:
        off = c["me"] == 0
        assert bool((got[:, :2 * Lc][off.repeat(1, 2, 1, 1, 1)] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. the network: one head conv, the split, the step programs
# ---------------------------------------------------------------------------------------------------------------------
NET_SHAPE = (1, 8, 4, 8, 8)


def _lv_program(pkg, g, unet, n, steps, clip=True, guided=False, precision="bf16"):
    """A separately built step program of kind 'ddpm_lv' (eager: no graph), scheduled for an N-step strided run."""
    sp = pkg.DDPMSampler(g, unet)
    kind, chain = sp.chain(steps, clip)
    plan = S._step_plan(g, kind, chain, 0.0, 2, S.lv_rows(g, chain, clip))
    ctx = E.Ctx.get(torch.device(DEV))
    cls = EX.unet_program(precision)
    nb = 2 * n if guided else n
    kw = dict(guided=True, rescale=False) if guided else {}
    if plan.pred is not None:
        kw["prediction"] = V
    prog = cls(ctx, unet, n, NET_SHAPE[2], NET_SHAPE[3], NET_SHAPE[4], (g.timesteps + 1) * nb, unet.attention_mode, **kw)
    prog.add_sampler_step(plan.kind, plan.with_noise, **(dict(learned_variance=True) if plan.learned else {}))
    return prog, plan, chain


def test_forward_returns_2L_channels_and_the_program_sees_the_packed_half(pkg, wide_unet):
    g = _learned(pkg)
    n, Lc, d, h, w = NET_SHAPE
    x, c = formula_input(NET_SHAPE, 10).to(DEV), formula_input(NET_SHAPE, 11).to(DEV)
    t = torch.tensor([500], device=DEV)
    out = wide_unet(x, t, c)
    assert out.shape == (n, 2 * Lc, d, h, w) and out.dtype == torch.float32 and torch.isfinite(out).all()
    # against the fp32 oracle with the 2L head: the bf16 engine's figure for this network (tests/test_gpu_network.py: 2e-2)
    sd = {k: v.detach().float() for k, v in wide_unet.state_dict().items()}
    ref = R.unet_forward(sd, unet_cfg(TINY_UNET), x, t, c, "")
    err_p, err_v = rel_l2(out[:, :Lc].cpu(), ref[:, :Lc].cpu()), rel_l2(out[:, Lc:].cpu(), ref[:, Lc:].cpu())
    print(f"learn_sigma forward vs fp32 oracle: prediction channels rel-L2 {err_p:.3e}, variance channels {err_v:.3e}")
    assert err_p < 2e-2 and err_v < 2e-2
    # the step program: ONE head conv of 2L channels, then the split; eps is the packed first half, vraw the second
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope():
        prog, plan, chain = _lv_program(pkg, g, wide_unet, 1, 10)
        names = [m[0] for m in prog.op_meta]
        assert names.count("conv_out") == 1 and names[prog.unet_op_count - 1] == "sigma.split"
        assert names[prog.unet_op_count:] == ["sampler.step", "sampler.advance"]
        assert prog.out2.shape == (1, d, h, w, 2 * Lc) and prog.vraw.shape == (1, d, h, w, Lc)
        prog.load_latents(x, c)
        prog.set_schedule([500], plan.coef[:1].to(DEV), None)
        for op in prog.ops[:prog.unet_op_count]:
            op()
        eps, vraw, full = prog.eps_ncdhw().cpu(), _nc(prog.vraw).cpu(), prog.out_ncdhw().cpu()
    torch.cuda.synchronize()
    assert torch.equal(full, out.cpu())                                       # the same launches as forward
    assert torch.equal(eps, out[:, :Lc].cpu()) and torch.equal(vraw, out[:, Lc:].cpu())


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_captured_equals_eager_and_repeats(pkg, wide_unet, precision):
    g = _learned(pkg)
    cond = formula_input(NET_SHAPE, 41).to(DEV)
    N = 4
    with _precision(wide_unet, precision):
        sp = pkg.DDPMSampler(g, wide_unet)
        runs = [sp.sample(NET_SHAPE, cond, DEV, progress=False, noise_fn=_noise_fn, num_inference_steps=N) for _ in range(2)]
        keys = [k for k in wide_unet._ctsi_programs if k[0] == "sampler" and "ddpm_lv" in k and precision in k]
        assert len(keys) == 1 and "learned" in keys[0]
        assert wide_unet._ctsi_programs[keys[0]].graph is not None
        ctx = E.Ctx.get(torch.device(DEV))
        with ctx.scope():
            prog, plan, chain = _lv_program(pkg, g, wide_unet, 1, N, precision=precision)
            prog.load_latents(_noise_fn(-1, NET_SHAPE), cond)
            prog.set_schedule(list(plan.t), plan.coef.to(DEV), plan.pred)
            for i in range(len(chain)):
                prog.noise.copy_(_noise_fn(i, NET_SHAPE))
                prog.run()
            eager = prog.z_ncdhw()
    torch.cuda.synchronize()
    assert len(chain) == N + 1 and torch.isfinite(runs[0]).all()
    assert torch.equal(runs[0], runs[1]) and torch.equal(eager, runs[0])


def test_batch_of_two_equals_two_single_runs(pkg, wide_unet):
    g = _learned(pkg)
    shape = (2,) + NET_SHAPE[1:]
    cond = formula_input(shape, 50).to(DEV)
    noises = {i: _randn(shape, 600 + i).to(DEV) for i in range(-1, 6)}
    with _precision(wide_unet, "fp32"):
        sp = pkg.DDPMSampler(g, wide_unet)
        both = sp.sample(shape, cond, DEV, progress=False, noise_fn=lambda i, s_: noises[i], num_inference_steps=4)
        one = [sp.sample(NET_SHAPE, cond[b:b + 1], DEV, progress=False, noise_fn=lambda i, s_, b=b: noises[i][b:b + 1],
                         num_inference_steps=4) for b in (0, 1)]
    for b in (0, 1):
        err = rel_l2(both[b:b + 1].cpu(), one[b].cpu())
        print(f"fp32 strided learned-variance run: sample {b} of a batch of two vs alone rel-L2 {err:.3e}")
        assert err < 1e-5          # the figure of test_gpu_cfg.test_batch_of_two_equals_two_single_guided_runs


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_guidance_scale_one_is_the_unguided_path(pkg, wide_unet, precision):
    g = _learned(pkg)
    cond = formula_input(NET_SHAPE, 43).to(DEV)
    with _precision(wide_unet, precision):
        sp = pkg.DDPMSampler(g, wide_unet)
        kw = dict(progress=False, noise_fn=_noise_fn, num_inference_steps=3)
        plain = sp.sample(NET_SHAPE, cond, DEV, **kw)
        before = set(wide_unet._ctsi_programs)
        one = sp.sample(NET_SHAPE, cond, DEV, guidance_scale=1.0, **kw)
    assert set(wide_unet._ctsi_programs) == before                      # no guided program was built
    assert torch.equal(plain, one)


def test_guidance_takes_the_variance_from_the_conditional_rows(pkg):
    """Scale 3.0, one step 999 -> 500 of a 2-step chain in fp32: the guided eps is eps_u + 3 (eps_c - eps_u) and the variance
    channels are the conditional evaluation's, checked against two separate forward passes combined on the host in float64.
    Yardstick: the fp32 mode's batch-invariance figure 1e-5 (a batch-2 evaluation against two batch-1 ones), times 1 + 2 |s|
    = 7 for the combination: 1e-4 with room.  Taking the variance from the unconditional rows instead must be at least 10
    times further away than what is measured, or the test could not tell."""
    g = _learned(pkg)
    n, Lc, d, h, w = NET_SHAPE
    # the formula weights make the variance channels depend on the conditioning only weakly: rows [L, 2L) of the head are scaled
    # by 30 here so that the two hypotheses lie well apart
    wide_unet = pkg.UNet3D(**TINY_UNET, learn_sigma=True)
    sd = load_formula(wide_unet, 8)
    sd["conv_out.2.weight"][Lc:] *= 30.0
    sd["conv_out.2.bias"][Lc:] *= 30.0
    wide_unet.load_state_dict(sd, strict=True)
    wide_unet.eval().to(DEV)
    cond = formula_input(NET_SHAPE, 44).to(DEV)
    z_T, nz = _noise_fn(-1, NET_SHAPE), _noise_fn(0, NET_SHAPE)
    s = 3.0
    with _precision(wide_unet, "fp32"):
        sp = pkg.DDPMSampler(g, wide_unet)
        traj = []
        sp.sample(NET_SHAPE, cond, DEV, progress=False, noise_fn=_noise_fn, num_inference_steps=2, guidance_scale=s,
                  trajectory=traj, clip_denoised=False)
        t = torch.tensor([999], device=DEV)
        out_c, out_u = wide_unet(z_T, t, cond), wide_unet(z_T, t, torch.zeros_like(cond))
        prog = [p for k, p in wide_unet._ctsi_programs.items() if k[0] == "sampler-cfg"]
        assert len(prog) == 1 and prog[0].vraw.shape[0] == 1 and prog[0].out2.shape[0] == 2
        names = [m[0] for m in prog[0].op_meta[prog[0].unet_op_count - 1:]]
        assert names == ["sigma.split", "cfg.combine", "sampler.step", "cfg.mirror", "sampler.advance"]
    torch.cuda.synchronize()
    kind, chain = sp.chain(2, False)
    assert chain == [999, 500, 0] and len(traj) == 3
    row = LR.rows64(g.alphas_cumprod, chain, False)[0]
    eps_g = out_u[:, :Lc].double() + s * (out_c[:, :Lc].double() - out_u[:, :Lc].double())
    want, _, _ = LR.step(z_T.cpu(), eps_g.cpu(), out_c[:, Lc:].cpu(), nz.cpu(), row)
    wrong, _, _ = LR.step(z_T.cpu(), eps_g.cpu(), out_u[:, Lc:].cpu(), nz.cpu(), row)
    err, err_wrong = rel_l2(traj[0].cpu(), want), rel_l2(traj[0].cpu(), wrong)
    dv = float((out_c[:, Lc:] - out_u[:, Lc:]).abs().max())
    print(f"guided learned-variance step: vs two passes with the conditional variance rel-L2 {err:.3e}; with the unconditional "
          f"variance {err_wrong:.3e}; max |v_c - v_u| {dv:.3e}")
    assert err < 1e-4 and err_wrong > 10 * err
    E.invalidate_engine_cache(wide_unet)


def test_deterministic_samplers_ignore_the_variance_channels(pkg, wide_unet):
    """DDIM (eta 0), DPM-Solver++ and Heun on a learn_sigma model equal the same samplers on a plain model holding the first L
    rows of the head: the packed eps is all they read."""
    g, gp = _learned(pkg), pkg.GaussianDiffusion()
    Lc = NET_SHAPE[1]
    plain = pkg.UNet3D(**TINY_UNET)
    sd = {k: v.clone() for k, v in wide_unet.state_dict().items()}
    sd["conv_out.2.weight"], sd["conv_out.2.bias"] = sd["conv_out.2.weight"][:Lc].clone(), sd["conv_out.2.bias"][:Lc].clone()
    plain.load_state_dict(sd, strict=True)
    plain.eval().to(DEV)
    cond, z_t = formula_input(NET_SHAPE, 46).to(DEV), _noise_fn(-1, NET_SHAPE)
    for name, cls in (("ddim", pkg.DDIMSampler), ("dpmpp", pkg.DPMSolverSampler), ("heun", pkg.HeunSampler)):
        a = cls(g, wide_unet).sample(NET_SHAPE, cond, 3, DEV, progress=False, z_init=z_t)
        b = cls(gp, plain).sample(NET_SHAPE, cond, 3, DEV, progress=False, z_init=z_t)
        err = rel_l2(a.cpu(), b.cpu())
        print(f"{name} on the learn_sigma model vs the plain model with the same prediction rows: rel-L2 {err:.3e}")
        # the head conv of 16 channels and the one of 8 are different launches of the same kernel family: the bf16 engine's
        # two evaluations of one network agree to its own rounding noise (the figure of test_gpu_network: 2e-2 against fp32)
        assert torch.isfinite(a).all() and err < 2e-2
    E.invalidate_engine_cache(plain)


def test_default_model_keeps_the_parents_launches_and_keys(pkg):
    """A default model: the launch names of forward, a sampler step and a training step are the fixture's (read, not edited),
    and its program cache keys carry nothing of this feature."""
    with open(GOLDEN) as f:
        want = json.load(f)
    un = pkg.UNet3D(**TINY_UNET)
    load_formula(un, 8)
    un.to(DEV)
    x, c = formula_input(NET_SHAPE, 10).to(DEV), formula_input(NET_SHAPE, 11).to(DEV)
    un(x, torch.tensor([500], device=DEV), c)
    g = pkg.GaussianDiffusion()
    pkg.DDIMSampler(g, un).sample(NET_SHAPE, c, 10, DEV, eta=0.0, progress=False, noise_fn=_noise_fn)
    pkg.DDPMSampler(g, un).sample(NET_SHAPE, c, DEV, progress=False, noise_fn=_noise_fn, num_steps=2)
    un.train()
    tshape = (2, 8, 2, 6, 6)
    z0, cond, noise = formula_input(tshape, 31).to(DEV), formula_input(tshape, 32).to(DEV), formula_noise(-1, tshape).to(DEV)
    loss, ld = g.to(DEV).training_loss(un, z0, cond, t=torch.tensor([37, 812], device=DEV), noise=noise)
    loss.backward()
    torch.cuda.synchronize()
    assert set(ld) == {"mse", "total"}
    keys = list(un._ctsi_programs)
    got = {}
    for key, prog in un._ctsi_programs.items():
        if key[0] in ("unet", "unet-train") or (key[0] == "sampler" and "ddim" in key):
            got[key[0]] = [m[0] for m in prog.op_meta]
    for k in ("unet", "sampler", "unet-train"):
        assert got[k] == want[k], k
    ddpm = [p for k, p in un._ctsi_programs.items() if k[0] == "sampler" and "ddpm" in k]
    assert len(ddpm) == 1 and [m[0] for m in ddpm[0].op_meta][:-2] == want["unet"]
    assert [m[0] for m in ddpm[0].op_meta][-2:] == ["sampler.step", "sampler.advance"]
    idx = torch.device(DEV).index
    n, Lc, d, h, w = NET_SHAPE
    assert sorted(map(repr, keys)) == sorted(map(repr, [
        ("unet", idx, 1, d, h, w, 1, "fast", "bf16"),
        ("sampler", idx, 1, d, h, w, 1001, "ddim", False, "fast", "bf16"),
        ("sampler", idx, 1, d, h, w, 1001, "ddpm", True, "fast", "bf16"),
        ("unet-train", idx, 2, 2, 6, 6)]))
    for p in un._ctsi_programs.values():
        assert not any(m[0] == "sigma.split" for m in p.op_meta) and getattr(p, "out2", None) is None
    E.invalidate_engine_cache(un)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the analytic model
# ---------------------------------------------------------------------------------------------------------------------
A_SHAPE, A_M, A_S, A_N = (2, 8, 4, 16, 16), 0.3, 0.5, 10


def _analytic_kernel_run(g, chain_t, rows, v_opt, learned):
    """'ddpm_spaced' on the analytic N(m, s^2) model by DIRECT kernel launches of a strided step -- ctsi_sigma_split on the
    model's 2L-channel output, then ctsi_ddpm_lv_step_f32 on the sampler's rows -- because a learned variance needs the engine's
    U-Net in the public loop (a 2L-channel callable is refused there) and a U-Net cannot be made analytic.  This does not run the
    plan, the vraw allocation or the split inside the graph: section 4 does, on the tiny U-Net.  The model: E[eps | z_t] in channels [0, L), the optimal v in [L, 2L)."""
    lib, ctx = L.get_lib(), E.Ctx.get(torch.device(DEV))
    n, Lc, d, h, w = A_SHAPE
    ac = g.alphas_cumprod.double()
    z = _nd(_randn(A_SHAPE, 7000)).to(DEV)
    zin = torch.empty_like(z)
    eps, vraw = torch.empty_like(z), torch.empty_like(z)
    table = rows.to(DEV).contiguous()
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for j, t in enumerate(chain_t):
        k, shift = LR.analytic_eps_coefs(float(ac[t]), A_M, A_S)
        out2 = torch.cat([(k * (z.double() - shift)).float(), torch.full_like(z, float(v_opt[j]))], dim=-1).contiguous()
        noise = _randn(A_SHAPE, 7001 + j).to(DEV)
        with ctx.scope():
            lib.sigma_split(_ptr(out2), _ptr(eps), _ptr(vraw) if learned else None, n, n if learned else 0, Lc, d, h, w, ctx.sptr)
            lib.ddpm_lv_step_f32(_ptr(z), _ptr(eps), _ptr(vraw) if learned else None, _ptr(noise), _ptr(zin), Lc, 0, _ptr(table),
                                 _ptr(step), n, Lc, d, h, w, ctx.sptr)
            lib.step_advance(_ptr(step), ctx.sptr)
        torch.cuda.synchronize()
    assert int(step.item()) == len(chain_t) and torch.equal(z, zin)
    return _nc(z).cpu()


@pytest.mark.parametrize("var_type", ["fixed_small", "learned_range"])
def test_analytic_model_sample_std(pkg, var_type):
    """i.i.d. N(0.3, 0.5^2) data: the optimal eps and the optimal reverse variance are closed forms.  'ddpm_spaced' with N = 10,
    clip_denoised=False, on 16384 elements; the host's linear-Gaussian recursion (float64) gives the std each variance type
    must produce -- 0.38878 for fixed-small (too small: the samples lose variance), 0.49990 for the learned range (the data's) --
    40 standard errors apart (asserted on the CPU in tests/test_host_learned_sigma.py and here).  The engine's sample std has to
    lie within 5 standard errors, std / sqrt(2 * 16384), of its own type's value."""
    g = pkg.GaussianDiffusion()
    g.var_type = var_type
    learned = var_type == "learned_range"
    sp = pkg.DDPMSampler(g, None)
    kind, chain_t = sp.chain(A_N, False)
    assert kind == "ddpm_lv" and len(chain_t) == A_N + 1
    rows = sp.coef_rows(A_N, False)
    chain = LR.respaced(g.alphas_cumprod, chain_t)
    v_opt, _ = LR.analytic_optimal_v(chain, A_M, A_S)
    want_mean, want = LR.analytic_sample_std(chain, A_M, A_S, v_opt if learned else None)
    _, other = LR.analytic_sample_std(chain, A_M, A_S, None if learned else v_opt)
    se = want / math.sqrt(2 * 16384)
    assert abs(want - other) > 10 * se
    out = _analytic_kernel_run(g, chain_t, rows, v_opt, learned)
    got, got_mean = float(out.double().std()), float(out.double().mean())
    print(f"analytic {var_type}: sample std {got:.5f} recursion {want:.5f} ({abs(got - want) / se:.2f} standard errors of {se:.2e}); "
          f"the other type's value {other:.5f} ({abs(got - other) / se:.1f} SE away); mean {got_mean:.4f} recursion {want_mean:.4f}")
    assert out.numel() == 16384 and torch.isfinite(out).all()
    assert abs(got - want) <= 5 * se
    assert abs(got_mean - want_mean) <= 5 * want / math.sqrt(out.numel())
    if not learned:
        # the public loop on the same model (a generic callable returns L channels: fixed-small only) draws the same process
        model = lambda z, t, c: (LR.analytic_eps_coefs(float(g.alphas_cumprod[int(t[0])]), A_M, A_S)[0]
                                 * (z - LR.analytic_eps_coefs(float(g.alphas_cumprod[int(t[0])]), A_M, A_S)[1]))
        nf = lambda i, shp: _randn(shp, 7000 if i < 0 else 7001 + i).to(DEV)
        pub = pkg.DDPMSampler(g, model).sample(A_SHAPE, torch.zeros(A_SHAPE, device=DEV), DEV, progress=False, noise_fn=nf,
                                               num_inference_steps=A_N, clip_denoised=False).cpu()
        err = rel_l2(pub, out)
        print(f"analytic fixed_small through DDPMSampler.sample(num_inference_steps=10) on the callable: rel-L2 to the launches "
              f"above {err:.3e}; std {float(pub.double().std()):.5f}")
        assert abs(float(pub.double().std()) - want) <= 5 * se and err < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 6. training
# ---------------------------------------------------------------------------------------------------------------------
TRAIN_SHAPE = (2, 8, 4, 8, 8)
T_FIX = torch.tensor([37, 812])


def _train_inputs():
    return formula_input(TRAIN_SHAPE, 31), formula_input(TRAIN_SHAPE, 32), formula_noise(-1, TRAIN_SHAPE)


def _oracle_grads(sd, cfg, g, learned):
    """The fp32 oracle's loss and parameter gradients (oracle/ref_ops.py's U-Net; the hybrid objective written here from the
    restatement's formulas in fp32)."""
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    z0, cond, noise = _train_inputs()
    a = g.sqrt_alphas_cumprod[T_FIX].float().view(-1, 1, 1, 1, 1)
    s = g.sqrt_one_minus_alphas_cumprod[T_FIX].float().view(-1, 1, 1, 1, 1)
    out = R.unet_forward(sd, cfg, a * z0 + s * noise, T_FIX, cond, "")
    ac = g.alphas_cumprod[T_FIX]
    snr = ac / (1 - ac + 1e-8)
    wgt = torch.clamp(snr, max=5.0) / (snr + 1e-8)
    Lc = z0.shape[1]
    loss = (((out[:, :Lc] - noise) ** 2).reshape(out.shape[0], -1).mean(1) * wgt).mean()
    if learned:
        sched = {k: v.float() for k, v in LR.schedule64(g).items()}
        _, vb = LR.hybrid_terms(out, z0.float(), noise.float(), T_FIX, sched, False)
        loss = loss + (g.timesteps / 1000.0) / math.log(2.0) * vb.reshape(out.shape[0], -1).mean(1).mean()
    loss.backward()
    return loss.item(), {k: v.grad for k, v in sd.items()}


def test_hybrid_training_against_the_oracle_and_one_optimizer_step(pkg):
    """One step at (2, 8, 4, 8, 8): the loss and every parameter gradient against the fp32 oracle's autograd, by the criterion of
    section 7 of tests/test_gpu_vpred.py -- the yardstick is the default (epsilon, fixed-small) model's rel-L2 against the same
    oracle, measured here; the learn_sigma run within 2 x, its loss within 2e-2.  Rows [L, 2L) of conv_out receive a gradient,
    and one FusedAdamW step changes the variance channels of the next forward."""
    cfg = unet_cfg(TINY_UNET)
    z0, cond, noise = (x.to(DEV) for x in _train_inputs())
    Lc = TRAIN_SHAPE[1]
    figures, un = {}, None
    for learned in (False, True):
        un = pkg.UNet3D(**TINY_UNET, learn_sigma=learned)
        sd = load_formula(un, 8)
        un.to(DEV).train()
        g = pkg.GaussianDiffusion()
        g.var_type = "learned_range" if learned else "fixed_small"
        ref_loss, ref_g = _oracle_grads(sd, cfg, g, learned)
        g.to(DEV)
        loss, ld = g.training_loss(un, z0, cond, t=T_FIX.to(DEV), noise=noise.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        got = torch.cat([p.grad.float().cpu().reshape(-1) for _, p in un.named_parameters()])
        ref = torch.cat([ref_g[k].reshape(-1) for k, _ in un.named_parameters()])
        figures[learned] = (rel_l2(got, ref), abs(loss.item() - ref_loss) / abs(ref_loss))
        print(f"{'hybrid (learn_sigma)' if learned else 'default'} training vs fp32 oracle: gradient rel-L2 {figures[learned][0]:.3e}, "
              f"loss {loss.item():.6f} oracle {ref_loss:.6f} rel {figures[learned][1]:.3e}; loss_dict {ld}")
        if learned:
            assert set(ld) == {"mse", "vb", "total"}
            assert abs(ld["total"] - (ld["mse"] + ld["vb"])) <= 1e-5 * abs(ld["total"]) and ld["vb"] != 0.0
            assert abs(ld["total"] - loss.item()) <= 1e-6 * abs(loss.item())
            gw, gb = un.conv_out[2].weight.grad, un.conv_out[2].bias.grad
            hi_w, hi_b = float(gw[Lc:].abs().max()), float(gb[Lc:].abs().max())
            rel_hi = rel_l2(gw[Lc:].cpu(), ref_g["conv_out.2.weight"][Lc:])
            print(f"conv_out rows [L, 2L): max |dW| {hi_w:.3e}, max |db| {hi_b:.3e}, rel-L2 to the oracle {rel_hi:.3e}")
            assert hi_w > 0 and hi_b > 0 and gw.shape[0] == 2 * Lc
            keys = [k for k in un._ctsi_programs if k[0] == "unet-train"]
            assert len(keys) == 1 and keys[0][-1] == "learn_sigma"
        else:
            assert set(ld) == {"mse", "total"}
            E.invalidate_engine_cache(un)
    assert figures[True][0] <= 2 * figures[False][0], figures
    assert figures[True][1] <= 2e-2
    # one FusedAdamW step changes the variance channels of the next forward
    g = _learned(pkg).to(DEV)
    un.eval()
    x, t = formula_input(TRAIN_SHAPE, 10).to(DEV), T_FIX.to(DEV)
    before = un(x, t, cond).clone()
    un.train()
    opt = pkg.FusedAdamW(list(un.parameters()), lr=2e-4, engine_modules=[un])
    opt.zero_grad(set_to_none=True)
    loss, _ = g.training_loss(un, z0, cond, t=t, noise=noise)
    loss.backward()
    opt.step()
    un.eval()
    after = un(x, t, cond)
    dv, dp = float((after[:, Lc:] - before[:, Lc:]).abs().max()), float((after[:, :Lc] - before[:, :Lc]).abs().max())
    print(f"one FusedAdamW step: max change of the variance channels {dv:.3e}, of the prediction channels {dp:.3e}")
    assert dv > 0 and dp > 0
    E.invalidate_engine_cache(un)


def test_training_loss_with_masks_equals_the_restatement_on_the_programs_prediction(pkg, wide_unet):
    """training_loss with and without a mask (equal and unequal valid counts): total, 'mse' and 'vb' against the float64
    restatement evaluated on the program's own 2L-channel prediction buffer; 1e-5 relative, the figure of
    tests/test_gpu_vpred.py's loss test."""
    g, gc = _learned(pkg).to(DEV), _learned(pkg)
    z0, cond, noise = _train_inputs()
    n, Lc, d, h, w = TRAIN_SHAPE
    t = torch.tensor([0, 812])
    wide_unet.train()
    try:
        for tag in ("nomask", "equal", "unequal"):
            mask = MASKS[tag]
            loss, ld = g.training_loss(wide_unet, z0.to(DEV), cond.to(DEV), mask=None if mask is None else mask.to(DEV),
                                       t=t.to(DEV), noise=noise.to(DEV))
            torch.cuda.synchronize()
            prog = [p for k, p in wide_unet._ctsi_programs.items() if k[0] == "unet-train" and k[2:6] == (n, d, h, w)]
            assert len(prog) == 1 and prog[0].eps.shape[-1] == 2 * Lc
            pred2 = _nc(prog[0].eps.cpu())
            ref = LR.hybrid_loss(pred2.double(), z0, noise, t, gc, gc._snr_weight(t), mask, False)
            rel = {k: abs(ld[k] - float(ref[k])) / abs(float(ref[k])) for k in ("total", "mse", "vb")}
            print(f"training_loss [{tag}]: {ld}; float64 on the program's prediction "
                  f"{ {k: float(v) for k, v in ref.items()} }; rel {rel}")
            assert all(v <= 1e-5 for v in rel.values()), rel
    finally:
        wide_unet.eval()
        for p in wide_unet.parameters():
            p.grad = None


# ---------------------------------------------------------------------------------------------------------------------
# 7. poison-and-guard
# ---------------------------------------------------------------------------------------------------------------------
def test_poison_strided_learned_variance_run_and_hybrid_training_step(pkg):
    un = pkg.UNet3D(**TINY_UNET, learn_sigma=True)
    load_formula(un, 8)
    un.to(DEV)
    g = _learned(pkg).to(DEV)
    shape = (1, 8, 5, 6, 10)
    cond = formula_input(shape, 12).to(DEV)
    nf = lambda i, shp: formula_noise(i, shp).to(DEV)

    def sample():
        traj = []
        out = pkg.DDPMSampler(g, un).sample(shape, cond, DEV, progress=False, noise_fn=nf, trajectory=traj,
                                            num_inference_steps=3, guidance_scale=2.5)
        torch.cuda.synchronize()
        return {"z0": out, "trajectory": traj}

    PZ.run_scenario(sample, name="lv-sample[ddpm_spaced,cfg]", modules=[un], ragged=True, inside=PZ.reevaluate(sample))
    tshape = (2, 8, 3, 6, 10)
    z0, tc, noise = (t.to(DEV) for t in (formula_input(tshape, 31), formula_input(tshape, 32), formula_noise(-1, tshape)))
    t = torch.tensor([0, 990], device=DEV)
    un.train()

    def train():
        for p in un.parameters():
            p.grad = None
        loss, _ = g.training_loss(un, z0, tc, t=t, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
        return {"loss": loss.detach(), "grad": {k: p.grad for k, p in un.named_parameters() if p.grad is not None}}

    PZ.run_scenario(train, name="hybrid-train", modules=[un], ragged=True, inside=PZ.reevaluate(train))
    E.invalidate_engine_cache(un)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the three precisions on one strided run
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


@contextlib.contextmanager
def _oracle(kind):
    with contextlib.ExitStack() as st:
        if kind != "f32":
            st.enter_context(_float64_default())
        if kind == "split":
            st.enter_context(x3_oracle())
        yield torch.float32 if kind == "f32" else F64


def test_three_precisions_agree_on_one_strided_run(pkg, wide_unet, monkeypatch):
    """A 4-step 'ddpm_spaced' learned-variance trajectory under bf16x3, fp32 and bf16 against the same loop around the oracle
    U-Net in float64 (truth), in fp32 and in float64 under the split-product shim, by the criterion
    tests/test_gpu_bf16x3_mode.py applies to its sampler trajectories: e(bf16x3) <= 2 e_split + max(4 e32, 2e-7) + 1e-6 and
    <= e(bf16) / 32 + 1e-6; the fp32 mode by its own rule (tests/test_gpu_fp32_mode.py), e(fp32) <= max(4 e32, 2e-7) + 1e-6."""
    monkeypatch.setattr(R, "CONVT_AS_CONV", True)     # (see tests/test_gpu_fullsize.py: MIOpen's fp32 ConvT search)
    g = _learned(pkg)
    cond = formula_input(NET_SHAPE, 21).to(DEV)
    N, Lc = 4, NET_SHAPE[1]
    sp = pkg.DDPMSampler(g, wide_unet)
    kind, chain = sp.chain(N)
    rows = LR.rows64(g.alphas_cumprod, chain, True)
    sd = {k: v.detach() for k, v in wide_unet.state_dict().items()}
    cfg = unet_cfg(TINY_UNET)
    trajs = {}
    for precision in ("bf16x3", "fp32", "bf16"):
        with _precision(wide_unet, precision):
            trajs[precision] = []
            sp.sample(NET_SHAPE, cond, DEV, progress=False, noise_fn=_noise_fn, num_inference_steps=N, trajectory=trajs[precision])
    refs = {}
    for okind in ("f64", "f32", "split"):
        with _oracle(okind) as dt:
            sdx = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
            z = _noise_fn(-1, NET_SHAPE).to(dt)
            traj = []
            for j, t in enumerate(chain):
                out = R.unet_forward(sdx, cfg, z, torch.tensor([t], device=DEV), cond.to(dt), "")
                if dt == F64:
                    z, _, _ = LR.step(z, out[:, :Lc], out[:, Lc:], _noise_fn(j, NET_SHAPE), rows[j])
                else:       # the fp32 oracle: the same update in fp32 torch ops
                    r = rows[j].float().tolist()
                    z0 = ((z - r[0] * out[:, :Lc]) / r[1]).clamp(-1, 1)
                    f = (out[:, Lc:] + 1) / 2
                    z = r[2] * z0 + r[3] * z + r[6] * torch.exp(0.5 * f * (r[4] - r[5])) * _noise_fn(j, NET_SHAPE)
                traj.append(z.clone())
            refs[okind] = traj
    assert len(trajs["bf16x3"]) == len(refs["f64"]) == N + 1
    for i in range(N + 1):
        t64 = refs["f64"][i]
        e32, es = rel_l2(refs["f32"][i], t64), rel_l2(refs["split"][i], t64)
        e, ef, ebf = (rel_l2(trajs[p][i], t64) for p in ("bf16x3", "fp32", "bf16"))
        print(f"strided learned-variance latent {i}: bf16x3 {e:.3g}, fp32 {ef:.3g}, bf16 {ebf:.3g}; split restatement {es:.3g}, "
              f"fp32 oracle {e32:.3g} (bf16 / bf16x3 = {ebf / max(e, 1e-30):.0f})")
        assert all(bool(torch.isfinite(trajs[p][i]).all()) for p in trajs)
        assert e <= 2.0 * es + max(4.0 * e32, 2e-7) + 1e-6
        assert e <= ebf / 32.0 + 1e-6
        assert ef <= max(4.0 * e32, 2e-7) + 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 9. the single-step API and what is refused
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False])
def test_single_step_api_returns_the_learned_variance(pkg, clip):
    """p_mean_variance / p_sample under 'learned_range' with per-sample t (0 and 600) on a callable that returns 2L channels,
    against float64 from the registered buffers: 1e-5 of the maximum, the figure of tests/test_gpu_vpred.py's single-step test
    (t stays where sqrt(abar) >= 0.1)."""
    g, gc = _learned(pkg).to(DEV), _learned(pkg)
    shape = (2, 8, 2, 4, 4)
    Lc = shape[1]
    z_t, cond, noise = _randn(shape, 3), formula_input(shape, 4), _randn(shape, 5)
    t = torch.tensor([0, 600])
    out2 = torch.cat([0.4 * z_t + 0.1 * cond, torch.rand(shape, generator=torch.Generator().manual_seed(6)) * 3.0 - 1.5], 1)
    model = lambda z, tt, c: out2.to(DEV)
    mean, var, logvar = g.p_mean_variance(model, z_t.to(DEV), t.to(DEV), cond.to(DEV), clip_denoised=clip)
    samp = g.p_sample(model, z_t.to(DEV), t.to(DEV), cond.to(DEV), clip_denoised=clip, noise=noise.to(DEV))
    torch.cuda.synchronize()
    sc = LR.schedule64(gc)
    col = lambda k: sc[k][t].view(-1, 1, 1, 1, 1)
    x0 = (z_t.double() - col("s") * out2[:, :Lc].double()) / col("a")
    if clip:
        x0 = x0.clamp(-1, 1)
    ref_mean = col("c1") * x0 + col("c2") * z_t.double()
    f = (out2[:, Lc:].double() + 1) / 2
    ref_lv = f * col("log_beta") + (1 - f) * col("log_post")
    ref_samp = ref_mean + (t != 0).double().view(-1, 1, 1, 1, 1) * torch.exp(0.5 * ref_lv) * noise.double()
    figs = {}
    for name, got, ref in (("mean", mean, ref_mean), ("log_variance", logvar, ref_lv), ("variance", var, torch.exp(ref_lv)),
                           ("p_sample", samp, ref_samp)):
        figs[name] = float((got.cpu().double() - ref).abs().max()) / float(ref.abs().max())
        assert got.shape == shape
    print(f"single step, learned variance, clip={clip}: max err / max|ref| {figs}")
    assert all(v <= 1e-5 for v in figs.values()), figs
    with pytest.raises(L.CtsiError, match="2 x 8 channels"):
        g.p_mean_variance(lambda z, tt, c: z, z_t.to(DEV), t.to(DEV), cond.to(DEV))


def test_refusals(pkg, wide_unet):
    """Depth sharding with learn_sigma, update_form 'x0' with a learned-variance step, a generic callable under
    'learned_range', and the two mismatched pairings: CtsiError with a sentence that says so, before any launch."""
    P = importlib.import_module("video-to-video-diffusion_amd.parallel")
    g, gp = _learned(pkg), pkg.GaussianDiffusion()
    cond = formula_input(NET_SHAPE, 12).to(DEV)
    before = set(wide_unet._ctsi_programs)
    plain = pkg.UNet3D(**TINY_UNET)
    load_formula(plain, 8)
    plain.to(DEV)
    with pytest.raises(L.CtsiError, match="var_type = 'learned_range'"):
        pkg.DDIMSampler(gp, wide_unet).sample(NET_SHAPE, cond, 2, DEV, progress=False)
    with pytest.raises(L.CtsiError, match="learn_sigma=True"):
        pkg.DDPMSampler(g, plain).sample(NET_SHAPE, cond, DEV, progress=False, num_inference_steps=2)
    with pytest.raises(L.CtsiError, match="learn_sigma=True"):
        g.to(DEV).training_loss(plain, cond, cond)
    g = _learned(pkg)
    with pytest.raises(L.CtsiError, match="generic model"):
        pkg.DDPMSampler(g, lambda z, t, c: z).sample(NET_SHAPE, cond, DEV, progress=False, num_inference_steps=2)
    gx = _learned(pkg, prediction_type=V)
    gx.update_form = "x0"
    with pytest.raises(L.CtsiError, match="update_form='x0'"):
        pkg.DDPMSampler(gx, wide_unet).sample(NET_SHAPE, cond, DEV, progress=False, num_inference_steps=2)

    class OneRank(P.LocalComm):
        rank = 0

    wide_unet.depth_shard_comm = OneRank(2)
    try:
        with pytest.raises(L.CtsiError, match="depth sharding"):
            pkg.DDPMSampler(g, wide_unet).sample(NET_SHAPE, cond, DEV, progress=False, num_inference_steps=2)
    finally:
        del wide_unet.depth_shard_comm
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope(), pytest.raises(L.CtsiError, match="depth sharding"):
        E.UNetProgram(ctx, wide_unet, 1, 2, 8, 8, 8, "fast", shard=P.ShardSpec(0, 2, OneRank(2), 4))
    assert set(wide_unet._ctsi_programs) == before                  # nothing was built
    # v-prediction in the eps form and the 'ddpm_spaced' name through generate's table run
    gv = _learned(pkg, prediction_type=V)
    out = S.SAMPLERS["ddpm_spaced"](gv, wide_unet, NET_SHAPE, cond, 3, DEV, noise_fn=_noise_fn, progress=False)
    assert out.shape == NET_SHAPE and torch.isfinite(out).all()
    keys = [k for k in wide_unet._ctsi_programs if k[0] == "sampler" and V in k]
    assert len(keys) == 1 and "learned" in keys[0] and "ddpm_lv" in keys[0]
    names = [m[0] for m in wide_unet._ctsi_programs[keys[0]].op_meta]
    i = names.index("sigma.split")
    assert names[i:i + 3] == ["sigma.split", "pred.to_eps", "sampler.step"]       # the split sits ahead of the conversion
    E.invalidate_engine_cache(plain)
