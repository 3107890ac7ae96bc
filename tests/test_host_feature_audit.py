"""CPU: the float64 references of tests/feature_audit.py on the restatements' own outputs (0 error) and on known wrong forms
(refused), what the per-launch comparison sees that the network bound does not, and that every launch the feature modules
emit has a reference or stands on feature_audit.DEFERRED_BACKWARD.

The gap.  The engine's U-Net with the optional features is held to NET_TOL = 3e-2 rel-L2 against its restatement
(tests/test_gpu_resblock_options.py, test_gpu_attn_softmax.py, test_gpu_spatial_attention.py).  Here the restatement of program
A's network (tests/test_gpu_feature_program_audit.py) runs on the CPU in float32 against float64 with one plumbing defect at a
time, and the launch the defect sits in is compared the way the audit compares it:
  (i)   mid_block2 reads the time-row columns of its neighbour mid_block1 (same width);
  (ii)  the spatial block of level 0 splits its channels into heads / 2 heads;
  (iii) two ResBlocks share a dropout layer_id (training restatement: mid_block2 draws mid_block1's mask stream).
`test_network_bound_against_launch_bound` prints the network rel-L2 of each beside NET_TOL and asserts that the launch
comparison refuses every one.  What it shows, said plainly: on this two-level network ALL THREE move the output by more than
NET_TOL (0.106, 0.426 and 0.584 rel-L2 -- every block carries a large share of so small a network), so none of them is an
example of a defect that passes the network bound; they are kept, untuned, as defects the per-launch comparison catches as
well and NAMES (6560 x, 822 x its bound; 1728 elements of the dropped set wrong).  Two limits of the network bound remain and
are what the launch audit is for: (iii) is invisible to the existing training tests whatever its size, because they take their
masks from the program's own layer ids, so a shared id is restated along with everything else; and the launches behind the
network (which half sigma_split keeps, which buffer pred_to_eps converts) are bounded by a sampler trajectory only."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R
from tests import attn_restatement as AR
from tests import feature_audit as A
from tests import fwd_audit as FA
from tests import learned_sigma_restatement as LR
from tests import resblock_restatement as RR
from tests import spatial_attn_restatement as SR
from tests import train_audit as T
from tests.helpers import rel_l2
from tests.test_host_resblock_options import keep_mask_np

F64 = torch.float64
SRC = Path(__file__).resolve().parents[1] / "video-to-video-diffusion_amd"
NET_TOL = 3e-2          # tests/test_gpu_network.py: the bf16 engine against the fp32 oracle
HEADS = 4


def _bf16(t):
    return t.to(torch.bfloat16)


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


# ---- the references on the restatements' own outputs, and on wrong forms ----------------------------------------------------------
@pytest.mark.parametrize("film,drop", [(True, False), (False, False), (True, True)])
def test_gn_apply_mod_reference(film, drop):
    n, c, d, h, w, groups = 2, 32, 3, 5, 7, 8
    x = _bf16(_randn((n, d, h, w, c), 1))
    gamma, beta = 1.0 + 0.3 * _randn((c,), 2), 0.3 * _randn((c,), 3)
    row = 0.5 * _randn((n, 2 * c if film else c), 4)
    sums = RR.group_sums(x, groups)
    keep = None
    if drop:
        keep = torch.from_numpy(keep_mask_np(7, 3, 16384, x.numel()).astype(np.bool_)).view(x.shape)
    ref, need = A.ref_gn_apply_mod(x, sums, gamma, beta, row, groups, 1e-5, film, keep=keep, inv=4.0 / 3.0 if drop else 1.0)
    assert torch.equal(ref, RR.pass_fwd64(x, sums, gamma, beta, row, groups, 1e-5, film, keep=keep, inv=4.0 / 3.0 if drop else 1.0))
    res = A._bf16_elem(ref, ref, need)
    assert res["ok"] and res["ulps"] == 0.0
    print(f"film {film} drop {drop}: extra {res['extra']}, worst need / (floor x rms) "
          f"{float(need.max()) / (A.BF16_FLOOR * float(ref.pow(2).mean().sqrt())):.2f}")
    assert A._bf16_elem(_bf16(ref), ref, need)["ok"]
    assert bool((need >= 0).all()) and (keep is None or bool((need[~keep] == 0).all()))
    if film and not drop:
        for form in ("additive", "swapped", "noscale"):
            wrong = RR.pass_fwd64(x, sums, gamma, beta, row, groups, 1e-5, True, form=form)
            assert not A._bf16_elem(_bf16(wrong), ref, need)["ok"], form
        # fp32 engine: the elementwise class
        ref32, need32 = A.ref_gn_apply_mod(x.float(), sums, gamma, beta, row, groups, 1e-5, True, f32=True)
        assert A.cmp_elem(ref32.float(), ref32, need32)["ok"] and not A.cmp_elem(_bf16(ref32), ref32, need32)["ok"]


def test_gn_apply_mod_need_exceeds_the_floor_where_x_sits_on_its_mean():
    """A channel far from 0 with a small spread: |x sc| and |m sc| are ~1e3 times the result, the fp32 chain leaves more than
    the rms floor and the reference says so."""
    n, c, d, h, w, groups = 1, 16, 2, 4, 4, 2
    x = _bf16(300.0 + _randn((n, d, h, w, c), 5))
    gamma, beta, row = torch.ones(c), torch.zeros(c), torch.zeros(n, 2 * c)
    sums = RR.group_sums(x, groups)
    ref, need = A.ref_gn_apply_mod(x, sums, gamma, beta, row, groups, 1e-5, True)
    res = A._bf16_elem(_bf16(ref), ref, need)
    assert res["extra"] == "fp32 chain" and res["ok"]


def _permute_heads(qkv, heads, third):
    c = qkv.shape[-1] // 3
    out = qkv.clone()
    blk = out[..., third * c:(third + 1) * c].reshape(*qkv.shape[:-1], heads, c // heads)
    out[..., third * c:(third + 1) * c] = blk.roll(1, dims=-2).reshape(*qkv.shape[:-1], c)
    return out


@pytest.mark.parametrize("kind", ["attn_core", "attn_plane"])
def test_attention_references(kind):
    n, c, d, h, w = 1, 32, 5, 4, 6
    qkv = _randn((n, d, h, w, 3 * c), 11)
    qkv[..., :2 * c] *= 2.0 ** 0.5
    qkv = _bf16(qkv)
    if kind == "attn_core":
        ref = lambda t, hd=HEADS: A.ref_attn_core(t, hd)
        own = AR.core_fwd64(*AR.split_qkv(qkv, HEADS))[0]
    else:
        ref = lambda t, hd=HEADS: (lambda r: (r["a"], r["extra"], r["uniform"]))(A.ref_attn_plane(t, hd))
        own = AR.core_fwd64(*SR.split_qkv_plane(qkv, HEADS))[0]
    a, extra, uni = ref(qkv)
    assert torch.equal(a, own) and A.cmp_bf16(a, a, extra)["ulps"] == 0.0 and A.cmp_bf16(_bf16(a), a, extra)["ok"]
    assert rel_l2(uni, a) > 0.5 and not A.cmp_bf16(_bf16(uni), a, extra)["ok"]
    wrong = {"heads of q permuted": ref(_permute_heads(qkv, HEADS, 0))[0],
             "heads of v permuted": ref(_permute_heads(qkv, HEADS, 2))[0],
             "v taken from the k third": ref(torch.cat([qkv[..., :2 * c], qkv[..., c:2 * c]], -1))[0]}
    for name, bad in wrong.items():
        assert not A.cmp_bf16(_bf16(bad), a, extra)["ok"], name
    if kind == "attn_plane":
        r = A.ref_attn_plane(qkv, HEADS)
        assert A.cmp_elem(r["lse"], r["lse"], r["lse_tol"])["ulps"] == 0.0 and A.cmp_elem(r["lse"].float(), r["lse"], r["lse_tol"])["ok"]
        assert not A.cmp_elem(r["lse"] * (1 + 1e-5), r["lse"], r["lse_tol"])["ok"]


def test_elementwise_references_pass_on_their_own_output():
    shape = (2, 3, 4, 6, 8)                                                   # NDHWC
    z, v, hist, noise = (_randn(shape, 20 + k) for k in range(4))
    # pred_to_eps on a doubled batch with a history row
    out = _randn((4,) + shape[1:], 30)
    row = torch.tensor([0.31, 0.95, 0.4, 0.0])
    ref, bound = A.ref_pred_to_eps(out, z, hist, row, 2)
    assert A.cmp_within(ref, ref, bound)["ulps"] == 0.0 and A.cmp_within(ref.float(), ref, bound)["ok"]
    assert torch.equal(ref[2:], A.ref_pred_to_eps(out[2:], z, hist, row, 2)[0])      # rows [n, 2n) read the n rows of z again
    assert not A.cmp_within(A.ref_pred_to_eps(out, z, None, row, 2)[0], ref, bound)["ok"]
    # x0_step with history, noise and non-finite values in v
    vv = v.clone()
    vv.view(-1)[[5, 77, 101]] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    r = A.ref_x0_step(z, vv, torch.tensor([0.62, 0.78, 0.55, 0.41, -0.23, 0.37, 10.0, 0.0]), hist, noise)
    assert r["counts"] == [1, 2, 0, 0, 0, 0] and bool(torch.isfinite(r["z"]).all())
    assert A.cmp_within(r["z"], r["z"], r["bz"])["ulps"] == 0.0 and A.cmp_within(r["x"].float(), r["x"], r["bx"])["ok"]
    # ddpm_lv with and without the variance operand
    row = LR.rows64(torch.linspace(0.9999, 1e-4, 1000), [999, 700, 300, 0], True)[1]
    for vr in (None, torch.rand(shape, generator=torch.Generator().manual_seed(3)) * 3 - 1.5):
        ref, bound = A.ref_lv_step(z, v, vr, noise, row)
        assert A.cmp_within(ref, ref, bound)["ulps"] == 0.0 and A.cmp_within(ref.float(), ref, bound)["ok"]
    a, b = A.ref_lv_step(z, v, None, noise, row)[0], A.ref_lv_step(z, v, torch.zeros(shape), noise, row)[0]
    assert not torch.equal(a, b)                                               # the variance operand matters


def test_sigma_split_reference_and_the_other_half():
    n, L = 2, 4
    out2 = _randn((2 * n, 3, 4, 4, 2 * L), 40)
    eps, var = A.ref_sigma_split(out2, L, n)
    assert torch.equal(eps, out2[..., :L]) and torch.equal(var, out2[:n, ..., L:]) and A.cmp_same(var, var.clone())["ok"]
    assert not A.cmp_same(out2[n:, ..., L:].contiguous(), var)["ok"]           # the unconditional half kept instead
    assert not A.cmp_same(out2[:n, ..., :L].contiguous(), var)["ok"]           # the prediction channels kept instead


def test_window_references():
    import importlib
    WF = importlib.import_module("video-to-video-diffusion_amd.window_fuse")
    full, win, axes = (18, 8, 6), (12, 4, 4), ([0, 6], [0, 3, 4], [0, 1, 2])
    tables = [WF.axis_table(f, s, st) for f, s, st in zip(full, win, axes)]
    starts = [(a, b, c) for a in axes[0] for b in axes[1] for c in axes[2]]
    n, halves, L, nwin = 2, 2, 4, (2, 3, 3)
    win_t = 3.0 * _randn((halves * len(starts) * n,) + win + (L,), 50)
    ref, bound, got_starts = A.ref_window_blend(win_t, tables, n, halves, nwin, full, win)
    assert got_starts == starts
    assert A.cmp_within(ref, ref, bound)["ulps"] == 0.0 and A.cmp_within(ref.float(), ref, bound)["ok"]
    ones, _, _ = A.ref_window_blend(torch.ones_like(win_t), tables, n, halves, nwin, full, win)
    assert float((ones - 1).abs().max()) < 1e-12                               # a partition of unity
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    raw_tables = [t._replace(weight=np.where(t.weight > 0, S._axis_window(sz).double().numpy()[t.offset], 0.0))
                  for t, sz in zip(tables, win)]              # the stitching window itself, not divided by its sum over the covers
    raw, _, _ = A.ref_window_blend(win_t, raw_tables, n, halves, nwin, full, win)
    assert not A.cmp_within(raw, ref, bound)["ok"]                             # blend weights not normalised
    # gather: both halves, the conditioning half untouched
    src = _bf16(_randn((n,) + full + (L,), 51))
    zin0 = _bf16(_randn((halves * len(starts) * n,) + win + (2 * L,), 52))
    want = A.ref_window_gather(src, zin0, starts, n, halves, L, win)
    assert torch.equal(want[..., L:], zin0[..., L:])
    k, b, g = 7, 1, 1
    sd, sh, sw = starts[k]
    assert torch.equal(want[(g * len(starts) + k) * n + b, ..., :L], src[b, sd:sd + 12, sh:sh + 4, sw:sw + 4])
    one_half = A.ref_window_gather(src, zin0, starts, n, 1, L, win)
    assert not A.cmp_same(one_half, want)["ok"]                                # the unconditional rows not written


@pytest.mark.parametrize("v_pred", [False, True])
def test_hybrid_loss_reference_against_the_restatement(pkg, v_pred):
    import importlib
    LS = importlib.import_module("video-to-video-diffusion_amd.learned_sigma")
    g = pkg.GaussianDiffusion("cosine", 1000, prediction_type="v_prediction" if v_pred else "epsilon")
    shape = (2, 4, 3, 4, 4)
    n, L, d = shape[:3]
    t = torch.tensor([0, 640])
    z0, noise, pred2 = _randn(shape, 60), _randn(shape, 61), _randn((n, 2 * L) + shape[2:], 62)
    mask = torch.tensor([[[1., 1., 1.]], [[1., 0., 1.]]])
    weight = g._snr_weight(t)
    cn, me, pooled = LR.count_norm(mask, shape)
    assert not pooled
    norm, norm_vb = (weight.double() * cn).float(), (cn * (g.timesteps / 1000.0) / np.log(2.0)).float()
    ref, bound = A.ref_hybrid_loss(pred2, z0, noise, t, LS.loss_schedule_rows(g), v_pred, mask.expand(n, L, d).contiguous(),
                                   norm, norm_vb)
    own = LR.hybrid_loss(pred2.double(), z0, noise, t, g, weight, mask, v_pred)
    # the launch's table holds fp32 roundings of the float64 schedule: the two agree to that, far inside the bound
    for k, name in enumerate(("total", "mse", "vb")):
        assert abs(float(ref[k]) - float(own[name])) <= 0.1 * float(bound[k]), name
    assert A.cmp_within(ref, ref, bound)["ulps"] == 0.0 and A.cmp_within(ref.float(), ref, bound)["ok"]
    nomask, _ = A.ref_hybrid_loss(pred2, z0, noise, t, LS.loss_schedule_rows(g), v_pred, None, norm, norm_vb)
    other, _ = A.ref_hybrid_loss(pred2, z0, noise, t, LS.loss_schedule_rows(g), not v_pred, mask.expand(n, L, d).contiguous(),
                                 norm, norm_vb)
    assert not A.cmp_within(nomask, ref, bound)["ok"] and not A.cmp_within(other, ref, bound)["ok"]


# ---- the model's plan against a record's ---------------------------------------------------------------------------------------
def test_time_row_plan_overrides_a_record_that_points_at_a_neighbour(pkg):
    un, _ = A.feature_unet(pkg, A.MODEL_SEED)
    plan = A.time_row_plan(un)
    offs = [p["off"] for p in plan]
    assert offs == sorted(offs) and offs[0] == 0 and all(b - a == p["width"] for a, b, p in zip(offs, offs[1:], plan))
    assert all(p["width"] == 2 * p["gamma"].numel() for p in plan)             # scale-shift: (s | b)
    assert A.model_heads(un) == HEADS
    ctx = dict(time_rows=plan)
    for j, p in enumerate(plan):
        sn = dict(gamma=p["gamma"].clone())
        assert A._tb_columns(dict(tbias_off=p["off"]), sn, ctx) == p["off"]
        assert A._tb_columns(dict(tbias_off=plan[j - 1]["off"]), sn, ctx) == p["off"]      # a neighbour's columns: the model's win
    assert A._tb_columns(dict(tbias_off=5), dict(gamma=plan[0]["gamma"]), {}) == 5           # no model: the record's
    # same-shaped blocks with equal GroupNorm weights (a freshly initialised model) cannot be told apart: refused, not guessed
    fresh = pkg.UNet3D(**A.feature_kw())
    with pytest.raises(AssertionError, match="same GroupNorm"):
        A.time_row_plan(fresh)


# ---- the gain ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(pkg):
    un, sd = A.feature_unet(pkg, A.MODEL_SEED)
    x, c = A.program_inputs(A.SHAPE_A, A.INPUT_SEED)
    return dict(un=un, sd32={k: v.float() for k, v in sd.items()}, sd64={k: v.double() for k, v in sd.items()}, x=x, c=c,
                t=torch.tensor([999]), cfg=A.feature_cfg())


def _farthest(dist):
    return {kind: max(v for k, v in dist.values() if k == kind) for kind in ("attn_core", "attn_plane")}


def test_qk_gain_is_the_smallest_power_of_two(pkg, net):
    """At QK_GAIN the float32 restatement of program A's network has an attn_core and an attn_plane launch more than 0.5 rel-L2
    from uniform attention; at half of it it has not."""
    at = _farthest(A.uniform_distances(net["sd32"], net["cfg"], net["x"], net["t"], net["c"], HEADS))
    _, sd_half = A.feature_unet(pkg, A.MODEL_SEED, gain=A.QK_GAIN / 2)
    below = _farthest(A.uniform_distances({k: v.float() for k, v in sd_half.items()}, net["cfg"], net["x"], net["t"], net["c"], HEADS))
    print(f"gain {A.QK_GAIN}: {at}; gain {A.QK_GAIN / 2}: {below}")
    assert min(at.values()) > 0.5 and min(below.values()) <= 0.5
    assert np.log2(A.QK_GAIN) == int(np.log2(A.QK_GAIN))


# ---- what the network bound lets through ----------------------------------------------------------------------------------------
def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _middle_pass(sd, p, tap, row_of, keep=None, inv=1.0):
    """The middle pass of ResBlock `p` on its tapped input, float64 NDHWC: (x, sums, gamma, beta, row, groups)."""
    cout = sd[p + ".conv1.conv.weight"].shape[0]
    x = _ndhwc(R.conv3d(sd, p + ".conv1.conv", tap["x"], padding=1))
    groups = R.conv_block_groups(cout)
    row = F.linear(F.silu(tap["temb"]), sd[row_of + ".time_mlp.1.weight"], sd[row_of + ".time_mlp.1.bias"])
    return x, RR.group_sums(x, groups), sd[p + ".conv1.norm.weight"], sd[p + ".conv1.norm.bias"], row, groups


def test_network_bound_against_launch_bound(pkg, net):
    sd32, sd64, cfg, t = net["sd32"], net["sd64"], net["cfg"], net["t"]
    x32, c32, x64, c64 = net["x"], net["c"], net["x"].double(), net["c"].double()
    t64 = t.double()
    ref, taps = A.restated_taps(sd64, cfg, x64, t64, c64)
    clean = rel_l2(A.restated_taps(sd32, cfg, x32, t, c32)[0], ref)
    print(f"\nprogram A's network, float32 against float64: rel-L2 {clean:.3e} (NET_TOL {NET_TOL:.0e})")
    assert clean < 1e-4
    report = {}

    # (i) mid_block2 reads mid_block1's columns of the time row
    def neighbour(kind, p, a):
        if p == "mid_block2":
            a["sd"] = dict(a["sd"])
            for leaf in ("weight", "bias"):
                a["sd"][f"{p}.time_mlp.1.{leaf}"] = a["sd"][f"mid_block1.time_mlp.1.{leaf}"]

    net_i = rel_l2(A.restated_taps(sd32, cfg, x32, t, c32, edit=neighbour)[0], ref)
    xx, sums, gam, bet, row, groups = _middle_pass(sd64, "mid_block2", taps["mid_block2"], "mid_block2")
    wrong_row = _middle_pass(sd64, "mid_block2", taps["mid_block2"], "mid_block1")[4]
    want, need = A.ref_gn_apply_mod(_bf16(xx), RR.group_sums(_bf16(xx), groups), gam, bet, row.float(), groups, 1e-5, True)
    got = RR.pass_fwd64(_bf16(xx), RR.group_sums(_bf16(xx), groups), gam, bet, wrong_row.float(), groups, 1e-5, True)
    report["(i) neighbour's time-row columns"] = (net_i, A._bf16_elem(_bf16(got), want, need))

    # (ii) the level-0 spatial block uses heads / 2
    p = "down_blocks.0.0.1"

    def half_heads(kind, name, a):
        if name == p:
            a["heads"] = a["heads"] // 2

    net_ii = rel_l2(A.restated_taps(sd32, cfg, x32, t, c32, edit=half_heads)[0], ref)
    qkv = _bf16(A.tap_qkv(sd64, p, taps[p]["x"]))
    right = A.ref_attn_plane(qkv, HEADS)
    wrong = A.ref_attn_plane(qkv, HEADS // 2)["a"]                               # (n, d, heads / 2, N, 2 hd)
    n, d, _, N, _ = wrong.shape
    wrong = SR.split_plane(wrong.permute(0, 1, 3, 2, 4).reshape(n, d, N, 1, -1), HEADS)
    report["(ii) heads / 2 in one spatial block"] = (net_ii, A.cmp_bf16(_bf16(wrong), right["a"], right["extra"]))

    # (iii) two ResBlocks share a dropout layer_id (training restatement; the masks of tests/test_host_resblock_options.py)
    names = [nm for nm, m in net["un"].named_modules() if type(m).__name__ == "ResBlock3D"]
    seed, thr, inv = 0x0123456789ABCDEF, 16384, 65536.0 / (65536.0 - 16384)

    def mask_of(layer_id):
        def make(shape):
            b, c, d_, h_, w_ = shape
            k = keep_mask_np(seed, layer_id, thr, b * c * d_ * h_ * w_).reshape(b, d_, h_, w_, c)
            return torch.from_numpy(k.astype(np.float64)).permute(0, 4, 1, 2, 3)
        return make

    ids = {nm: j for j, nm in enumerate(names)}
    shared = dict(ids, mid_block2=ids["mid_block1"])
    ref_d = A.restated_taps(sd64, cfg, x64, t64, c64, masks={nm: mask_of(j) for nm, j in ids.items()}, inv=inv)
    net_iii = rel_l2(A.restated_taps(sd32, cfg, x32, t, c32, masks={nm: mask_of(j) for nm, j in shared.items()}, inv=inv)[0], ref_d[0])
    xx, sums, gam, bet, row, groups = _middle_pass(sd64, "mid_block2", ref_d[1]["mid_block2"], "mid_block2")
    xb = _bf16(xx)
    keep_r, keep_w = (torch.from_numpy(keep_mask_np(seed, j, thr, xb.numel()).astype(np.bool_)).view(xb.shape)
                      for j in (ids["mid_block2"], ids["mid_block1"]))
    got = _bf16(RR.pass_fwd64(xb, RR.group_sums(xb, groups), gam, bet, row.float(), groups, 1e-5, True, keep=keep_w, inv=inv))
    dropped = got[~keep_r]
    res = A.cmp_same(dropped, torch.zeros_like(dropped))
    report["(iii) a shared dropout layer_id"] = (net_iii, res)

    for name, (net_err, res) in report.items():
        inside = "inside" if net_err < NET_TOL else "OUTSIDE"
        worst = res.get("mismatches") if res["cls"] == "exact" else f"{res['ulps']:.1f} x its bound"
        print(f"{name}: network rel-L2 {net_err:.3e} ({inside} NET_TOL {NET_TOL:.0e}); its launch: "
              f"{'ok' if res['ok'] else 'FAIL'} ({worst})")
        assert not res["ok"], name


# ---- every launch of the feature modules has a reference --------------------------------------------------------------------------
def test_every_feature_record_kind_has_a_reference_or_is_deferred():
    assert set(A.REFS) == set(A._INPUTS)
    assert set(A.DEFERRED_BACKWARD) == {"gn_bwd_mod", "attn_core_bwd", "attn_plane_bwd", "hybrid_loss_bwd"}
    kinds = set()
    for f in ("norm_mod.py", "attention.py", "spatial_attention.py", "prediction.py", "x0_form.py", "learned_sigma.py",
              "window_fuse.py"):
        kinds |= set(re.findall(r'kind="([a-z0-9_.]+)"', (SRC / f).read_text()))
    assert kinds, "the scan found no record"
    known = set(A.REFS) | set(FA.REFS) | set(T._INPUTS)
    loose = {k for k in kinds if k not in known and k not in A.DEFERRED_BACKWARD}
    assert not loose, f"feature launches without a reference: {sorted(loose)}"
    assert set(A.DEFERRED_BACKWARD) <= kinds                   # the list names launches that exist
    # the learned-variance update is a sampler_step record of engine.py told apart by its `sampler`
    assert A.kind_of(dict(kind="sampler_step", sampler="ddpm_lv")) in A.REFS
    assert A.kind_of(dict(kind="sampler_step", sampler="ddim")) in FA.REFS and A.references("add") == "train"
    # what the references did not cover before: none of these is in fwd_audit's tables (pinned by test_host_fwd_audit.py)
    assert not set(A.REFS) & set(FA.REFS)
