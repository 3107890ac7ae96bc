"""CPU: the forward audit's comparison sees the defects the older bounds let through (tests/fwd_audit.py).

The unit tests bound a conv by rel-L2 <= 3e-3 and max |d| <= 2e-2 max |ref| against fp32 F.conv3d, and its GroupNorm sums by
rtol 1e-3 (+ an absolute term on the plain sum).  Here a "kernel output" is built on the CPU as bf16(fp32-accumulated conv) of
bf16 operands -- what a correct kernel stores -- and compared with the float64 reference by the audit's own comparison; it must
pass, every element compared.  Then five defects a halo-tile / split-K kernel can have at one tile are put in, each of which the
audit must refuse:
  1  one tap's 8-channel chunk lost in one 512-voxel tile
  2  one W-line of the staged halo shifted by one voxel in one tile
  3  one split-K partial of one tile added twice
  4  an intermediate (a split-K partial) rounded to bf16 before the final rounding -- a second rounding
  5  one tile's contribution missing from the column sums
and defects 1 and 5 are shown to lie INSIDE the older bounds: that is the gap.

Two constructions, both unit-variance bf16 inputs and weights of variance 1 / K:
  A  K = 27 x 768 (the deepest K of the programs), 128 tiles (8 x 64 x 128 voxels), 8 couts: defects 1-4.  The lost chunk moves
     an affected output by sigma_e = sqrt(8 / K) sigma = 0.020 sigma; the largest of the 512 x 8 affected ones (~3.7 sigma_e)
     stays under 2e-2 max |ref| ~ 0.09 sigma, and the global rel-L2 stays under 3e-3.  (At K = 27 x 128, sigma_e = 0.048 sigma and
     the largest affected output does poke above the older max bound; its rel-L2 bound still misses it.)
  B  K = 27 x 128, 2048 tiles (64 x 128 x 128 voxels), 8 couts, bias 1: defect 5.  One tile is 4.9e-4 of either sum: inside rtol
     1e-3, outside F32_REL_L2 = 1e-4.  The bias models a conv's own: on zero-mean outputs the older test's absolute term on the
     plain sum, 1e-2 sqrt(N), is smaller than one tile's own sum (~ sqrt(512 x 8) sigma), so the plain sum would betray the tile
     about two times in three; the sum of squares never would.

Also here: conv64's depth slabs give the values of one call, and every record kind has a reference and an _INPUTS entry."""
import math
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from tests import fwd_audit as A
from tests import train_audit as T

F64 = torch.float64
TILE = 512
BUDGET = 1 << 30            # bytes of float64 columns per conv call on the host


def _operands(cin, cout, d, h, w, seed, bias=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, cin, d, h, w), generator=g).to(torch.bfloat16)
    wt = (torch.randn((cout, cin, 3, 3, 3), generator=g) / math.sqrt(27 * cin)).to(torch.bfloat16)
    b = torch.full((cout,), float(bias))
    return x, wt, b


def _kernel_f32(x, wt, b):
    """What a correct kernel accumulates: exact bf16 products, fp32 sums."""
    return F.conv3d(x.float(), wt.float(), b.float(), padding=1).contiguous()


def _tile(t, idx):
    """view of tile `idx` of a (1, c, d, h, w) tensor: (c, 512) consecutive voxels"""
    return t.view(t.shape[1], -1)[:, idx * TILE:(idx + 1) * TILE]


def _old_conv_bounds(out_bf16, ref64):
    err = out_bf16.to(F64) - ref64
    return float(err.norm() / ref64.norm()) <= 3e-3 and float(err.abs().max()) <= 2e-2 * float(ref64.abs().max())


@pytest.fixture(scope="module")
def case_a():
    x, wt, b = _operands(768, 8, 8, 64, 128, seed=0)
    ref = A.conv64(x, wt, (1, 1), (1, 1, 1), False, BUDGET) + b.to(F64).view(1, -1, 1, 1, 1)
    return x, wt, b, _kernel_f32(x, wt, b), ref


def test_unmutated_output_passes_with_every_element_compared(case_a):
    x, wt, b, acc, ref = case_a
    out = acc.to(torch.bfloat16)
    assert ref.numel() == out.numel() == 8 * 128 * TILE         # 128 tiles of 512 voxels, 27 x 768 terms each
    res = T.cmp_bf16(out, ref)
    assert res["ok"], res
    assert res["ulps"] <= 0.51 + 1e-3, res       # one rounding: half an ulp (+ the fp32 accumulation, far below it)
    # every element takes part: moving any single one by two ulps flips the result
    for flat in (0, out.numel() // 2 + 77, out.numel() - 1):
        bad = out.clone().reshape(-1)
        bad[flat] = (bad[flat].double() + 2.5 * T.bf16_ulp(ref.reshape(-1)[flat]) + 3 * T.BF16_FLOOR).to(torch.bfloat16)
        assert not T.cmp_bf16(bad, ref)["ok"], flat


def _mutations(case):
    x, wt, b, acc, ref = case
    tile = 37                                   # an interior tile: depth slice 2 (16 tiles per slice), rows 20 .. 23
    # 1: tap (0, 1, 2), channels 8 .. 15
    xc, wc = torch.zeros_like(x), torch.zeros_like(wt)
    xc[:, 8:16] = x[:, 8:16]
    wc[:, :, 0, 1, 2] = wt[:, :, 0, 1, 2]
    lost = F.conv3d(xc.float(), wc.float(), padding=1).contiguous()
    m1 = acc.clone()
    _tile(m1, tile).sub_(_tile(lost, tile))
    # 2: the tile is computed from an input whose line (d = 2, h = 21) sits one voxel further along w
    xs = x.clone()
    xs[:, :, 2, 21, 1:] = x[:, :, 2, 21, :-1]
    xs[:, :, 2, 21, 0] = 0
    m2 = acc.clone()
    _tile(m2, tile).copy_(_tile(_kernel_f32(xs, wt, b), tile))
    # 3 and 4: the split-K partial over the second half of the channels
    xh = x.clone()
    xh[:, :384] = 0
    part = F.conv3d(xh.float(), wt.float(), padding=1).contiguous()
    m3 = acc.clone()
    _tile(m3, tile).add_(_tile(part, tile))
    m4 = ((acc - part) + part.to(torch.bfloat16).float())
    return dict(lost_chunk=m1, shifted_halo_line=m2, doubled_splitk_partial=m3, double_rounding=m4)


def test_tile_defects_fail_the_audit(case_a):
    ref = case_a[4]
    muts = _mutations(case_a)
    for name, acc in muts.items():
        res = T.cmp_bf16(acc.to(torch.bfloat16), ref)
        assert not res["ok"], (name, res)
    # the gap: the lost chunk is inside the older conv bounds (and the unmutated output, of course, too)
    assert _old_conv_bounds(case_a[3].to(torch.bfloat16), ref)
    assert _old_conv_bounds(muts["lost_chunk"].to(torch.bfloat16), ref)


def test_lost_colsum_tile_fails_the_audit_inside_the_old_bounds():
    x, wt, b = _operands(128, 8, 64, 128, 128, seed=1, bias=1.0)
    ref = A.conv64(x, wt, (1, 1), (1, 1, 1), False, BUDGET) + b.to(F64).view(1, -1, 1, 1, 1)
    acc = _kernel_f32(x, wt, b)
    tiles = acc[0, 0].numel() // TILE
    assert tiles == 2048
    # the slab a kernel writes: per tile fp32 sums of the unrounded accumulators
    t1 = acc.reshape(8, tiles, TILE).sum(-1)
    t2 = (acc * acc).reshape(8, tiles, TILE).sum(-1)
    ref1, ref2 = ref.sum((2, 3, 4)), (ref * ref).sum((2, 3, 4))
    ok1, ok2 = T.cmp_f32(t1.double().sum(1), ref1), T.cmp_f32(t2.double().sum(1), ref2)
    assert ok1["ok"] and ok2["ok"], (ok1, ok2)
    keep = torch.ones(tiles, dtype=torch.bool)
    keep[1000] = False
    m1, m2 = t1[:, keep].double().sum(1), t2[:, keep].double().sum(1)
    bad1, bad2 = T.cmp_f32(m1, ref1), T.cmp_f32(m2, ref2)
    assert not bad1["ok"] and not bad2["ok"], (bad1, bad2)
    # the older check: the group's (sum, sumsq) (one group of 8 channels) against fp32 sums, rtol 1e-3
    n_el = float(ref.numel())
    assert torch.allclose(m1.sum(), ref1.sum(), rtol=1e-3, atol=1e-2 * math.sqrt(n_el))
    assert torch.allclose(m2.sum(), ref2.sum(), rtol=1e-3, atol=0.0)


@pytest.mark.parametrize("form", ["k3", "k1", "down", "convT"])
def test_depth_slabs_equal_one_call(form):
    g = torch.Generator().manual_seed(5)
    n, cin, cout, d, h, w = 2, 5, 6, 7, 6, 8
    k, s, p, tr = dict(k3=((3, 3, 3), (1, 1), (1, 1, 1), False), k1=((1, 1, 1), (1, 1), (0, 0, 0), False),
                       down=((3, 4, 4), (2, 2), (1, 1, 1), False), convT=((3, 4, 4), (2, 2), (1, 1, 1), True))[form]
    wshape = (cin, cout) + k if tr else (cout, cin) + k
    for integer in (True, False):
        if integer:      # small integers: every product and sum is exact, whatever the order -> the same bits
            x = torch.randint(-4, 5, (n, cin, d, h, w), generator=g).to(F64)
            wt = torch.randint(-4, 5, wshape, generator=g).to(F64)
        else:
            x, wt = torch.randn((n, cin, d, h, w), generator=g, dtype=F64), torch.randn(wshape, generator=g, dtype=F64)
        fn = F.conv_transpose3d if tr else F.conv3d
        whole = fn(x, wt, stride=(1,) + s, padding=p)
        for budget in (1, 3 * whole[0, 0, 0].numel() * 8 * cin * 48, 1 << 40):      # one slice per slab, a few, all
            got = A.conv64(x, wt, s, p, tr, budget)
            assert got.shape == whole.shape
            if integer:
                assert torch.equal(got, whole), (form, budget)
            else:                # a BLAS call of another shape may add in another order: a few float64 ulps of the sum
                assert float((got - whole).abs().max()) <= 1e-13 * float(whole.abs().max()), (form, budget)


def test_every_record_kind_has_a_reference_and_inputs():
    assert set(A.REFS) == set(A._INPUTS)
    # every kind the engines attach is known to the forward or the backward audit
    src = Path(__file__).resolve().parents[1] / "video-to-video-diffusion_amd"
    kinds = set()
    for f in ("engine.py", "engine_f32.py", "train_engine.py", "vae_train_engine.py"):
        kinds |= set(re.findall(r'kind="([a-z0-9_.]+)"', (src / f).read_text()))
    backward = set(T._INPUTS) | {"linear_wgrad_multi", "linear_bwd_chain"}
    assert kinds - backward == set(A.REFS), (kinds - backward) ^ set(A.REFS)
    for name, reason in A.SKIP.items():
        assert reason and ("comm" in reason or "memset" in reason), name
