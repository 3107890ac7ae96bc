"""CPU: the criterion the conv op tests now assert (tests/fwd_audit.py: one bf16 ulp per element against float64, F32_REL_L2 /
F32_MAX_REL for the fp32 weight gradient) bites at the op tests' own small shapes, where the bounds they had do not.

On three cases of tests/test_gpu_ops.py -- the narrow-tile split-K case `w24_256_256`, the ragged halo case `ragged_edges_batch2`
and the ConvTranspose case `ragged_batch2`, each with the operands the GPU test builds -- a "kernel output" is made on the CPU as
bf16(fp32-accumulated conv): what a correct kernel stores.  It must pass `cmp_bf16` against the float64 reference at <= 1 ulp.
Four defects a halo-tile / split-K kernel can have are then put in, each of which `cmp_bf16` must refuse:
  parked_bf16_partial   the split-K partial over the second half of the input channels rounded to bf16 before the final add
  lost_chunk            one corner voxel loses the 8-channel chunk of one tap
  tap_reads_w_minus_1   one tap reads an 8-channel chunk one voxel to the left, at one voxel of the ragged W edge
  one_ulp_high          every element one bf16 ulp above the correctly rounded value
and for each it is recorded (printed) whether the older pair of bounds -- rel-L2 < 3e-3 against the reference and, where a test
asserted it, max |d| < 2e-2 max |ref| -- would have passed it.  The older rel-L2 bound does pass the parked partial at every case
and the two single-voxel defects at `w24_256_256` (asserted): three of the op tests asserted nothing else.

The weight gradient: at the `S1_CASES` case `k3_long_k_256_128`, one voxel's contribution lost for 8 input channels fails `cmp_f32`
against float64 autograd, but its rel-L2 here is 3.7e-3, which the older 3e-3 refuses as well (printed).  The defect the older
bound passes is half of it -- the same voxel lost for 4 input channels, 2.6e-3 -- and `cmp_f32` fails that one too: asserted."""
import pytest
import torch
import torch.nn.functional as F

from tests import fwd_audit as A
from tests.helpers import bf16_round, formula_input
from tests.test_gpu_ops import CONVT_CASES, HALO3_CASES, _w
from tests.test_gpu_train_ops import S1_CASES
from tests.test_gpu_train_ops import _w as _w_train

F64 = torch.float64
BUDGET = 1 << 30
OLD_REL_L2, OLD_MAX = 3e-3, 2e-2


def _conv(x, wt, transposed):
    if transposed:
        return F.conv_transpose3d(x, wt, None, stride=(1, 2, 2), padding=(1, 1, 1))
    return F.conv3d(x, wt, None, padding=1)


def _build(kind):
    if kind == "narrow_split_k_w24_256_256":       # test_narrow_plane_tiles_split_k
        cin, cout, dims, tr, seeds = 256, 256, (2, 6, 8, 24), False, (1, 3, 4)
    elif kind == "halo_ragged_edges_batch2":        # test_conv3_halo_tile_kernel
        _, cin, _, cout, dims = next(c for c in HALO3_CASES if c[0] == "ragged_edges_batch2")
        tr, seeds = False, (1, 3, 4)
    else:                                           # test_conv_transpose_halo_tile_kernel
        _, cin, cout, dims = next(c for c in CONVT_CASES if c[0] == "ragged_batch2")
        tr, seeds = True, (61, 62, 63)
    n, d, h, w = dims
    x = bf16_round(formula_input((n, cin, d, h, w), seeds[0]))
    wt = bf16_round(_w((cin, cout, 3, 4, 4), seeds[1], transposed=True) if tr else _w((cout, cin, 3, 3, 3), seeds[1]))
    b = formula_input((cout,), seeds[2]) * 0.1
    bias = b.view(1, -1, 1, 1, 1)
    ref = A.conv64(x, wt, (2, 2) if tr else (1, 1), (1, 1, 1), tr, BUDGET) + bias.to(F64)
    acc = (_conv(x, wt, tr) + bias).contiguous()          # exact bf16 products, fp32 sums: a correct kernel's accumulators
    return dict(x=x, wt=wt, bias=bias, ref=ref, acc=acc, tr=tr, cin=cin)


@pytest.fixture(scope="module", params=["narrow_split_k_w24_256_256", "halo_ragged_edges_batch2", "convT_ragged_batch2"])
def case(request):
    return request.param, _build(request.param)


def _one_tap(c, tap, chans=None, shift_w=False):
    """the fp32 contribution of weight tap `tap` (and input channels `chans`) to every output; `shift_w`: computed from the
    input one voxel further along w (what the tap sees when it reads w - 1)"""
    x, wt = c["x"], torch.zeros_like(c["wt"])
    wt[:, :, tap[0], tap[1], tap[2]] = c["wt"][:, :, tap[0], tap[1], tap[2]]
    if chans is not None:
        keep = torch.zeros(c["cin"], dtype=torch.bool)
        keep[chans] = True
        if c["tr"]:
            wt[~keep] = 0
        else:
            wt[:, ~keep] = 0
    if shift_w:
        xs = torch.zeros_like(x)
        xs[..., 1:] = x[..., :-1]
        x = xs
    return _conv(x, wt, c["tr"])


def _defects(c):
    acc, ref, x = c["acc"], c["ref"], c["x"]
    half = c["cin"] // 2
    xh = x.clone()
    xh[:, :half] = 0
    part = _conv(xh, c["wt"], c["tr"])
    out = {"parked_bf16_partial": ((acc - part) + bf16_round(part)).to(torch.bfloat16)}
    # the first corner voxel of the second sample; the centre tap (1, 1, 1) reaches it in the stride-1 and the transposed form
    m = acc.clone()
    m[1, :, 0, 0, 0] -= _one_tap(c, (1, 1, 1), slice(8, 16))[1, :, 0, 0, 0]
    assert not torch.equal(m, acc)
    out["lost_chunk"] = m.to(torch.bfloat16)
    # a voxel of the last (ragged) W column, mid-volume; a tap that reads inside the volume there, shifted or not (transposed
    # form: output row 7 and the last, odd column take the taps kh = kw = 2)
    tap = (1, 2, 2) if c["tr"] else (0, 1, 0)
    m = acc.clone()
    v = (0, slice(None), acc.shape[2] // 2, acc.shape[3] // 2, acc.shape[4] - 1)
    m[v] += _one_tap(c, tap, slice(8, 16), shift_w=True)[v] - _one_tap(c, tap, slice(8, 16))[v]
    assert not torch.equal(m, acc)
    out["tap_reads_w_minus_1"] = m.to(torch.bfloat16)
    good = acc.to(torch.bfloat16)
    out["one_ulp_high"] = (good.to(F64) + A.bf16_ulp(good.to(F64))).to(torch.bfloat16)
    return out


def _old(out, ref):
    err = out.to(F64) - ref
    return float(err.norm() / ref.norm()), float(err.abs().max() / ref.abs().max())


def test_correct_output_passes_and_the_four_defects_fail(case):
    name, c = case
    ref = c["ref"]
    good = A.cmp_bf16(c["acc"].to(torch.bfloat16), ref)
    rel, mx = _old(c["acc"].to(torch.bfloat16), ref)
    print(f"[{name}] correct: old rel-L2 {rel:.2e} max {mx:.2e} | worst/tol {good['ulps']:.2f} rel-L2 vs bf16(ref) {good['rel_l2']:.2e}")
    assert good["ok"] and good["ulps"] <= 1.0, good
    assert rel < OLD_REL_L2 and mx < OLD_MAX
    # the per-element tolerance the cross-form comparisons use is the one cmp_bf16 applies
    tol = A.bf16_tol(ref)
    assert float(((c["acc"].to(torch.bfloat16).to(F64) - ref).abs() / tol).max()) == pytest.approx(good["ulps"], rel=1e-12)
    for dname, out in _defects(c).items():
        res = A.cmp_bf16(out, ref)
        rel, mx = _old(out, ref)
        print(f"[{name}] {dname}: old rel-L2 {rel:.2e} ({'passes' if rel < OLD_REL_L2 else 'fails'}) max {mx:.2e} "
              f"({'passes' if mx < OLD_MAX else 'fails'}) | worst/tol {res['ulps']:.1f} rel-L2 vs bf16(ref) {res['rel_l2']:.2e}")
        assert not res["ok"], (name, dname, res)
        assert not bool(((out.to(F64) - ref).abs() <= tol).all()), (name, dname)
        # the gap: what the three rel-L2-only op tests let through
        if dname == "parked_bf16_partial" or (name == "narrow_split_k_w24_256_256" and dname in ("lost_chunk", "tap_reads_w_minus_1")):
            assert rel < OLD_REL_L2, (name, dname, rel)
        if dname == "one_ulp_high":
            assert rel >= OLD_REL_L2, (name, rel)


def test_weight_gradient_loses_one_voxel_of_eight_channels():
    _, cin, cout, dims, k = next(c for c in S1_CASES if c[0] == "k3_long_k_256_128")
    n, d, h, w = dims
    x = bf16_round(formula_input((n, cin, d, h, w), 1))
    wshape = (cout, cin, k, k, k)
    assert tuple(bf16_round(_w_train(wshape, 2, cin * k ** 3)).shape) == wshape      # (the weights do not enter their own gradient)
    dy = bf16_round(formula_input((n, cout, d, h, w), 3))
    ref = torch.nn.grad.conv3d_weight(x.to(F64), wshape, dy.to(F64), padding=1)
    dw = torch.nn.grad.conv3d_weight(x, wshape, dy, padding=1)              # fp32 sums of exact bf16 products
    good = A.cmp_f32(dw, ref)
    assert good["ok"], good
    dy1 = torch.zeros_like(dy)
    vox = (0, slice(None), d // 2, h // 2, w // 2)
    dy1[vox] = dy[vox]
    print(f"[k3_long_k_256_128] correct: rel-L2 {good['rel_l2']:.2e} max/max|ref| {good['max_rel']:.2e}")
    old = {}
    for lose in (8, 4):
        lost = torch.nn.grad.conv3d_weight(x[:, 8:8 + lose], (cout, lose, k, k, k), dy1, padding=1)
        bad = dw.clone()
        bad[:, 8:8 + lose] -= lost
        res = A.cmp_f32(bad, ref)
        old[lose] = float((bad.to(F64) - ref).norm() / ref.norm())
        print(f"[k3_long_k_256_128] one voxel lost for {lose} input channels: rel-L2 {res['rel_l2']:.2e} max/max|ref| "
              f"{res['max_rel']:.2e} ({'passes' if res['ok'] else 'fails'} cmp_f32), old rel-L2 bound "
              f"{'passes' if old[lose] <= 3e-3 else 'fails'}")
        assert not res["ok"], (lose, res)
    assert old[4] <= 3e-3 < old[8], old
