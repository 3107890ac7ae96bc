"""GPU: the bf16x3 convolution kernel (csrc/conv_bf16x3.hip) through the C ABI.

Per case, on the device: y64 = torch float64, y32 = torch fp32, ys = the three-term split restatement in float64
(tests/x3_restatement.py), ybf = its one-term form conv(xh, wh).  With e32 = rel_l2(y32, y64), e_split = rel_l2(ys, y64):
  1. rel_l2(y, y64) <= e_split + max(4 e32, 2e-7)   the defined arithmetic plus the fp32 mode's allowance for accumulation
  2. rel_l2(y, ys)  <= e_split                      the accumulation error does not exceed the format's own error
  3. rel_l2(y, y64) <= rel_l2(ybf, y64) / 32        about 500 expected; fails any kernel that drops a cross term
  4. a relaunch is bit-identical, output and column sums
  5. the column-sum slab sums to a float64 reduction of y within 1e-5
  6. padding columns of the slab are exactly zero
and one exact case (small integers, weights hi + lo with non-zero lo, an asymmetric pattern) that pins the operand lane maps
and the pairing of the hi / lo terms bit for bit."""
import ctypes as C
import importlib

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import rel_l2
from tests.x3_restatement import conv3d_x3, conv_transpose3d_x3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = importlib.import_module("video-to-video-diffusion_amd.engine")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
FLOOR = 2e-7


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale


def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def run_conv_x3(x1, x2, w, b, *, transposed=False, k=(3, 3, 3), s=(1, 1), p=(1, 1, 1), act=0, residual=None,
                ncdhw_out=False, colsum=False, into=None, c_off=0):
    """x1 / x2 fp32 NCDHW on the device; returns (y NCDHW, colsum slab or None, geometry).  `into`: an fp32 NDHWC buffer with
    more channels than cout; the result goes to its channels [c_off, c_off + cout) and the buffer is returned as it is."""
    lib = E.get_lib()
    ctx = E.Ctx.get(torch.device(DEV))
    n, c1, di, hi, wi = x1.shape
    c2 = 0 if x2 is None else x2.shape[1]
    cout = w.shape[1] if transposed else w.shape[0]
    desc = L.ConvDesc(int(transposed), k[0], k[1], k[2], s[0], s[1], p[0], p[1], p[2], n, c1, c2, cout, di, hi, wi, 0)
    assert lib.conv_bf16x3_supported(C.byref(desc)) == 1, lib.last_error()
    g = [C.c_int() for _ in range(6)]
    lib.conv_bf16x3_geometry(C.byref(desc), *[C.byref(v) for v in g])
    do, ho, wo, tps, ncls, cpad = [v.value for v in g]
    packed = torch.empty(lib.conv_bf16x3_weight_bytes(C.byref(desc)), dtype=torch.uint8, device=DEV)
    a1 = _ndhwc(x1)
    a2 = None if x2 is None else _ndhwc(x2)
    wc = w.contiguous()
    co = L.ConvOut()
    if into is not None:
        y = into
        assert tuple(y.shape[:4]) == (n, do, ho, wo)
        co.mode, co.cout_stride, co.c_off = 0, y.shape[4], c_off
    elif ncdhw_out:
        y = torch.empty((n, cout, do, ho, wo), device=DEV)
        co.mode, (co.sn, co.sc, co.sd, co.sh, co.sw) = 1, y.stride()
    else:
        y = torch.empty((n, do, ho, wo, cout), device=DEV)
        co.mode, co.cout_stride, co.c_off = 0, cout, 0
    co.y = y.data_ptr()
    co.act = act
    cs = torch.zeros(2 * ncls * n * tps * cpad, device=DEV) if colsum else None
    co.colsum = 0 if cs is None else cs.data_ptr()
    res = None
    if residual is not None:
        res = residual.contiguous() if ncdhw_out else _ndhwc(residual)
    torch.cuda.synchronize()
    with ctx.scope():
        lib.conv_bf16x3_pack_weights(C.byref(desc), E._ptr(wc), E._ptr(packed), ctx.sptr)
        lib.conv_bf16x3_fwd(C.byref(desc), E._ptr(a1), E._ptr(a2), E._ptr(packed), E._ptr(b), E._ptr(res), C.byref(co),
                            ctx.sptr)
    torch.cuda.synchronize()
    out = y if (ncdhw_out or into is not None) else y.permute(0, 4, 1, 2, 3).contiguous()
    return out, cs, dict(tps=tps, ncls=ncls, cpad=cpad, cout=cout, n=n)


def _torch_conv(x, w, b, transposed, s, p):
    if transposed:
        return F.conv_transpose3d(x, w, b, stride=(1,) + tuple(s), padding=p)
    return F.conv3d(x, w, b, stride=(1,) + tuple(s), padding=p)


def _split_conv(x, w, b, transposed, s, p, terms):
    fn = conv_transpose3d_x3 if transposed else conv3d_x3
    return fn(x, w, b, stride=(1,) + tuple(s), padding=p, terms=terms)


UPG = dict(transposed=True, k=(3, 4, 4), s=(2, 2))
CONV_CASES = {
    # name: (n, c1, c2, cout, dims, geometry, act, residual): the ten cases of tests/test_gpu_fp32_mode.py ...
    "k333_cat_ragged_res": (2, 24, 13, 40, (5, 9, 11), dict(), 0, True),
    "k333_stem_cin1": (1, 1, 0, 16, (4, 12, 10), dict(), 0, False),
    "k333_head_cout1_tanh": (1, 20, 0, 1, (3, 16, 14), dict(), 1, False),
    "k333_wide": (1, 256, 0, 128, (6, 16, 16), dict(), 0, False),
    "k111_cat": (2, 64, 32, 70, (6, 7, 9), dict(k=(1, 1, 1), p=(0, 0, 0)), 0, False),
    "down_odd": (2, 24, 0, 36, (4, 10, 13), dict(k=(3, 4, 4), s=(2, 2)), 0, False),
    "up_ragged": (2, 20, 0, 12, (3, 5, 7), UPG, 0, False),
    "up_wide": (1, 128, 0, 128, (4, 8, 8), UPG, 0, True),
    "k333_cout200_two_ntiles": (1, 48, 0, 200, (4, 10, 12), dict(), 0, True),
    "up_cout200_two_ntiles": (2, 40, 0, 200, (3, 6, 5), UPG, 0, False),
    # ... and: a source boundary inside an 8-channel vector with cin no multiple of 32; a multiple of 16 but not of the slice
    "k333_cat_20_13": (1, 20, 13, 24, (5, 9, 11), dict(), 0, False),
    "k333_cin48": (1, 48, 0, 64, (4, 8, 8), dict(), 0, False),
}


def _case(name):
    n, c1, c2, cout, dims, geom, act, with_res = CONV_CASES[name]
    tr = geom.get("transposed", False)
    k, s, p = geom.get("k", (3, 3, 3)), geom.get("s", (1, 1)), geom.get("p", (1, 1, 1))
    seed = sum(map(ord, name))
    cin = c1 + c2
    x1 = _randn((n, c1) + dims, seed).to(DEV)
    x2 = _randn((n, c2) + dims, seed + 1).to(DEV) if c2 else None
    fan = cin * k[0] * k[1] * k[2]
    w = _randn((cin, cout) + k if tr else (cout, cin) + k, seed + 2, fan ** -0.5).to(DEV)
    b = _randn((cout,), seed + 3, 0.1).to(DEV)
    return n, cout, tr, k, s, p, act, with_res, seed, x1, x2, w, b


def _references(x1, x2, w, b, tr, s, p, res, act):
    """(y64, y32, ys, ybf): float64 truth, torch fp32, the three-term and the one-term restatement in float64."""
    xcat = x1 if x2 is None else torch.cat([x1, x2], 1)
    x64, w64, b64 = xcat.double(), w.double(), b.double()
    ys = [_torch_conv(x64, w64, b64, tr, s, p), _torch_conv(xcat, w, b, tr, s, p),
          _split_conv(x64, w64, b64, tr, s, p, 3), _split_conv(x64, w64, b64, tr, s, p, 1)]
    if res is not None:
        ys = [y + res.to(y.dtype) for y in ys]
    if act:
        ys = [torch.tanh(y) for y in ys]
    return ys


def _assert_criteria(name, y, y64, y32, ys, ybf):
    e32, e_split, ebf = rel_l2(y32, y64), rel_l2(ys, y64), rel_l2(ybf, y64)
    e, e_acc = rel_l2(y, y64), rel_l2(y, ys)
    print(f"{name}: bf16x3 kernel {e:.3g} (to the restatement {e_acc:.3g} = {e_acc / e_split:.3f} x e_split), "
          f"restatement {e_split:.3g}, torch fp32 {e32:.3g}, one-term bf16 {ebf:.3g} (ratio {ebf / e:.0f})")
    assert e <= e_split + max(4.0 * e32, FLOOR), f"{name}: {e:.3g} > {e_split:.3g} + max(4 x {e32:.3g}, {FLOOR})"
    assert e_acc <= e_split, f"{name}: accumulation error {e_acc:.3g} above the split's own {e_split:.3g}"
    assert e <= ebf / 32.0, f"{name}: {e:.3g} > one-term bf16 {ebf:.3g} / 32"


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_bf16x3_against_float64(name):
    n, cout, tr, k, s, p, act, with_res, seed, x1, x2, w, b = _case(name)
    y64 = _torch_conv((x1 if x2 is None else torch.cat([x1, x2], 1)).double(), w.double(), b.double(), tr, s, p)
    res = _randn(tuple(y64.shape), seed + 4).to(DEV) if with_res else None
    y64, y32, ys, ybf = _references(x1, x2, w, b, tr, s, p, res, act)
    ncdhw = bool(act)
    kw = dict(transposed=tr, k=k, s=s, p=p, act=act, residual=res, ncdhw_out=ncdhw, colsum=True)
    y, cs, geo = run_conv_x3(x1, x2, w, b, **kw)
    assert tuple(y.shape) == tuple(y64.shape)
    _assert_criteria(name, y, y64, y32, ys, ybf)
    # a relaunch is bit-identical (output and column sums)
    y2, cs2, _ = run_conv_x3(x1, x2, w, b, **kw)
    assert torch.equal(y, y2) and torch.equal(cs, cs2)
    # column sums: per (sample, channel) totals over every tile (and parity class) against a float64 reduction of y
    tps, ncls, cpad = geo["tps"], geo["ncls"], geo["cpad"]
    slab = cs.view(2, ncls, n, tps, cpad).double()
    tot = slab.sum(dim=(1, 3))[:, :, :cout]                               # [2][n][cout]
    yd = y.double().reshape(n, cout, -1)
    ref = torch.stack([yd.sum(-1), (yd * yd).sum(-1)])
    assert rel_l2(tot[0], ref[0]) < 1e-5 and rel_l2(tot[1], ref[1]) < 1e-5
    assert float(slab[:, :, :, :, cout:].abs().max() if cpad > cout else 0.0) == 0.0


def test_store_at_a_channel_offset_keeps_the_other_channels():
    name = "k333_cat_20_13"
    n, cout, tr, k, s, p, act, _, seed, x1, x2, w, b = _case(name)
    y64, y32, ys, ybf = _references(x1, x2, w, b, tr, s, p, None, act)
    wide, c_off = cout + 19, 7
    fill = _randn((n,) + tuple(y64.shape[2:]) + (wide,), seed + 9).to(DEV)
    buf = fill.clone()
    run_conv_x3(x1, x2, w, b, into=buf, c_off=c_off)
    y = buf[..., c_off:c_off + cout].permute(0, 4, 1, 2, 3)
    _assert_criteria(name + "@offset", y, y64, y32, ys, ybf)
    plain, _, _ = run_conv_x3(x1, x2, w, b)
    assert torch.equal(y, plain)                      # the same bits as the dense store
    keep = torch.ones(wide, dtype=torch.bool, device=DEV)
    keep[c_off:c_off + cout] = False
    assert torch.equal(buf[..., keep].view(torch.int32), fill[..., keep].view(torch.int32))


def _grid(shape):
    return torch.meshgrid(*[torch.arange(v, dtype=torch.int64) for v in shape], indexing="ij")


@pytest.mark.parametrize("lo_in", ["w", "x"])
@pytest.mark.parametrize("geom", ["k333", "up"])
def test_exact_small_integers_pin_the_lane_maps(lo_in, geom):
    """Values i + 2^-10 m (i a small integer, m in 0..3) are hi + lo exactly, with lo != 0 for most; the other operand holds
    small integers (lo = 0), so every kept product and every partial sum is a multiple of 2^-10 below 2^14: exact in fp32, and
    the dropped product is zero.  The result must be the float64 convolution, bit for bit.  The patterns depend on every
    index with different coefficients (nothing symmetric in rows / columns / k), once with the lo parts in w and once in x."""
    tr = geom == "up"
    n, c1, c2, cout, dims = 2, 12, 9, 40, (3, 6, 7)
    k, s, p = ((3, 4, 4), (2, 2), (1, 1, 1)) if tr else ((3, 3, 3), (1, 1), (1, 1, 1))
    cin = c1 + c2
    bi, ci, d, h, w_ = _grid((n, cin) + dims)
    xi = (3 * bi + 5 * ci + 7 * d + 11 * h + 13 * w_) % 9 - 4
    xm = (bi + 2 * ci + 3 * d + h + 5 * w_) % 4
    wshape = (cin, cout) + k if tr else (cout, cin) + k
    a, b_, kd, kh, kw = _grid(wshape)
    wi = (2 * a + 7 * b_ + 3 * kd + 5 * kh + 11 * kw) % 7 - 3
    wm = (3 * a + b_ + 2 * kd + 7 * kh + kw) % 4
    x = xi.double() + (xm.double() * 2.0 ** -10 if lo_in == "x" else 0.0)
    w = wi.double() + (wm.double() * 2.0 ** -10 if lo_in == "w" else 0.0)
    bias = (torch.arange(cout, dtype=torch.float64) % 5 - 2) * 0.25
    x32, w32, b32 = x.float().to(DEV), w.float().to(DEV), bias.float().to(DEV)
    assert torch.equal(x32.double().cpu(), x) and torch.equal(w32.double().cpu(), w)
    lo_t = (w32 if lo_in == "w" else x32)
    assert int((lo_t - lo_t.to(torch.bfloat16).float() != 0).sum()) > lo_t.numel() // 2       # the lo parts are there
    y64 = _torch_conv(x32.double(), w32.double(), b32.double(), tr, s, p)
    assert torch.equal(y64.float().double(), y64)                  # representable: the comparison below is exact
    y, _, _ = run_conv_x3(x32[:, :c1].contiguous(), x32[:, c1:].contiguous(), w32, b32, transposed=tr, k=k, s=s, p=p)
    bad = int((y.double() != y64).sum())
    assert bad == 0, f"{bad} of {y.numel()} outputs differ; max |diff| {float((y.double() - y64).abs().max()):.3g}"
