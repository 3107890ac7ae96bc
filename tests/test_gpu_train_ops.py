"""GPU: the training-path kernels (weight gradient, data gradient through the forward kernels, GroupNorm backward,
loss, q_sample, small Linear backward) against torch autograd in fp32 on the same bf16-rounded operands.

 wgrad / dgrad     rel-L2 <= 3e-3   (fp32 accumulate of bf16 products), and against float64 from the same operands: the weight
                   gradient in the f32 class (F32_REL_L2 / F32_MAX_REL of tests/train_audit.py, every forced form), the data
                   gradient's conv launch under the forward audit (tests/fwd_audit.py: one bf16 ulp per element)
 GroupNorm bwd     rel-L2 <= 8e-3   (bf16 in / out, fp32 statistics; g is rounded to bf16 between the two passes)
 fp32-only ops     rel-L2 <= 1e-5
"""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import bf16_round, formula_input, rel_l2
from tests.train_audit import cmp_f32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_DW64 = {}            # float64 weight gradients, shared by the tests and forced forms of one case


@pytest.fixture(scope="module")
def G():
    from tests import gpu_utils
    return gpu_utils


def _w(shape, k, fan):
    return formula_input(shape, k) * (1.5 / math.sqrt(fan))


def _ndhwc_bf16(G, prog, x):
    return G.to_act(prog, x)


def _wgrad(G, r, g, k, s, p, n_taps_shape, out_shape, stride_rgt, c_off_elems=0, dw=None):
    """Run ctsi_wgrad for R = r (NCDHW fp32), G = g; returns the dw tensor (device)."""
    E, L = G.E, importlib.import_module("video-to-video-diffusion_amd.lib")
    c = G.ctx()
    with c.scope():
        prog = E.Program(c)
        ar, ag = G.to_act(prog, r), G.to_act(prog, g)
        desc = L.WgradDesc(k[0], k[1], k[2], s[0], s[1], p[0], p[1], p[2], ar.n, ar.d, ar.h, ar.w, ag.d, ag.h, ag.w,
                           ar.c, ar.c, ag.c, ag.c)
        ws = torch.empty(max(c.lib.wgrad_workspace_bytes(C.byref(desc)), 16), dtype=torch.uint8, device=DEV)
        if dw is None:
            dw = torch.full(out_shape, float("nan"), dtype=torch.float32, device=DEV)
        c.lib.wgrad(C.byref(desc), ar.ip, ag.ip, G._ptr(ws), ws.numel(), C.c_void_p(dw.data_ptr() + 4 * c_off_elems), stride_rgt[0],
                    stride_rgt[1], stride_rgt[2], 1.0, c.sptr)
    torch.cuda.synchronize()
    return dw


def _dw64(key, x, dy, wshape, k, s, p, transposed=False):
    """float64 autograd weight gradient from the same bf16-rounded operands (on the device, MIOpen off), computed once per `key`"""
    if key not in _DW64:
        with torch.backends.cudnn.flags(enabled=False):
            xd, gd = x.detach().to(DEV, torch.float64), dy.to(DEV, torch.float64)
            wz = torch.zeros(wshape, dtype=torch.float64, device=DEV, requires_grad=True)
            fn = F.conv_transpose3d if transposed else F.conv3d
            (g,) = torch.autograd.grad(fn(xd, wz, None, stride=(1,) + tuple(s), padding=tuple(p)), wz, gd)
        _DW64[key] = g.cpu()
    return _DW64[key]


def _dw_f32_class(label, dw, ref64):
    """The weight gradient is an fp32 accumulation of exact bf16 products: F32_REL_L2 / F32_MAX_REL (1e-4 / 1e-3) against float64,
    the bounds tests/train_audit.py holds the same kernels to at the programs' shapes.  Every entry was written (no NaN left)."""
    got = dw.detach().cpu()
    assert torch.isfinite(got).all(), label
    res = cmp_f32(got, ref64)
    print(f"[conv-op-audit] {label} | wgrad | dW {'x'.join(str(v) for v in got.shape)} | f32 | rel-L2 {res['rel_l2']:.3e} | "
          f"max/max|ref| {res['max_rel']:.3e} | worst/tol - | {'ok' if res['ok'] else 'FAIL'}")
    assert res["ok"], (label, res)


WG_CASES = [
    # name, cin, cout, (n,d,h,w) of the layer input, kind
    ("k3_128_128", 128, 128, (1, 4, 6, 6), "k3"),
    ("k3_batch2_odd_64_192", 64, 192, (2, 3, 7, 9), "k3"),
    ("k3_cout8_head", 128, 8, (1, 3, 6, 6), "k3"),
    ("k3_cin16_stem", 16, 128, (2, 4, 5, 6), "k3"),
    ("k1_256_64", 256, 64, (1, 2, 6, 6), "k1"),
    ("down_64", 64, 64, (1, 3, 8, 12), "down"),
    ("down_128_odd_batch2", 128, 128, (2, 3, 10, 6), "down"),
    ("convT_64", 64, 64, (1, 3, 4, 5), "up"),
    ("convT_256_128_batch2", 256, 128, (2, 2, 5, 4), "up"),
]


@pytest.mark.parametrize("name,cin,cout,dims,kind", WG_CASES, ids=[c[0] for c in WG_CASES])
def test_wgrad_and_dgrad_vs_autograd(G, name, cin, cout, dims, kind):
    n, d, h, w = dims
    x = bf16_round(formula_input((n, cin, d, h, w), 1)).requires_grad_(True)
    if kind == "k3":
        k, s, p = (3, 3, 3), (1, 1), (1, 1, 1)
        wt = bf16_round(_w((cout, cin, 3, 3, 3), 2, cin * 27)).requires_grad_(True)
        y = F.conv3d(x, wt, None, padding=1)
    elif kind == "k1":
        k, s, p = (1, 1, 1), (1, 1), (0, 0, 0)
        wt = bf16_round(_w((cout, cin, 1, 1, 1), 2, cin)).requires_grad_(True)
        y = F.conv3d(x, wt, None)
    elif kind == "down":
        k, s, p = (3, 4, 4), (2, 2), (1, 1, 1)
        wt = bf16_round(_w((cout, cin, 3, 4, 4), 2, cin * 48)).requires_grad_(True)
        y = F.conv3d(x, wt, None, stride=(1, 2, 2), padding=1)
    else:
        k, s, p = (3, 4, 4), (2, 2), (1, 1, 1)
        wt = bf16_round(_w((cin, cout, 3, 4, 4), 2, cin * 12)).requires_grad_(True)
        y = F.conv_transpose3d(x, wt, None, stride=(1, 2, 2), padding=1)
    dy = bf16_round(formula_input(tuple(y.shape), 3))
    y.backward(dy)
    T = k[0] * k[1] * k[2]
    # ---- weight gradient ----
    if kind == "up":   # R = layer input, G = dy; weight (cin, cout, T)
        dw = _wgrad(G, x.detach(), dy, k, s, p, T, tuple(wt.shape), (cout * T, T, 1))
    else:              # R = dy, G = layer input; weight (cout, cin, T)
        dw = _wgrad(G, dy, x.detach(), k, s, p, T, tuple(wt.shape), (cin * T, T, 1))
    e_w = rel_l2(dw.cpu(), wt.grad)
    _dw_f32_class(f"wgrad[{name}]", dw, _dw64(("wg", name), x, dy, tuple(wt.shape), k, s, p, kind == "up"))
    # ---- data gradient through the forward conv kernels ----
    c = G.ctx()
    if kind in ("k3", "k1"):
        wd = torch.empty((cin, cout) + tuple(wt.shape[2:]), dtype=torch.float32, device=DEV)
        wsrc = wt.detach().to(DEV).contiguous()
        with c.scope():
            c.lib.weight_dgrad_layout(G._ptr(wsrc), G._ptr(wd), cout, cin, T, 0, cin, c.sptr)
        torch.cuda.synchronize()
        dx, _, _ = G.run_conv(dy, None, wd.cpu(), None, k=k, s=s, p=p, audit=True)
    elif kind == "down":   # data gradient of the strided conv = ConvTranspose3d with the same weight tensor
        dx, _, _ = G.run_conv(dy, None, wt.detach(), None, transposed=True, k=k, s=s, p=p, audit=True)
    else:                  # data gradient of the ConvTranspose3d = strided Conv3d with the same weight tensor
        dx, _, _ = G.run_conv(dy, None, wt.detach(), None, k=k, s=s, p=p, audit=True)
    e_x = rel_l2(dx, x.grad)
    print(f"{name}: wgrad rel-L2 {e_w:.2e}, dgrad rel-L2 {e_x:.2e}")
    assert tuple(dx.shape) == tuple(x.shape)
    assert e_w <= 3e-3 and e_x <= 3e-3


S1_CASES = [
    # name, cin, cout, (n,d,h,w), k
    ("k3_128_128", 128, 128, (1, 4, 6, 6), 3),
    ("k3_batch2_odd_64_192", 64, 192, (2, 3, 7, 9), 3),
    ("k3_cin16_stem", 16, 128, (2, 4, 5, 6), 3),
    ("k3_long_k_256_128", 256, 128, (1, 6, 20, 24), 3),       # several split-K slices, W rows that straddle K-steps
    ("k1_256_64", 256, 64, (1, 2, 6, 6), 1),
]


@pytest.mark.parametrize("name,cin,cout,dims,k", S1_CASES, ids=[c[0] for c in S1_CASES])
def test_wgrad_tap_sharing_kernel(G, monkeypatch, name, cin, cout, dims, k):
    """conv_wgrad_s1_kernel<TG, BK> (one R slab + one halo'd G slab serve the 3 kw taps of a (kd, kh) row; K-steps of 64 voxels)
    against autograd, and run-to-run bit-identical."""
    n, d, h, w = dims
    x = bf16_round(formula_input((n, cin, d, h, w), 1)).requires_grad_(True)
    kk, pp = (k, k, k), (k // 2, k // 2, k // 2)
    wt = bf16_round(_w((cout, cin, k, k, k), 2, cin * k ** 3)).requires_grad_(True)
    y = F.conv3d(x, wt, None, padding=k // 2)
    dy = bf16_round(formula_input(tuple(y.shape), 3))
    y.backward(dy)
    T = k ** 3
    monkeypatch.setenv("CTSI_WGRAD_S1", "64")
    monkeypatch.setenv("CTSI_WGRAD_HALO", "0")          # (the halo-tile kernel would take the well-fitting 3x3x3 cases)
    dw = _wgrad(G, dy, x.detach(), kk, (1, 1), pp, T, tuple(wt.shape), (cin * T, T, 1))
    assert rel_l2(dw.cpu(), wt.grad) <= 3e-3, name
    _dw_f32_class(f"wgrad-s1[{name}]", dw, _dw64(("s1", name), x, dy, tuple(wt.shape), kk, (1, 1), pp))
    dw2 = _wgrad(G, dy, x.detach(), kk, (1, 1), pp, T, tuple(wt.shape), (cin * T, T, 1))
    assert torch.equal(dw, dw2)


HALO_WG_CASES = [
    # name, cin, cout, (n,d,h,w), expected tile code (1: 3x8x8, 2: 6x4x8, 3: 3x4x16, 4: 4x4x12, 5: 8x6x4)
    ("aligned_128_128", 128, 128, (1, 6, 8, 16), 1),
    ("batch2_ragged_64_192", 64, 192, (2, 5, 16, 24), 1),           # D = 5: ragged depth tiles; two cout tiles (192 of 256)
    ("cin16_cout72", 16, 72, (1, 3, 8, 8), 1),
    ("tile_3x4x16", 32, 128, (1, 3, 4, 32), 3),
    ("tile_6x4x8", 32, 64, (1, 6, 4, 16), 2),
    ("ragged_planes_12x12", 64, 128, (1, 6, 12, 12), 2),            # 12-wide planes: W tiles of 8 cover 16 (75 %)
    ("tile_4x4x12", 64, 128, (1, 8, 12, 12), 4),                     # 12-wide planes at 100 %: blocks of 4 voxels straddle lines
    ("tile_4x4x12_w24_batch2", 32, 64, (2, 4, 8, 24), 4),
    ("tile_8x6x4_6wide_planes", 128, 128, (2, 16, 6, 6), 5),        # the 6 x 6 level of config 3
    ("multi_slice_256_256", 256, 256, (1, 12, 16, 16), 1),          # several voxel-tile slices per (chunk, cout tile)
    ("config3_level_shape", 128, 128, (2, 6, 24, 24), 1),
]


@pytest.mark.parametrize("name,cin,cout,dims,code", HALO_WG_CASES, ids=[c[0] for c in HALO_WG_CASES])
def test_wgrad_halo_tile_kernel(G, monkeypatch, name, cin, cout, dims, code):
    """conv_wgrad_halo_kernel (csrc/conv_wgrad_halo.hip: one 16-cin chunk x 128 couts x all 27 taps per block over voxel
    tiles, X halo tile + dY tile in LDS, transposing reads) against autograd, against the one-tap kernel, run-to-run
    bit-identical; zero padding at the volume faces comes from the DMA's zero fill (no masks): checked by the ragged cases."""
    n, d, h, w = dims
    lib = G.ctx().lib
    plan = lib._dll.ctsi_wgrad_halo_plan
    plan.restype = C.c_int
    S, ws = C.c_int(), C.c_size_t()
    assert plan(n, d, h, w, cin, cout, C.byref(S), C.byref(ws), None, None) == code and ws.value > 0
    x = bf16_round(formula_input((n, cin, d, h, w), 1)).requires_grad_(True)
    wt = bf16_round(_w((cout, cin, 3, 3, 3), 2, cin * 27)).requires_grad_(True)
    y = F.conv3d(x, wt, None, padding=1)
    dy = bf16_round(formula_input(tuple(y.shape), 3))
    y.backward(dy)
    args = (G, dy, x.detach(), (3, 3, 3), (1, 1), (1, 1, 1), 27, tuple(wt.shape), (cin * 27, 27, 1))
    dw = _wgrad(*args)
    e = rel_l2(dw.cpu(), wt.grad)
    print(f"{name}: halo-tile wgrad rel-L2 {e:.2e} (S = {S.value})")
    assert torch.isfinite(dw).all() and e <= 3e-3, name
    ref64 = _dw64(("halo", name), x, dy, tuple(wt.shape), (3, 3, 3), (1, 1), (1, 1, 1))
    _dw_f32_class(f"wgrad-halo[{name}] S={S.value}", dw, ref64)
    assert torch.equal(dw, _wgrad(*args))
    monkeypatch.setenv("CTSI_WGRAD_REDUCE_T", "0")         # the one-thread-per-output reduce pass: same sums, other order
    dw_t0 = _wgrad(*args)
    assert rel_l2(dw.cpu(), dw_t0.cpu()) <= 1e-6
    _dw_f32_class(f"wgrad-halo[{name}] reduce_t=0", dw_t0, ref64)
    monkeypatch.delenv("CTSI_WGRAD_REDUCE_T")
    monkeypatch.setenv("CTSI_WGRAD_HALO", "0")
    dw_old = _wgrad(*args)
    assert rel_l2(dw.cpu(), dw_old.cpu()) <= 1e-3          # same products, other summation order
    _dw_f32_class(f"wgrad-halo[{name}] halo=0", dw_old, ref64)
    # exactness: dY = one-hot in (voxel, cout) picks X's 27 neighbours of that voxel -- incl. the zero padding at a face
    monkeypatch.delenv("CTSI_WGRAD_HALO")
    dy1 = torch.zeros_like(dy)
    dy1[0, 0, 0, 0, w - 1] = 1.0                           # a corner voxel of the volume
    dw1 = _wgrad(G, dy1, x.detach(), (3, 3, 3), (1, 1), (1, 1, 1), 27, tuple(wt.shape), (cin * 27, 27, 1)).cpu()
    xp = F.pad(x.detach(), (1, 1, 1, 1, 1, 1))
    expect = xp[0, :, 0:3, 0:3, w - 1:w + 2]                # (cin, 3, 3, 3) window around the corner voxel
    assert torch.equal(dw1[0].reshape(cin, 3, 3, 3), expect) and float(dw1[1:].abs().max()) == 0.0


@pytest.mark.parametrize("name,cin,cout,dims,kind", WG_CASES, ids=[c[0] for c in WG_CASES])
def test_wgrad_mfma_16x16x32_form(G, monkeypatch, name, cin, cout, dims, kind):
    """conv_wgrad_kernel<SHAPE16>: the one-tap-per-block kernel on v_mfma_f32_16x16x32_bf16 -- every layer kind, against
    the 32x32x16 form (same products, another summation tree: fp32 rounding only) and autograd."""
    n, d, h, w = dims
    x = bf16_round(formula_input((n, cin, d, h, w), 1)).requires_grad_(True)
    if kind in ("k3", "k1"):
        kk = 3 if kind == "k3" else 1
        k, s, p = (kk, kk, kk), (1, 1), (kk // 2, kk // 2, kk // 2)
        wt = bf16_round(_w((cout, cin, kk, kk, kk), 2, cin * kk ** 3)).requires_grad_(True)
        y = F.conv3d(x, wt, None, padding=kk // 2)
    elif kind == "down":
        k, s, p = (3, 4, 4), (2, 2), (1, 1, 1)
        wt = bf16_round(_w((cout, cin, 3, 4, 4), 2, cin * 48)).requires_grad_(True)
        y = F.conv3d(x, wt, None, stride=(1, 2, 2), padding=1)
    else:
        k, s, p = (3, 4, 4), (2, 2), (1, 1, 1)
        wt = bf16_round(_w((cin, cout, 3, 4, 4), 2, cin * 12)).requires_grad_(True)
        y = F.conv_transpose3d(x, wt, None, stride=(1, 2, 2), padding=1)
    dy = bf16_round(formula_input(tuple(y.shape), 3))
    y.backward(dy)
    T = k[0] * k[1] * k[2]
    res = []
    for shape16 in ("0", "1"):
        monkeypatch.setenv("CTSI_WGRAD_SHAPE16", shape16)
        monkeypatch.setenv("CTSI_WGRAD_HALO", "0")
        if kind == "up":
            res.append(_wgrad(G, x.detach(), dy, k, s, p, T, tuple(wt.shape), (cout * T, T, 1)))
        else:
            res.append(_wgrad(G, dy, x.detach(), k, s, p, T, tuple(wt.shape), (cin * T, T, 1)))
    assert rel_l2(res[1].cpu(), wt.grad) <= 3e-3, name
    assert rel_l2(res[1].cpu(), res[0].cpu()) <= 1e-5
    ref64 = _dw64(("wg", name), x, dy, tuple(wt.shape), k, s, p, kind == "up")
    for shape16 in (0, 1):
        _dw_f32_class(f"wgrad-shape16={shape16}[{name}]", res[shape16], ref64)


def test_wgrad_two_sources_and_split_k(G):
    """A concatenated input is two calls that write disjoint input-channel slices of one weight gradient; a long
    voxel range exercises several split-K slices (fixed summation order: two runs are bit-identical)."""
    n, c1, c2, cout, d, h, w = 1, 64, 32, 64, 6, 20, 24
    x1 = bf16_round(formula_input((n, c1, d, h, w), 1))
    x2 = bf16_round(formula_input((n, c2, d, h, w), 4))
    xx = torch.cat([x1, x2], 1).requires_grad_(True)
    wt = bf16_round(_w((cout, c1 + c2, 3, 3, 3), 2, (c1 + c2) * 27)).requires_grad_(True)
    y = F.conv3d(xx, wt, None, padding=1)
    dy = bf16_round(formula_input(tuple(y.shape), 3))
    y.backward(dy)
    T, cin = 27, c1 + c2
    dw = torch.full(tuple(wt.shape), float("nan"), dtype=torch.float32, device=DEV)
    _wgrad(G, dy, x1, (3, 3, 3), (1, 1), (1, 1, 1), T, None, (cin * T, T, 1), 0, dw)
    # the first call wrote its own input-channel slice of every row and nothing else: the rest is still the NaN pre-fill
    assert torch.isfinite(dw[:, :c1]).all() and torch.isnan(dw[:, c1:]).all()
    first = dw[:, :c1].clone()
    _wgrad(G, dy, x2, (3, 3, 3), (1, 1), (1, 1, 1), T, None, (cin * T, T, 1), c1 * T, dw)
    assert torch.equal(dw[:, :c1], first)                  # ... and the second call left that slice alone
    assert rel_l2(dw.cpu(), wt.grad) <= 3e-3
    _dw_f32_class("wgrad[two_sources_split_k]", dw, _dw64(("two", 0), xx, dy, tuple(wt.shape), (3, 3, 3), (1, 1), (1, 1, 1)))
    dw2 = torch.empty_like(dw)
    _wgrad(G, dy, x1, (3, 3, 3), (1, 1), (1, 1, 1), T, None, (cin * T, T, 1), 0, dw2)
    _wgrad(G, dy, x2, (3, 3, 3), (1, 1), (1, 1, 1), T, None, (cin * T, T, 1), c1 * T, dw2)
    assert torch.equal(dw, dw2)


GN_CASES = [
    # name, c, groups, dims, silu_pre, residual, silu_post, bcast, add
    ("conv3dblock_silu_tbias", 128, 8, (2, 3, 6, 5), True, False, False, False, False),
    ("resblock_tail_residual_silu", 64, 32, (1, 4, 5, 7), False, True, True, False, False),
    ("attention_norm_bcast_add", 256, 32, (2, 3, 4, 4), False, False, False, True, True),
    ("head_silu_c32", 32, 8, (1, 2, 9, 8), True, False, False, False, False),
    ("wide_512", 512, 32, (1, 2, 4, 4), True, False, False, False, False),
    # the remaining instantiations of gn_bwd_reduce_kernel<SILU_PRE, RES, SILU_POST> and of gn_bwd_apply_kernel<ADD>
    ("silu_pre_residual", 64, 8, (1, 3, 5, 6), True, True, False, False, False),
    ("silu_pre_residual_silu_post_add", 64, 8, (2, 2, 6, 5), True, True, True, False, True),
    ("silu_pre_silu_post", 128, 16, (1, 2, 5, 4), True, False, True, False, False),
    ("plain_residual_add", 64, 8, (1, 3, 4, 6), False, True, False, False, True),
    ("silu_post_only", 64, 8, (1, 2, 6, 6), False, False, True, False, False),
    ("c192_24_chunks_per_row", 192, 8, (1, 3, 6, 7), True, False, False, False, True),
    ("c384_grid_stride", 384, 32, (1, 6, 24, 24), True, False, False, False, False),
    ("c512_6x6_plane_batch4_small_tiles", 512, 32, (4, 12, 6, 6), True, False, False, False, False),
    ("c256_12x12_bcast_small_tiles", 256, 32, (2, 8, 12, 12), False, False, False, True, True),
]


@pytest.mark.parametrize("name,c,groups,dims,silu_pre,res,silu_post,bcast,add", GN_CASES, ids=[g[0] for g in GN_CASES])
def test_gn_backward_vs_autograd(G, name, c, groups, dims, silu_pre, res, silu_post, bcast, add):
    E = G.E
    n, d, h, w = dims
    x = (bf16_round(formula_input((n, c, d, h, w), 1) * 1.5 + 0.3)).requires_grad_(True)
    gamma = (1.0 + 0.3 * formula_input((c,), 5)).requires_grad_(True)
    beta = (0.2 * formula_input((c,), 6)).requires_grad_(True)
    tb = (0.5 * formula_input((n, c), 7)).requires_grad_(True)
    r = bf16_round(formula_input((n, c, d, h, w), 8)).requires_grad_(True) if res else None
    hh = F.group_norm(x, groups, gamma, beta, 1e-5)
    a = F.silu(hh) if silu_pre else hh
    use_tb = not res and not bcast and not silu_post   # (ctsi_gn_bwd takes no time bias: the engine never has one before a second SiLU)
    if use_tb:
        a = a + tb[:, :, None, None, None]
    if res:
        a = a + r
    y = F.silu(a) if silu_post else a
    dshape = (n, c, 1, h, w) if bcast else (n, c, d, h, w)
    dy = bf16_round(formula_input(dshape, 9))
    y.backward(dy.expand_as(y).contiguous())
    addt = bf16_round(formula_input((n, c, d, h, w), 10)) if add else None

    cx = G.ctx()
    with cx.scope():
        prog = E.Program(cx)
        ax = G.to_act(prog, x.detach())
        ady = G.to_act(prog, dy)
        ar = G.to_act(prog, r.detach()) if res else None
        aadd = G.to_act(prog, addt) if add else None
        prog.zero_gn_op()
        st = prog.gn_colsum(ax)
        slot = prog.gn_finalize(ax, groups, st)
        prog.finalize_layout()
        prog.run()
        gbuf = torch.empty_like(ax.t)
        dx = torch.empty_like(ax.t)
        ws = torch.empty(cx.lib.gn_bwd_workspace_floats(n, c, d, h, w, groups), dtype=torch.float32, device=DEV)
        dgam = torch.empty(c, dtype=torch.float32, device=DEV)
        dbet = torch.empty(c, dtype=torch.float32, device=DEV)
        dtb = torch.zeros(n, c + 3, dtype=torch.float32, device=DEV)
        dxs = torch.empty(c, dtype=torch.float32, device=DEV)
        gam_d, bet_d = gamma.detach().to(DEV), beta.detach().to(DEV)
        cx.lib.gn_bwd(ax.ip, ady.ip, int(bcast), C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), G._ptr(gam_d),
                      G._ptr(bet_d), n, c, d, h, w, groups, 1e-5, int(silu_pre), ar.ip if res else None, int(silu_post),
                      aadd.ip if add else None, G._ptr(gbuf), G._ptr(dx), G._ptr(ws), G._ptr(dgam), G._ptr(dbet),
                      G._ptr(dtb), c + 3, G._ptr(dxs), cx.sptr)
        dx_f = G.from_act(prog, E.Act(dx, n, c, d, h, w))
        g_f = G.from_act(prog, E.Act(gbuf, n, c, d, h, w))
        if not res and not silu_post:
            # without a buffer for the GroupNorm output's gradient pass 3 re-derives it from dy (what the training engine does
            # wherever nothing else needs that gradient): same dx bit for bit, same parameter gradients
            dx2, dgam2, dbet2 = torch.empty_like(dx), torch.empty_like(dgam), torch.empty_like(dbet)
            cx.lib.gn_bwd(ax.ip, ady.ip, int(bcast), C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), G._ptr(gam_d),
                          G._ptr(bet_d), n, c, d, h, w, groups, 1e-5, int(silu_pre), None, 0, aadd.ip if add else None, None,
                          G._ptr(dx2), G._ptr(ws), G._ptr(dgam2), G._ptr(dbet2), G._ptr(dtb), c + 3, G._ptr(dxs), cx.sptr)
            torch.cuda.synchronize()
            assert torch.equal(dx2.view(torch.int16), dx.view(torch.int16)) and torch.equal(dgam2, dgam) and torch.equal(dbet2, dbet)
    torch.cuda.synchronize()
    want_dx = x.grad + (addt if add else 0.0)
    e_dx = rel_l2(dx_f.cpu(), want_dx)
    e_g, e_b = rel_l2(dgam.cpu(), gamma.grad), rel_l2(dbet.cpu(), beta.grad)
    print(f"{name}: dx {e_dx:.2e} dgamma {e_g:.2e} dbeta {e_b:.2e}")
    assert e_dx <= 8e-3 and e_g <= 5e-3 and e_b <= 5e-3
    # bias gradient of the producing conv = sum of dx over samples and voxels (fp32, from the statistics)
    want_b = x.grad.sum(dim=(0, 2, 3, 4))
    assert float((dxs.cpu() - want_b).norm()) <= 5e-3 * float(x.grad.abs().sum(dim=(0, 2, 3, 4)).norm())
    if res and not silu_pre:
        assert rel_l2(g_f.cpu(), r.grad) <= 8e-3     # g_buf doubles as the residual's gradient (g = gc without a SiLU before the add)
    if use_tb:
        assert rel_l2(dtb[:, :c].cpu(), tb.grad) <= 5e-3


def test_batched_small_linear_gradients(G):
    """ctsi_linear_wgrad_multi: weight and bias gradients of several small pointwise layers in one launch (the attention
    projections of the training path), against fp32 torch on the same bf16 operands: ragged row counts, channel counts that
    are not multiples of the 64 x 64 tile, a scaled bias gradient, a dW with a wider row stride, a layer without bias."""
    import struct
    cx = G.ctx()
    specs = [(300, 256, 256, 256, 1.0, True), (77, 72, 40, 96, 48.0, True), (1000, 512, 128, 512, 1.0, False)]   # rows, cin, cout, dw_stride, b_scale, bias
    ents, blks, keep, want = [], [], [], []
    for i, (rows, cin, cout, dws, bsc, has_b) in enumerate(specs):
        x = bf16_round(formula_input((rows, cin), 30 + i))
        dy = bf16_round(formula_input((rows, cout), 40 + i))
        xd, dyd = x.to(DEV).to(torch.bfloat16).contiguous(), dy.to(DEV).to(torch.bfloat16).contiguous()
        dw = torch.full((cout, dws), float("nan"), dtype=torch.float32, device=DEV)
        db = torch.full((cout,), float("nan"), dtype=torch.float32, device=DEV)
        keep += [xd, dyd, dw, db]
        ents.append(struct.pack("<QQQQiiiifi", xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr() if has_b else 0, rows, cin,
                                cout, dws, bsc, 0))
        for ct in range((cout + 63) // 64):
            for it in range((cin + 63) // 64):
                blks.append(struct.pack("<iiii", i, ct, it, 0))
        want.append((dy.double().t() @ x.double(), dy.double().sum(0) * bsc, dw, db, cin, has_b))
    et = torch.frombuffer(bytearray(b"".join(ents)), dtype=torch.uint8).to(DEV)
    bt = torch.frombuffer(bytearray(b"".join(blks)), dtype=torch.uint8).to(DEV)
    with cx.scope():
        cx.lib.linear_wgrad_multi(G._ptr(et), G._ptr(bt), len(blks), cx.sptr)
        cx.lib.linear_wgrad_multi(G._ptr(et), G._ptr(bt), len(blks), cx.sptr)      # written, not accumulated: a second launch changes nothing
    torch.cuda.synchronize()
    for w_ref, b_ref, dw, db, cin, has_b in want:
        assert rel_l2(dw[:, :cin].cpu().double(), w_ref) < 1e-5
        assert torch.isnan(dw[:, cin:]).all()                      # columns beyond cin untouched
        if has_b:
            assert rel_l2(db.cpu().double(), b_ref) < 1e-5
        else:
            assert torch.isnan(db).all()


def test_channel_sum_add_and_convert(G):
    cx = G.ctx()
    x = bf16_round(formula_input((3000, 40), 1))
    xd = x.to(DEV).to(torch.bfloat16).contiguous()
    out = torch.empty(40, dtype=torch.float32, device=DEV)
    ws = torch.empty(cx.lib.channel_sum_workspace_floats(3000, 40), dtype=torch.float32, device=DEV)
    y = bf16_round(formula_input((3000, 40), 2)).to(DEV).to(torch.bfloat16)
    f = formula_input((1000,), 3).to(DEV)
    fb = torch.empty(1000, dtype=torch.bfloat16, device=DEV)
    with cx.scope():
        cx.lib.channel_sum(G._ptr(xd), 3000, 40, 40, G._ptr(ws), G._ptr(out), 0.5, cx.sptr)
        ysum = y.clone()
        cx.lib.add_bf16(G._ptr(ysum), G._ptr(xd), ysum.numel(), cx.sptr)
        cx.lib.f32_to_bf16(G._ptr(f), G._ptr(fb), 1000, cx.sptr)
    torch.cuda.synchronize()
    assert rel_l2(out.cpu(), 0.5 * x.sum(0)) <= 1e-5
    assert torch.equal(ysum.float().cpu(), bf16_round(y.float().cpu() + x))
    assert torch.equal(fb.float().cpu(), bf16_round(f.cpu()))


def test_q_sample_and_loss(G, pkg):
    cx = G.ctx()
    n, L, d, h, w = 3, 8, 4, 5, 6
    diff = pkg.GaussianDiffusion()
    z0 = formula_input((n, L, d, h, w), 1)
    noise = formula_input((n, L, d, h, w), 2)
    t = torch.tensor([0, 500, 999])
    want_zt = (diff.sqrt_alphas_cumprod[t].view(-1, 1, 1, 1, 1) * z0 +
               diff.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1, 1) * noise)
    xin = torch.zeros(n * d * h * w * 2 * L, dtype=torch.bfloat16, device=DEV)
    pred_ncdhw = formula_input((n, L, d, h, w), 3).requires_grad_(True)
    mask = (formula_input((n, L, d), 4) > 0).float()
    snr = diff.alphas_cumprod[t] / (1 - diff.alphas_cumprod[t] + 1e-8)
    wgt = torch.clamp(snr, max=5.0) / (snr + 1e-8)
    for use_mask in (False, True):
        if use_mask:
            me = mask[:, :, :, None, None].expand_as(pred_ncdhw)
            per = (((pred_ncdhw - noise) ** 2) * me).reshape(n, -1).sum(1) / me.reshape(n, -1).sum(1)
            loss = (per * wgt).mean()
            norm = wgt / (me.reshape(n, -1).sum(1) * n)
        else:
            per = F.mse_loss(pred_ncdhw, noise, reduction="none").reshape(n, -1).mean(1)
            loss = (per * wgt).mean()
            norm = wgt / (n * L * d * h * w)
        pred_ncdhw.grad = None
        (loss * 3.0).backward()
        pred = pred_ncdhw.detach().permute(0, 2, 3, 4, 1).contiguous().to(DEV)
        z0d, nd, td = z0.to(DEV), noise.to(DEV), t.to(DEV, torch.int32)
        sa, s1 = diff.sqrt_alphas_cumprod.to(DEV), diff.sqrt_one_minus_alphas_cumprod.to(DEV)
        normd, maskd = norm.float().to(DEV), mask.to(DEV)
        gs = torch.tensor([3.0], device=DEV)
        lo = torch.empty(1 + n, dtype=torch.float32, device=DEV)
        wsd = torch.empty(cx.lib.mse_loss_workspace_doubles(n), dtype=torch.float64, device=DEV)
        dp = torch.empty(n * d * h * w * L, dtype=torch.bfloat16, device=DEV)
        with cx.scope():
            cx.lib.q_sample(G._ptr(z0d), G._ptr(nd), G._ptr(sa), G._ptr(s1), G._ptr(td), G._ptr(xin), n, L, d, h, w,
                            2 * L, 0, cx.sptr)
            cx.lib.mse_loss_fwd(G._ptr(pred), G._ptr(nd), G._ptr(maskd) if use_mask else None, G._ptr(normd), n, L, d,
                                h, w, G._ptr(wsd), G._ptr(lo), cx.sptr)
            cx.lib.mse_loss_bwd(G._ptr(pred), G._ptr(nd), G._ptr(maskd) if use_mask else None, G._ptr(normd),
                                G._ptr(gs), n, L, d, h, w, G._ptr(dp), L, cx.sptr)
        torch.cuda.synchronize()
        assert abs(lo[0].item() - loss.item()) <= 1e-5 * abs(loss.item())
        got = dp.float().reshape(n, d, h, w, L).permute(0, 4, 1, 2, 3).cpu()
        assert rel_l2(got, pred_ncdhw.grad) <= 4e-3    # bf16 output rounding
    zt = xin.float().reshape(n, d, h, w, 2 * L)[..., :L].permute(0, 4, 1, 2, 3).cpu()
    assert torch.equal(zt, bf16_round(want_zt))


def test_linear_bwd_and_time_embed_train(G):
    cx = G.ctx()
    rows, din, dout = 4, 48, 100
    x = formula_input((rows, din), 1).requires_grad_(True)
    wt = (0.2 * formula_input((dout, din), 2)).requires_grad_(True)
    b = (0.1 * formula_input((dout,), 3)).requires_grad_(True)
    dy = formula_input((rows, dout), 4)
    for silu_in in (0, 1):
        for v in (x, wt, b):
            v.grad = None
        y = F.linear(F.silu(x) if silu_in else x, wt, b)
        y.backward(dy)
        xd, wd, dyd = x.detach().to(DEV), wt.detach().to(DEV), dy.to(DEV)
        dw = torch.empty_like(wd)
        db = torch.empty(dout, device=DEV)
        dx = torch.empty_like(xd)
        with cx.scope():
            cx.lib.linear_bwd(G._ptr(xd), G._ptr(wd), G._ptr(dyd), rows, din, dout, silu_in, G._ptr(dw), G._ptr(db),
                              G._ptr(dx), cx.sptr)
        torch.cuda.synchronize()
        assert rel_l2(dw.cpu(), wt.grad) <= 1e-5 and rel_l2(db.cpu(), b.grad) <= 1e-5
        assert rel_l2(dx.cpu(), x.grad) <= 1e-5
