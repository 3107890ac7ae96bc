"""CPU: the bf16x3 convolution's C ABI (host-only sizing / support queries).  No compute is launched."""
import ctypes as C
import importlib
import re

import pytest

L = importlib.import_module("video-to-video-diffusion_amd.lib")

NEW_SYMBOLS = ["ctsi_conv_bf16x3_supported", "ctsi_conv_bf16x3_weight_bytes", "ctsi_conv_bf16x3_geometry",
               "ctsi_conv_bf16x3_flops", "ctsi_conv_bf16x3_pack_weights", "ctsi_conv_bf16x3_fwd"]


@pytest.fixture(scope="module")
def lib():
    if not L.LIB_PATH.exists():
        L.build()
    return L.get_lib()


def _desc(**kw):
    d = dict(transposed=0, kd=3, kh=3, kw=3, sh=1, sw=1, pd=1, ph=1, pw=1, n=1, c1=128, c2=0, cout=128, di=48, hi=128,
             wi=128, halo_d=0)
    d.update(kw)
    return L.ConvDesc(**d)


K111 = dict(kd=1, kh=1, kw=1, pd=0, ph=0, pw=0)
DOWN = dict(kh=4, kw=4, sh=2, sw=2)
UP = dict(transposed=1, kh=4, kw=4, sh=2, sw=2)


def test_every_new_symbol_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", L.HEADER_PATH.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(ctsi_[a-z0-9_]+)\s*\(", text))
    dll = C.CDLL(str(L.LIB_PATH))
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} not declared in include/ctsi.h"
        assert hasattr(dll, s), f"{s} not exported"
        assert s in L.SIGNATURES, f"{s} not bound in lib.py"
        assert hasattr(lib, s[len("ctsi_"):])
        assert L.SIGNATURES[s] == L.SIGNATURES[s.replace("bf16x3", "f32")]     # the same descriptor and output struct


@pytest.mark.parametrize("geom, cin, cout, dims, out_dims, ncls, taps", [
    ({}, 128, 128, (48, 128, 128), (48, 128, 128), 1, 27),
    (K111, 96 + 32, 70, (6, 7, 9), (6, 7, 9), 1, 1),
    (DOWN, 24, 36, (4, 10, 13), (4, 5, 6), 1, 48),
    (UP, 20, 12, (3, 5, 7), (3, 10, 14), 4, 12),
    ({}, 1, 16, (8, 192, 192), (8, 192, 192), 1, 27),     # VAE stem: one input channel
    ({}, 128, 1, (48, 512, 512), (48, 512, 512), 1, 27),  # VAE head: one output channel
])
def test_supported_geometries_and_sizes(lib, geom, cin, cout, dims, out_dims, ncls, taps):
    d = _desc(c1=cin, cout=cout, di=dims[0], hi=dims[1], wi=dims[2], **geom)
    assert lib.conv_bf16x3_supported(C.byref(d)) == 1
    do, ho, wo, tps, nc, cpad = (C.c_int() for _ in range(6))
    lib.conv_bf16x3_geometry(C.byref(d), C.byref(do), C.byref(ho), C.byref(wo), C.byref(tps), C.byref(nc), C.byref(cpad))
    assert (do.value, ho.value, wo.value) == out_dims and nc.value == ncls
    bn = 32 if cout <= 32 else (64 if cout <= 64 else 128)
    assert cpad.value == -(-cout // bn) * bn
    rows = out_dims[0] * out_dims[1] * out_dims[2] // ncls
    assert tps.value == -(-rows // 128)
    # the geometry is the fp32 kernel's: a colsum slab of one serves ctsi_gn_finalize like the other's
    f = [C.c_int() for _ in range(6)]
    lib.conv_f32_geometry(C.byref(d), *[C.byref(v) for v in f])
    assert [v.value for v in f] == [do.value, ho.value, wo.value, tps.value, nc.value, cpad.value]
    kpad = -(-cin // 32) * 32                    # the K slice is 32 channels; a hi and a lo bf16 image
    assert lib.conv_bf16x3_weight_bytes(C.byref(d)) == 2 * 2 * ncls * taps * kpad * cpad.value
    fl = lib.conv_bf16x3_flops(C.byref(d))
    vox = dims[0] * dims[1] * dims[2] if geom.get("transposed") else out_dims[0] * out_dims[1] * out_dims[2]
    k = d.kd * d.kh * d.kw
    assert abs(fl - 2.0 * vox * cin * cout * k) < 1            # the useful 2 M N K, not the three products
    assert fl == lib.conv_f32_flops(C.byref(d))


def test_concatenated_source_counts_both_halves(lib):
    d = _desc(c1=24, c2=13, cout=40, di=5, hi=9, wi=11)
    assert lib.conv_bf16x3_supported(C.byref(d)) == 1
    assert lib.conv_bf16x3_weight_bytes(C.byref(d)) == 2 * 2 * 27 * 64 * 64      # cpad = 32 * ceil(37 / 32), cout_pad = 64


@pytest.mark.parametrize("bad, msg", [
    (dict(halo_d=1), "depth-sharded"),
    (dict(kd=5), "unsupported geometry"),
    (dict(kh=4, kw=4, sh=1, sw=1), "unsupported geometry"),
    (dict(sh=2, sw=2), "unsupported geometry"),
    (dict(transposed=1), "unsupported geometry"),
    (dict(n=0), "positive"),
    (dict(c1=0), "positive"),
    (dict(cout=-3), "positive"),
    (dict(di=0), "positive"),
])
def test_rejections_carry_a_message(lib, bad, msg):
    d = _desc(**bad)
    assert lib.conv_bf16x3_supported(C.byref(d)) == 0
    err = lib.last_error().decode()
    assert msg in err and "bf16x3" in err
    assert lib.conv_bf16x3_weight_bytes(C.byref(d)) == 0
    assert lib.conv_bf16x3_flops(C.byref(d)) == 0.0
    with pytest.raises(L.CtsiError, match=msg):
        lib.conv_bf16x3_geometry(C.byref(d), None, None, None, None, None, None)
    with pytest.raises(L.CtsiError):
        lib.conv_bf16x3_pack_weights(C.byref(d), C.c_void_p(16), C.c_void_p(16), None)
    with pytest.raises(L.CtsiError):
        lib.conv_bf16x3_fwd(C.byref(d), C.c_void_p(16), None, C.c_void_p(16), None, None, C.byref(L.ConvOut()), None)


def test_fwd_argument_checks(lib):
    d = _desc(c1=8, cout=8, di=2, hi=4, wi=4)
    co = L.ConvOut()
    with pytest.raises(L.CtsiError, match="null argument"):
        lib.conv_bf16x3_fwd(C.byref(d), C.c_void_p(256), None, C.c_void_p(256), None, None, C.byref(co), None)
    co.y = 256
    co.mode, co.cout_stride, co.c_off = 0, 8, 4
    with pytest.raises(L.CtsiError, match="channel slice"):
        lib.conv_bf16x3_fwd(C.byref(d), C.c_void_p(256), None, C.c_void_p(256), None, None, C.byref(co), None)
    co.c_off = 0
    with pytest.raises(L.CtsiError, match="16-byte aligned"):
        lib.conv_bf16x3_fwd(C.byref(d), C.c_void_p(256), None, C.c_void_p(264), None, None, C.byref(co), None)
    d2 = _desc(c1=8, c2=4, cout=8, di=2, hi=4, wi=4)
    with pytest.raises(L.CtsiError, match="x2 is null"):
        lib.conv_bf16x3_fwd(C.byref(d2), C.c_void_p(256), None, C.c_void_p(256), None, None, C.byref(co), None)
