"""CPU: the packed-weight cache key names the image layout, not just the kernel family.  Programs built from the same weights
share packed images through engine._PACKED, keyed by engine._pack_sig; the k32 kernel packs a cout-permuted image for its
direct-store tiles and a natural-order one for the staged 384-voxel tiles, and the plan picks the tile from the batch size.
Host-only plan calls, no launches (the GPU side of the same property: tests/test_gpu_weight_cache.py)."""
import ctypes as C
import importlib

import pytest

L = importlib.import_module("video-to-video-diffusion_amd.lib")
E = importlib.import_module("video-to-video-diffusion_amd.engine")


@pytest.fixture(scope="module")
def lib():
    if not L.LIB_PATH.exists():
        L.build()
    return L.get_lib()


def _plan(lib, **kw):
    d = dict(transposed=0, kd=3, kh=3, kw=3, sh=1, sw=1, pd=1, ph=1, pw=1, n=1, c1=128, c2=0, cout=128, di=48,
             hi=24, wi=24, halo_d=0)
    d.update(kw)
    plan = C.c_void_p()
    lib.conv_plan_create(C.byref(plan), C.byref(L.ConvDesc(**d)))
    return plan, d


def _sig(lib, plan, d, cin_w=None):
    return E._pack_sig(lib, plan, d["transposed"], (d["kd"], d["kh"], d["kw"]), (d["sh"], d["sw"]), d["c1"], d["c2"],
                       d["cout"], cin_w)


def _old_key(lib, plan, sig):
    """The key before the layout id existed: the kernel family as ctsi_conv_plan_config's mode tells it, then the rest."""
    bm, bn, mode = C.c_int(), C.c_int(), C.c_int()
    lib.conv_plan_config(plan, C.byref(bm), C.byref(bn), C.byref(mode))
    return ("gather" if mode.value in (0, 2) else mode.value,) + tuple(sig[1:])


# (descriptor, batch sizes of a staged 384-voxel k32 tile, batch sizes of a direct-store tile): the 48 x 24 x 24 latent of one
# 48 x 192 x 192 stitching window, at one window (generate() on a patch) or a few and at a window batch (13 on a 288 GB part)
CROSSING = [
    (dict(c1=128, cout=128), (2, 4, 8), (13, 16, 25)),          # U-Net level 0 ResBlocks
    (dict(c1=256, cout=256), (1,), (13, 16, 25)),
    (dict(c1=256, c2=128, cout=128), (2,), (13, 25)),           # U-Net decoder level 0, skip concat
    (dict(c1=128, cout=256), (1, 2, 4), (8, 13, 16, 25)),
]


@pytest.mark.parametrize("desc,staged,direct", CROSSING, ids=["128-128", "256-256", "256+128-128", "128-256"])
def test_cache_key_separates_staged_and_direct_k32_images(lib, desc, staged, direct):
    keys = {}
    for n in staged + direct:
        p, d = _plan(lib, n=n, **desc)
        sig = _sig(lib, p, d)
        keys[n] = (sig, _old_key(lib, p, sig), lib.conv_plan_pack_layout(p))
        lib.conv_plan_destroy(p)
    for a in staged:
        for b in direct:
            (sa, oa, la), (sb, ob, lb) = keys[a], keys[b]
            assert oa == ob, (a, b, oa, ob)                          # the fields the key had before are all equal ...
            assert la & 0xF == lb & 0xF == 4, (la, lb)                # ... both are k32 plans ...
            assert (la >> 6) & 1 == 0 and (lb >> 6) & 1 == 1, (a, b, hex(la), hex(lb))   # ... of the two image layouts
            assert sa != sb, f"n={a} and n={b} would share one packed image: {sa}"
    # plans on the same tile whatever the batch size: one image, one key (sharing must not be lost)
    for group in (staged, direct):
        assert len({keys[n][0] for n in group}) == 1, {n: keys[n][0] for n in group}


def test_pack_layout_ids_per_family(lib):
    fam = lambda p: lib.conv_plan_pack_layout(p) & 0xF
    cases = [
        (dict(hi=128, wi=128), None, None, 4),                                         # k32 4x4x32
        (dict(c1=128, cout=128), None, None, 3),                                      # n = 1 at 24^2: 4x4x16 halo tile
        (dict(c1=128, cout=8), None, None, 5),                                        # head
        (dict(c1=8, cout=128), 1, None, 7),                                           # stem (1-channel volume, 8 stored)
        (dict(kd=1, kh=1, kw=1, pd=0, ph=0, pw=0, c1=256, cout=128), None, 1, 6),     # streaming 1^3 ResBlock tail
        (dict(kd=1, kh=1, kw=1, pd=0, ph=0, pw=0, c1=256, cout=128), None, None, 1),  # the same conv on the gather kernel
        (dict(c1=16, cout=32, hi=8, wi=8), None, None, 2),                            # small-Cin gather
    ]
    for desc, cin_w, tail, want in cases:
        p, d = _plan(lib, **desc)
        if cin_w is not None:
            lib.conv_plan_set_weight_cin(p, cin_w)
        if tail is not None:
            lib.conv_plan_set_stream_tail(p, tail)
        assert fam(p) == want, (desc, hex(lib.conv_plan_pack_layout(p)))
        lib.conv_plan_destroy(p)
    # k32 forms: plain, ConvTranspose3d, strided Downsample
    for desc, form in ((dict(hi=128, wi=128), 0),
                       (dict(transposed=1, kh=4, kw=4, sh=2, sw=2, c1=256, cout=256, hi=64, wi=64), 1),
                       (dict(kh=4, kw=4, sh=2, sw=2, c1=256, cout=256, hi=64, wi=64), 2)):
        p, d = _plan(lib, **desc)
        lay = lib.conv_plan_pack_layout(p)
        assert lay & 0xF == 4 and (lay >> 4) & 3 == form and lay >> 8 == 128 // 16, (desc, hex(lay))
        lib.conv_plan_destroy(p)
    assert lib.conv_plan_pack_layout(None) == 0
