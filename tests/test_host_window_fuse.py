"""CPU: the host side of latent window fusion -- the per-axis blend tables against a brute-force
enumeration, every refusal before a device is touched, the defaults of the public signatures, and the C ABI of the three
new entries (declared, exported, bound; argument checks before any launch)."""
import ctypes as C
import importlib
import inspect
import re

import numpy as np
import pytest
import torch

from tests.helpers import TINY_UNET

L = importlib.import_module("video-to-video-diffusion_amd.lib")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
WF = importlib.import_module("video-to-video-diffusion_amd.window_fuse")

# the test geometry of the feature in latent coordinates (pixel: volume (6, 32, 24), patch (4, 16, 16) -> (12, 16, 16), stride
# (2, 12, 4)), and the README's stitching case 512 / 192 / 96 along one axis, in pixels and in latent voxels
AXES = [(18, 12, [0, 6]), (8, 4, [0, 3, 4]), (6, 4, [0, 1, 2]), (512, 192, None), (128, 48, None)]
NEW = {"ctsi_window_gather": 16, "ctsi_window_gather_f32": 16, "ctsi_window_blend": 20}


class _VAE:
    latent_dim = 8

    def get_latent_shape(self, s):
        return (s[0], 8, s[2], s[3] // 4, s[4] // 4)


def test_geometry_of_the_test_volume():
    geo = WF.stitch_geometry(_VAE(), (2, 1, 6, 32, 24), (4, 16, 16), (12, 16, 16), (2, 12, 4))
    assert geo.full == (18, 8, 6) and geo.win == (12, 4, 4) and geo.factor == 4 and len(geo.starts) == 18
    assert geo.pixel_windows == [(d, h, w) for d in (0, 2) for h in (0, 12, 16) for w in (0, 4, 8)]
    assert geo.starts == [(d, h, w) for d in (0, 6) for h in (0, 3, 4) for w in (0, 1, 2)]
    assert WF.axis_starts(geo.starts) == ([0, 6], [0, 3, 4], [0, 1, 2])
    tabs = [WF.axis_table(f, s, st) for f, s, st in zip(geo.full, geo.win, WF.axis_starts(geo.starts))]
    assert [int(t.count.max()) for t in tabs] == [2, 2, 3] and [t.index.shape[1] for t in tabs] == [2, 2, 3]


@pytest.mark.parametrize("full,size,starts", AXES, ids=[f"{a[0]}-{a[1]}" for a in AXES])
def test_axis_table_is_a_partition_of_unity_and_matches_brute_force(full, size, starts):
    if starts is None:
        starts = S._window_starts(full, size, size // 2)
    t = WF.axis_table(full, size, starts)
    w = S._axis_window(size).double().numpy()
    assert t.weight.dtype == np.float64 and np.abs(t.weight.sum(axis=1) - 1.0).max() <= 1e-15
    kmax = 0
    for p in range(full):
        cover = [k for k, s in enumerate(starts) if 0 <= p - s < size]
        kmax = max(kmax, len(cover))
        assert int(t.count[p]) == len(cover) and list(t.index[p, :len(cover)]) == cover
        assert list(t.offset[p, :len(cover)]) == [p - starts[k] for k in cover]
        tot = sum(w[p - starts[k]] for k in cover)
        assert np.array_equal(t.weight[p, :len(cover)], np.array([w[p - starts[k]] / tot for k in cover]))
        assert not t.weight[p, len(cover):].any()
    assert t.index.shape == (full, kmax)        # the table is as wide as the largest cover count, no wider
    ti, tw = WF.pack_tables([t, t, t])
    assert ti.dtype == torch.int32 and tw.dtype == torch.float32
    assert ti.numel() == 3 * full * (1 + 2 * kmax) and tw.numel() == 3 * full * kmax


def test_the_last_start_can_add_an_overlap():
    """512 / 192 / 96: starts 0, 96, 192, 288 and the last one 320 -- three windows over [320, 384), one more than size / stride."""
    starts = S._window_starts(512, 192, 96)
    assert starts == [0, 96, 192, 288, 320]
    assert int(WF.axis_table(512, 192, starts).count.max()) == 3


def test_bad_tables_and_grids_are_refused():
    with pytest.raises(L.CtsiError, match="uncovered"):
        WF.axis_table(10, 4, [0, 6])
    with pytest.raises(L.CtsiError, match="inside"):
        WF.axis_table(10, 4, [0, 7])
    with pytest.raises(L.CtsiError, match="product grid"):
        WF.axis_starts([(0, 0, 0), (0, 0, 2), (0, 2, 0)])
    for shape, patch, stride, bad in (((1, 1, 4, 34, 16), (4, 16, 16), (2, 8, 8), "34"),
                                      ((1, 1, 4, 32, 16), (4, 16, 16), (2, 6, 8), "6"),
                                      ((1, 1, 4, 32, 18), (4, 16, 18), (2, 8, 8), "18")):
        with pytest.raises(L.CtsiError, match=bad):
            WF.stitch_geometry(_VAE(), shape, patch, patch, stride)


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
SAMPLERS = ("DDIMSampler", "DDPMSampler", "DPMSolverSampler", "HeunSampler")


def test_pixel_fusion_is_the_default_everywhere():
    for name in SAMPLERS:
        p = inspect.signature(getattr(S, name).sample_with_stitching).parameters
        assert p["fusion"].default == "pixel" and p["decode"].default is None, name
    assert WF.check_fusion("pixel", None) == ("pixel", None)
    assert WF.check_fusion("latent", None) == ("latent", "full")
    assert WF.check_fusion("latent", "windows") == ("latent", "windows")


@pytest.fixture(scope="module")
def parts(pkg):
    torch.manual_seed(0)
    return pkg.GaussianDiffusion("cosine", 1000), pkg.UNet3D(**TINY_UNET), pkg.UNet3D(**TINY_UNET, learn_sigma=True), _VAE()


def _samplers(g, un):
    return [S.DDIMSampler(g, un), S.DDPMSampler(g, un), S.DPMSolverSampler(g, un), S.HeunSampler(g, un)]


V_CPU = torch.zeros(1, 1, 4, 32, 32)      # a CPU tensor: everything below raises before a device is touched
GEO = dict(patch_size=(4, 16, 16), target_patch_size=(4, 16, 16), stride=(2, 8, 8), device="cuda", progress=False)


def _call(sm, **kw):
    args = (V_CPU, _VAE()) if isinstance(sm, S.DDPMSampler) else (V_CPU, _VAE(), 3)
    return sm.sample_with_stitching(*args, **GEO, **kw)


def test_bad_values_are_value_errors(parts):
    g, un, _, _ = parts
    for sm in _samplers(g, un):
        with pytest.raises(ValueError, match="unknown fusion"):
            _call(sm, fusion="latents")
        with pytest.raises(ValueError, match="unknown fusion"):
            _call(sm, fusion=None)
        with pytest.raises(ValueError, match="unknown decode"):
            _call(sm, fusion="latent", decode="window")
        with pytest.raises(ValueError, match="belongs to fusion='latent'"):
            _call(sm, decode="full")
        with pytest.raises(ValueError, match="belongs to fusion='latent'"):
            _call(sm, fusion="pixel", decode="windows")


def test_refusals_name_the_alternative_before_a_device_is_touched(parts, pkg):
    g, un, un_ls, _ = parts
    for sm in _samplers(g, un):
        with pytest.raises(L.CtsiError, match="dp_group.*fusion='pixel'"):
            _call(sm, fusion="latent", dp_group=True)
    for sm in _samplers(g, un)[:1] + _samplers(g, un)[2:]:        # (DDPMSampler has no window_batch)
        for wb in (1, 3):
            with pytest.raises(L.CtsiError, match="window_batch.*decode='windows'"):
                _call(sm, fusion="latent", window_batch=wb)
    for sm in _samplers(g, un_ls):
        with pytest.raises(L.CtsiError, match="learn_sigma.*fusion='pixel'"):
            _call(sm, fusion="latent")
    g_lr = pkg.GaussianDiffusion("cosine", 1000)
    g_lr.var_type = "learned_range"
    with pytest.raises(L.CtsiError, match="learn_sigma"):
        _call(S.DDIMSampler(g_lr, un_ls), fusion="latent")
    with pytest.raises(L.CtsiError, match="ddpm_spaced"):      # the strided ancestral sampler: kind 'ddpm_lv'
        _call(S.DDPMSampler(g, un), fusion="latent", num_inference_steps=10)
    with pytest.raises(L.CtsiError, match="UNet3D.*fusion='pixel'"):
        _call(S.DDIMSampler(g, lambda z, t, c: z), fusion="latent")

    class Comm:
        world, rank = 2, 0

    un.depth_shard_comm = Comm()
    try:
        with pytest.raises(L.CtsiError, match="depth sharding"):
            _call(S.DDIMSampler(g, un), fusion="latent")
    finally:
        del un.depth_shard_comm
    # the lower-level entry refuses the same things itself
    with pytest.raises(L.CtsiError, match="UNet3D"):
        S.run_sampler_fused(g, lambda z, t, c: z, (1, 8, 4, 8, 8), torch.zeros(1, 8, 4, 8, 8), (4, 8, 8), [(0, 0, 0)], "cuda",
                            kind="ddim", t_desc=[999, 0])
    with pytest.raises(L.CtsiError, match="learn_sigma"):
        S.run_sampler_fused(g, un_ls, (1, 8, 4, 8, 8), torch.zeros(1, 8, 4, 8, 8), (4, 8, 8), [(0, 0, 0)], "cuda",
                            kind="ddim", t_desc=[999, 0])


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not L.LIB_PATH.exists():
        L.build()
    return L.get_lib()


def test_new_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", L.HEADER_PATH.read_text(), flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\b(ctsi_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}
    dll = C.CDLL(str(L.LIB_PATH))
    for s, nargs in NEW.items():
        assert s in declared, f"{s} not declared in include/ctsi.h"
        assert len(declared[s].split(",")) == nargs, (s, declared[s])
        assert hasattr(dll, s), f"{s} not exported"
        assert s in L.SIGNATURES and len(L.SIGNATURES[s][1]) == nargs and L.SIGNATURES[s][2]
        assert hasattr(lib, s[len("ctsi_"):])


ONE = C.c_void_p(16)     # never dereferenced: argument checks run before any launch


def test_entries_reject_bad_arguments_without_launching(lib):
    ok_g = (1, 1, 2, 8, 8, 8, 4, 4, 4, 8, 8, 16)
    for fn in (lib.window_gather, lib.window_gather_f32):
        for ptrs in ((None, ONE, ONE), (ONE, None, ONE), (ONE, ONE, None)):
            with pytest.raises(L.CtsiError, match="null argument"):
                fn(*ptrs, *ok_g, None)
        for bad in ((0,) + ok_g[1:], (1, 3) + ok_g[2:], (1, 1, 0) + ok_g[3:], (1, 1, 2, 8, 8, 8, 9, 4, 4, 8, 8, 16),
                    (1, 1, 2, 8, 8, 8, 4, 4, 4, 8, 4, 16), (1, 1, 2, 8, 8, 8, 4, 4, 4, 8, 8, 4)):
            with pytest.raises(L.CtsiError, match="bad shape"):
                fn(ONE, ONE, ONE, *bad, None)
    ok_b = (1, 1, 1, 2, 2, 8, 8, 8, 4, 4, 4, 8, 1, 2, 2)
    for ptrs in ((None, ONE, ONE, ONE), (ONE, None, ONE, ONE), (ONE, ONE, None, ONE), (ONE, ONE, ONE, None)):
        with pytest.raises(L.CtsiError, match="null argument"):
            lib.window_blend(*ptrs, *ok_b, None)
    for bad in ((0,) + ok_b[1:], (1, 0) + ok_b[2:], ok_b[:8] + (9,) + ok_b[9:], ok_b[:12] + (2, 2, 2), ok_b[:12] + (1, 0, 2)):
        with pytest.raises(L.CtsiError, match="bad shape"):
            lib.window_blend(ONE, ONE, ONE, ONE, *bad, None)
    for c in (6, 0, -4):
        with pytest.raises(L.CtsiError, match="multiple of 4"):
            lib.window_blend(ONE, ONE, ONE, ONE, *ok_b[:11], c, *ok_b[12:], None)
    with pytest.raises(L.CtsiError, match="aligned"):
        lib.window_blend(C.c_void_p(20), ONE, ONE, ONE, *ok_b, None)
    assert lib.raw["ctsi_window_blend"](None, ONE, ONE, ONE, *ok_b, None) == -1          # CTSI_ERR_INVALID
