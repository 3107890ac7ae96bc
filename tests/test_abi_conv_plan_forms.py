"""CPU: which kernel form and tile ctsi_conv_plan_create picks -- host-only plan calls, no launches.

(a) tests/golden/conv_plan_forms.npz holds the plan of every descriptor of tools/conv_plan_sweep.py's grid (the nine ABI
    values a caller sizes its buffers and cache keys from, plus ctsi_conv_plan_form) with no override set, and one SHA-256 of
    that table per override block; the library must reproduce every row and every digest.  Here: all rows, and the blocks of
    every single variable, every test dictionary and a fixed stride through the pairs; the tool's --check covers all blocks.
(b) every override dictionary tests/test_gpu_ops.py and tests/test_gpu_poison.py build to reach one tile does reach it, on
    that test's own case shapes -- or falls back exactly as FALLBACKS lists."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

L = importlib.import_module("video-to-video-diffusion_amd.lib")
SWEEP = importlib.import_module("tools.conv_plan_sweep")
OPS = importlib.import_module("tests.test_gpu_ops")
POISON = importlib.import_module("tests.test_gpu_poison")

REGENERATE = ("the full table of both libraries, for diffing: CTSI_LIB=<libctsi.so> python tools/conv_plan_sweep.py --dump <out.npz> "
              "[--block NAME]; to record again: CTSI_LIB=<libctsi.so> python tools/conv_plan_sweep.py --write")


@pytest.fixture(scope="module")
def lib():
    if not L.LIB_PATH.exists():
        L.build()
    return L.get_lib()


@pytest.fixture(autouse=True)
def _keep_environment():
    saved = {k: v for k, v in os.environ.items() if k.startswith("CTSI_CONV")}
    yield
    SWEEP.set_env(saved)


# ---- (a) the recorded table -------------------------------------------------------------------------------------------
def test_plans_without_overrides_match_the_recorded_table(lib):
    want, _ = SWEEP.load_table()
    got = SWEEP.sweep({})
    assert got.shape == want.shape == (len(SWEEP.descriptors()), len(SWEEP.COLUMNS)), (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    detail = [f"{SWEEP.describe(i)}: recorded {dict(zip(SWEEP.COLUMNS, want[i].tolist()))}, library {got[i].tolist()}" for i in bad[:5]]
    assert len(bad) == 0, f"{len(bad)} plans differ, e.g.\n" + "\n".join(detail) + "\n" + REGENERATE


def test_plans_under_overrides_match_the_recorded_digests(lib):
    _, want = SWEEP.load_table()
    every = SWEEP.blocks()
    assert [name for name, _ in every] == list(want), "the tool's blocks and the recorded ones differ\n" + REGENERATE
    pairs = [b for b in every if "," in b[0] and not b[0].startswith("test:")]
    todo = [b for b in every if b not in pairs] + pairs[::101]
    bad = [name for name, env in todo if SWEEP.digest(SWEEP.sweep(env)) != want[name]]
    assert not bad, f"plans differ under {len(bad)} of {len(todo)} override blocks: {bad[:8]}\n" + REGENERATE


# ---- (b) the override dictionaries reach the tile their name claims ---------------------------------------------------------
K3 = dict(transposed=0, kd=3, kh=3, kw=3)
DOWN = dict(transposed=0, kd=3, kh=4, kw=4, sh=2, sw=2)
UP = dict(transposed=1, kd=3, kh=4, kw=4, sh=2, sw=2)
HALO32, K32 = 4, 9    # ctsi_conv_plan_config's mode of conv3_halo32_kernel / conv3_halo_k32_kernel
# tile name -> (mode, (TD, TH, TW), split-K factor)
HALO3_FORMS = {"16h": (HALO32, (4, 4, 16), 0), "16h3": (HALO32, (3, 4, 16), 0), "32": (HALO32, (4, 2, 32), 0),
               "16k": (K32, (4, 8, 16), 0), "32k": (K32, (4, 4, 32), 0), "32k3": (K32, (3, 4, 32), 0), "16k3": (K32, (3, 8, 16), 1),
               "16k3s": (K32, (3, 8, 16), 2), "32ks": (K32, (4, 4, 32), 2)}
DOWN_FORMS = {"32k": (K32, (4, 4, 32), 0), "16k": (K32, (4, 8, 16), 0), "32k3": (K32, (3, 4, 32), 0), "16k3": (K32, (3, 8, 16), 0),
              "16k3s": (K32, (3, 8, 16), 2)}
CONVT_FORMS = {"32": (K32, (4, 4, 32), 0), "16": (K32, (4, 8, 16), 0), "32x384": (K32, (3, 4, 32), 0), "16x384": (K32, (3, 8, 16), 0)}

# (helper, tile, case) that do NOT reach the named tile at the parent of the commit that added this test, with what they do
# reach: recorded from that library, not edited to make a later one pass
FALLBACKS = {
    ("halo3_tile_env", "16h", "cin32_cout_72_pad"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "16h", "cin16_stem_two_sources"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "16h", "cin16_unet_stem"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "16h3", "cin32_cout_72_pad"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "16h3", "cin16_stem_two_sources"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "16h3", "cin16_unet_stem"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "32", "cin32_cout_72_pad"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "32", "cin16_stem_two_sources"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "32", "cin16_unet_stem"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "16k3", "concat_256+128"): (9, (3, 8, 16), 2),
    ("halo3_tile_env", "16k3", "cin512_deep_k"): (9, (3, 8, 16), 2),
    ("halo3_tile_env", "16k3s", "aligned_64_128"): (4, (3, 4, 16), 0),
    ("halo3_tile_env", "16k3s", "ragged_edges_batch2"): (4, (3, 4, 16), 0),
    ("halo3_tile_env", "16k3s", "concat_64+32_cout256"): (4, (3, 4, 16), 0),
    ("halo3_tile_env", "16k3s", "cin32_cout_72_pad"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "16k3s", "cin16_stem_two_sources"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "16k3s", "cin16_unet_stem"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "32ks", "aligned_64_128"): (4, (4, 2, 32), 0),
    ("halo3_tile_env", "32ks", "ragged_edges_batch2"): (4, (4, 2, 32), 0),
    ("halo3_tile_env", "32ks", "concat_64+32_cout256"): (4, (4, 2, 32), 0),
    ("halo3_tile_env", "32ks", "cin32_cout_72_pad"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "32ks", "cin16_stem_two_sources"): (9, (4, 4, 32), 0),
    ("halo3_tile_env", "32ks", "cin16_unet_stem"): (9, (4, 4, 32), 0),
    ("down_tile_env", "16k3s", "cin16_cout72"): (9, (3, 8, 16), 0),
}


def reached(lib, env, kind, n, c1, c2, cout, d, h, w):
    SWEEP.set_env(env)
    desc = dict(sh=1, sw=1, pd=1, ph=1, pw=1, halo_d=0, n=n, c1=c1, c2=c2, cout=cout, di=d, hi=h, wi=w)
    desc.update(kind)
    plan, mode, form = C.c_void_p(), C.c_int(), (C.c_int * 8)()
    lib.conv_plan_create(C.byref(plan), C.byref(L.ConvDesc(**desc)))
    lib.conv_plan_config(plan, None, None, C.byref(mode))
    lib.conv_plan_form(plan, form)
    ws = lib.conv_plan_workspace_bytes(plan)
    lib.conv_plan_destroy(plan)
    assert (ws > 0) == (form[3] >= 2), (ws, list(form))
    assert bool(form[4] & 8) == (mode.value == K32 and kind is DOWN), list(form)
    return mode.value, tuple(form[:3]), form[3]


def tile_dictionaries():
    """(helper, tile, case name, env, kind, (n, c1, c2, cout, d, h, w), claimed form)"""
    out = []
    for tile in OPS.HALO3_TILES:
        for name, c1, c2, cout, (n, d, h, w) in OPS.HALO3_CASES:
            out.append(("halo3_tile_env", tile, name, OPS.halo3_tile_env(tile), K3, (n, c1, c2, cout, d, h, w), HALO3_FORMS[tile]))
    for tile in OPS.DOWN_TILES:
        for name, cin, cout, (n, d, h, w) in OPS.DOWN_CASES:
            out.append(("down_tile_env", tile, name, OPS.down_tile_env(tile), DOWN, (n, cin, 0, cout, d, h, w), DOWN_FORMS[tile]))
    for tile in OPS.CONVT_TILES:
        for name, cin, cout, (n, d, h, w) in OPS.CONVT_CASES:
            out.append(("convt_tile_env", tile, name, OPS.convt_tile_env(tile), UP, (n, cin, 0, cout, d, h, w), CONVT_FORMS[tile]))
    return out


def test_every_tile_is_named_by_a_dictionary():
    assert set(HALO3_FORMS) == set(OPS.HALO3_TILES) and set(DOWN_FORMS) == set(OPS.DOWN_TILES) and set(CONVT_FORMS) == set(OPS.CONVT_TILES)
    used = {(c[0], c[1], c[2]) for c in tile_dictionaries()}
    assert set(FALLBACKS) <= used, set(FALLBACKS) - used


def test_tile_dictionaries_reach_their_tile(lib):
    wrong = []
    for helper, tile, case, env, kind, shape, claimed in tile_dictionaries():
        got = reached(lib, env, kind, *shape)
        want = FALLBACKS.get((helper, tile, case), claimed)
        if got != want:
            wrong.append(f"{helper}({tile!r}) on {case}: reached {got}, expected {want}")
    assert not wrong, "\n".join(wrong)


def narrow_tile(w):
    return (4, 4, 24) if w % 24 == 0 else (8, 4, 12)


def test_narrow_dictionaries_reach_the_straddling_tiles(lib):
    for name, c1, c2, cout, (n, d, h, w), bm in OPS.NARROW_CASES:
        mode, tile, split = reached(lib, {"CTSI_CONV_K32_NARROW": "1"}, K3, n, c1, c2, cout, d, h, w)
        if bm is None:      # a plane 16-wide tiles divide takes no straddling tile
            assert tile[2] in (16, 32), (name, mode, tile)
        else:
            assert (mode, tile) == (K32, narrow_tile(w)) and tile[0] * tile[1] * tile[2] == bm and split in (0, 2), (name, mode, tile, split)
    split_k = next(m for m in OPS.test_narrow_plane_tiles_split_k.pytestmark if m.name == "parametrize").args[1]
    narrow_sk = [c for c in SWEEP.split_k_cases(POISON) if c[0].startswith("narrow-split-K")]
    assert narrow_sk and all(c[1] == narrow_sk[0][1] for c in narrow_sk)
    shapes = [(c1, c2, cout, dims) for c1, c2, cout, dims in split_k] + [c[2:] for c in narrow_sk]
    for c1, c2, cout, (n, d, h, w) in shapes:
        assert reached(lib, narrow_sk[0][1], K3, n, c1, c2, cout, d, h, w) == (K32, narrow_tile(w), 2), (c1, c2, cout, n, d, h, w)
    for name, env, c1, c2, cout, (n, d, h, w) in SWEEP.split_k_cases(POISON):
        if name.startswith("k32-split-K"):
            assert reached(lib, env, K3, n, c1, c2, cout, d, h, w) == (K32, (3, 8, 16), 2), name
