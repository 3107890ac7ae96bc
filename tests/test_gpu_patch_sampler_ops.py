"""GPU: ctsi_patch_sample against the restatement (tests/patch_sampler_restatement.py).  The thin output is a gather and must
be bit-identical (fp16 storage: float(half(x))); the thick output may differ from the float64 blend on the same fp32 weights
by at most THICK_TOL = 2^-22 (two fp32 roundings of values below 1), and from torch's own F.interpolate on the device by the
same bound.  Patch sides 8 / 20 / 36 / 68 lie below, above and off the 64-wide tile and its 16-byte chunks; x0 in {0, 1, 3}
and volume widths pw, pw + 5, pw + 6 put source rows on and off the 16-byte grid for both storage types."""
import importlib
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import patch_sampler_restatement as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DD = importlib.import_module("video-to-video-diffusion_amd.device_data")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_sampler_v1.npz")


def make_volumes(shapes, seed):
    """[(thick, thin)] fp32 in [-1, 1] for (D_thick, D_thin, H, W) shapes."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((1, dk, h, w), generator=g) * 2 - 1, torch.rand((1, dt, h, w), generator=g) * 2 - 1)
            for dk, dt, h, w in shapes]


def make_store(vols, dtype):
    store = DD.DeviceVolumeStore(DEV, dtype)
    for i, (tk, tn) in enumerate(vols):
        store.add(tk, tn, category=f"c{i}", patient_id=f"p{i}")
    return store


def make_row(vols, v, z, y0, x0, flags, depth_thin):
    tk, tn = vols[v]
    d_thick, d_thin = tk.shape[1], tn.shape[1]
    z1 = min(z + depth_thin, d_thin)
    k0 = max(0, int(z * d_thick / d_thin))
    k1 = min(d_thick, max(int(z1 * d_thick / d_thin), k0 + 1))
    return [v, d_thin, d_thick, tn.shape[2], tn.shape[3], z, y0, x0, k0, k1, flags]


def check(sampler, vols, rows, dtype, interp_every=0):
    """One launch for all rows; thin bit for bit, thick within THICK_TOL of the float64 blend (and of F.interpolate on the
    device for every `interp_every`-th row).  Returns the largest thick error."""
    dt, dk, ph, pw = sampler.depth_thin, sampler.depth_thick, sampler.ph, sampler.pw
    thick, thin = sampler.sample(rows)
    torch.cuda.synchronize()
    want_thick, want_thin = PR.batch(vols, rows, dt, dk, ph, pw, dtype)
    assert thin.dtype == torch.float32 and tuple(thin.shape) == (rows.shape[0], 1, dt, ph, pw) and thin.is_contiguous()
    assert thick.dtype == torch.float32 and tuple(thick.shape) == (rows.shape[0], 1, dk, ph, pw)
    bad = (thin.cpu() != want_thin).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, f"thin patch differs in rows {[rows[i].tolist() for i in bad[:4]]}"
    err = (thick.cpu().double() - want_thick).abs().flatten(1).max(1).values
    print(f"patch-sample {dtype} {dt}/{dk} x {ph} x {pw}, {rows.shape[0]} rows: thick max |err| {float(err.max()):.3e} "
          f"(bound {PR.THICK_TOL:.3e})")
    assert float(err.max()) <= PR.THICK_TOL, [rows[i].tolist() for i in (err > PR.THICK_TOL).nonzero().flatten().tolist()[:4]]
    if interp_every:
        for i in range(0, rows.shape[0], interp_every):
            r = rows[i].tolist()
            y0, x0, fl = r[DD.C_Y0], r[DD.C_X0], r[DD.C_FLAGS]
            sub = sampler.store.thick[r[DD.C_VOL]][r[DD.C_K0]:r[DD.C_K1], y0:y0 + ph, x0:x0 + pw].float()
            ref = F.interpolate(sub[None, None], size=(dk, ph, pw), mode="trilinear", align_corners=False)[0]
            ref = PR.augment(ref, bool(fl & 1), bool(fl & 2), fl >> 2)
            e = float((thick[i] - ref).abs().max())
            assert e <= PR.THICK_TOL, (r, e)
    return float(err.max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("depths", [(12, 2), (48, 8)], ids=["12/2", "48/8"])
@pytest.mark.parametrize("side", [8, 20, 36, 68])
def test_sides_flags_offsets_widths(side, depths, dtype):
    """One batch mixing three volumes of different shapes: volume 0 is exactly the patch (depth, H, W), volume 1 is 5 wider
    (odd W: no two rows share an alignment), volume 2 is 6 wider and shallower than the patch (padded thin slices)."""
    dt, dk = depths
    shapes = [(dk, dt, side, side), (dk + 3, dt + 7, side + 3, side + 5), (max(dk // 2, 1), dt - 3, side + 2, side + 6)]
    vols = make_volumes(shapes, 100 + side)
    sampler = DD.DevicePatchSampler(make_store(vols, dtype), dt, dk, (side, side))
    rng = random.Random(side)
    rows = []
    for flags in range(16):
        rows.append(make_row(vols, 0, 0, 0, 0, flags, dt))
        for v in (1, 2):
            d_thin, h = shapes[v][1], shapes[v][2]
            for x0 in (0, 1, 3):
                rows.append(make_row(vols, v, rng.randint(0, max(d_thin - dt, 0)), rng.randint(0, h - side), x0, flags, dt))
    if dt == 48:        # the full cross product ran at 12/2: a third of it here, every flag combination still present
        rows = rows[::3] + rows[1::21]
        assert {r[DD.C_FLAGS] for r in rows} == set(range(16)) and {r[DD.C_X0] for r in rows} == {0, 1, 3}
    check(sampler, vols, torch.tensor(rows, dtype=torch.int64), dtype, interp_every=5)


def test_rectangular_patch_without_rotation():
    """ph != pw (augment off, or flips alone), pw no multiple of 4: the scalar store path and a tile that is wider than tall."""
    vols = make_volumes([(3, 20, 30, 90), (5, 31, 23, 77)], 9)
    for dtype in (torch.float32, torch.float16):
        sampler = DD.DevicePatchSampler(make_store(vols, dtype), 12, 2, (21, 70), augment=False)
        rows = [make_row(vols, v, z, y0, x0, flags, 12) for v, z, y0, x0 in ((0, 3, 2, 1), (0, 8, 9, 20), (1, 0, 0, 7), (1, 19, 2, 0))
                for flags in (0, 1, 2, 3)]
        check(sampler, vols, torch.tensor(rows, dtype=torch.int64), dtype, interp_every=3)
        bad = torch.tensor([make_row(vols, 0, 0, 0, 0, 4, 12)], dtype=torch.int64)
        with pytest.raises(ValueError, match="sample: row"):
            sampler.sample(bad)                                  # k = 1 on a rectangular patch


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_every_golden_item_through_the_kernel(dtype):
    """The reference's own items (padding, n_sub = 1, a thick range that ends at D_thick, H != W with W odd, a patch equal to
    the volume): fp32 storage reproduces them -- thin bit for bit, thick within THICK_TOL of the reference's fp32 result --
    and fp16 storage reproduces the restatement on the rounded volumes."""
    g = np.load(GOLDEN, allow_pickle=False)
    vols = [(torch.from_numpy(g[f"vol{v}_thick"]), torch.from_numpy(g[f"vol{v}_thin"])) for v in range(4)]
    dt, dk, ph, pw = (int(x) for x in g["config"])
    store = make_store(vols, dtype)
    cases = g["cases"].tolist()
    samplers = {a: DD.DevicePatchSampler(store, dt, dk, (ph, pw), augment=bool(a)) for a in (0, 1)}
    for aug in (0, 1):
        pick = [i for i, c in enumerate(cases) if c[2] == aug]
        rows = torch.cat([samplers[aug].draw([cases[i][0]], rng=random.Random(cases[i][1])) for i in pick])
        check(samplers[aug], vols, rows, dtype, interp_every=4)
        if dtype == torch.float32:
            thick, thin = samplers[aug].sample(rows)
            assert torch.equal(thin.cpu(), torch.from_numpy(g["thin"][pick]))
            assert float((thick.cpu() - torch.from_numpy(g["thick"][pick])).abs().max()) <= PR.THICK_TOL
        n_sub = (rows[:, DD.C_K1] - rows[:, DD.C_K0]).tolist()
        assert 1 in n_sub and max(n_sub) >= 2 and bool((rows[:, DD.C_Z] + dt > rows[:, DD.C_DTHIN]).any())


def test_real_size_batch_from_an_fp16_volume():
    """B = 4 at 48 / 8 x 192 x 192 from a 300 x 512 x 512 volume with 50 thick slices: nine tiles per slice, all four
    rotations, odd and even x0."""
    g = torch.Generator().manual_seed(3)
    thin = torch.rand((1, 300, 512, 512), generator=g) * 2 - 1
    thick = torch.rand((1, 50, 512, 512), generator=g) * 2 - 1
    vols = [(thick, thin)]
    store = make_store(vols, torch.float16)
    assert store.nbytes == 350 * 512 * 512 * 2 and len(store) == 1
    sampler = DD.DevicePatchSampler(store, 48, 8, (192, 192))
    rows = torch.tensor([make_row(vols, 0, 252, 320, 317, 0 << 2 | 1, 48), make_row(vols, 0, 0, 0, 0, 1 << 2, 48),
                         make_row(vols, 0, 100, 13, 130, 2 << 2 | 2, 48), make_row(vols, 0, 37, 200, 3, 3 << 2 | 3, 48)],
                        dtype=torch.int64)
    check(sampler, vols, rows, torch.float16, interp_every=2)
    drawn = sampler.draw([0, 0, 0, 0], rng=random.Random(1))
    check(sampler, vols, drawn, torch.float16)
