"""GPU: the patch sampler under the poison-and-guard harness (tests/poison.py).  The store's volumes, the device table and
both outputs are allocated inside guard bands pre-filled with 0x00 / 0xFF (NaN) / 0x7F: every output element is written
(the results are bit-identical to an unpoisoned run whatever the buffers held), nothing is stored outside them, and -- the
volumes sitting between guards too -- a gather that strays past a volume's first or last row reads the fill and shows up
as a difference.  Shapes off the tile and the 16-byte grid, both storage types, stored and measured thick patches."""
import importlib
import random

import pytest
import torch

from tests import patch_sampler_restatement as PR
from tests import poison as PZ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DD = importlib.import_module("video-to-video-diffusion_amd.device_data")
SHAPES = [(2, 12, 20, 20), (3, 17, 23, 27), (1, 9, 31, 22), (4, 30, 20, 85)]      # (D_thick, D_thin, H, W)


def test_poisoned_buffers():
    g = torch.Generator().manual_seed(8)
    vols = [(torch.rand((1, dk, h, w), generator=g) * 2 - 1, torch.rand((1, dt, h, w), generator=g) * 2 - 1)
            for dk, dt, h, w in SHAPES]
    rows_of = {}

    def f():
        out = {}
        for name, dtype in (("f16", torch.float16), ("f32", torch.float32)):
            store = DD.DeviceVolumeStore(DEV, dtype)
            for tk, tn in vols:
                store.add(tk, tn)
            sampler = DD.DevicePatchSampler(store, 12, 2, (20, 20))
            rng = random.Random(5)
            rows = torch.cat([sampler.draw([0, 1, 2, 3], rng=rng) for _ in range(8)])
            rows[:16, DD.C_FLAGS] = torch.arange(16)                    # every flag combination at least once
            rows_of[name] = rows
            out[name] = sampler.sample(rows)
            out[name + "_measure"] = DD.DevicePatchSampler(store, 12, 2, (20, 20), thick="measure").sample(rows)
        torch.cuda.synchronize()
        return out

    ref = PZ.run_scenario(f, name="patch-sampler[12/2 x 20 x 20]", ragged=True, expect_programs=False)
    for name, dtype in (("f16", torch.float16), ("f32", torch.float32)):
        thick, thin = ref[name]
        want_thick, want_thin = PR.batch(vols, rows_of[name], 12, 2, 20, 20, dtype)
        assert torch.equal(thin, want_thin) and torch.equal(ref[name + "_measure"][1], want_thin)
        assert float((thick.double() - want_thick).abs().max()) <= PR.THICK_TOL
        assert not torch.isnan(ref[name + "_measure"][0]).any()
