"""GPU: the device patch loader end to end.  It feeds the tiny model's training step; the same seed gives the same batches and
the same loss bits; batches drawn back to back without a synchronisation match the restatement (the pinned staging ring is
reused under copies in flight); thick='measure' is SliceProfile.measure of the thin output; the store refuses a volume that
does not fit instead of letting the allocator fail."""
import importlib
import random

import pytest
import torch

from tests import patch_sampler_restatement as PR
from tests.helpers import formula_noise, tiny_model_sd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DD = importlib.import_module("video-to-video-diffusion_amd.device_data")
CS = importlib.import_module("video-to-video-diffusion_amd.consistency")
CtsiError = importlib.import_module("video-to-video-diffusion_amd.lib").CtsiError
SHAPES = [(5, 10, 20, 24), (3, 7, 16, 16), (8, 16, 33, 21), (4, 9, 18, 27), (6, 13, 16, 40)]      # (D_thick, D_thin, H, W)


@pytest.fixture(scope="module")
def vols():
    g = torch.Generator().manual_seed(21)
    return [(torch.rand((1, dk, h, w), generator=g) * 2 - 1, torch.rand((1, dt, h, w), generator=g) * 2 - 1)
            for dk, dt, h, w in SHAPES]


def make_store(vols, dtype=torch.float16, thick=True):
    store = DD.DeviceVolumeStore(DEV, dtype)
    for i, (tk, tn) in enumerate(vols):
        store.add(tk if thick else None, tn, category=f"c{i % 2}", patient_id=f"p{i}")
    return store


def test_loader_feeds_the_training_step_and_is_deterministic(pkg, vols):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    t = torch.tensor([612, 100], device=DEV)
    noise = formula_noise(-1, (2, 8, 4, 4, 4)).to(DEV)

    def epoch(seed):
        loader = DD.DevicePatchLoader(DD.DevicePatchSampler(make_store(vols), 4, 2, (16, 16)), batch_size=2, seed=seed)
        assert len(loader) == 2 and len(loader.dataset) == 5
        out = []
        for batch in loader:
            assert set(batch) == {"input", "target", "x_lr", "x_hr", "category", "patient_id"} and batch["input"] is batch["x_lr"]
            v_in, v_gt = batch["input"].to(DEV), batch["target"].to(DEV)
            assert v_in is batch["input"] and tuple(v_in.shape) == (2, 1, 2, 16, 16) and tuple(v_gt.shape) == (2, 1, 4, 16, 16)
            for p in model.parameters():
                p.grad = None
            loss, _ = model(v_in, v_gt, t=t, noise=noise)
            loss.backward()
            g = model.unet.conv_in.weight.grad
            assert torch.isfinite(loss) and torch.isfinite(g).all() and float(g.abs().max()) > 0
            out.append((v_in.cpu(), v_gt.cpu(), loss.detach().cpu(), batch["patient_id"]))
        return out

    a, b, c = epoch(42), epoch(42), epoch(43)
    for x, y in zip(a, b):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[3] == y[3]
        assert x[2].view(torch.int32).item() == y[2].view(torch.int32).item()
    assert any(not torch.equal(x[1], y[1]) for x, y in zip(a, c))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_batches_back_to_back_match_the_restatement(vols, dtype):
    """Six batches of different sizes with no synchronisation in between: more than the ring has slots, so slots are rewritten
    while earlier launches may still be queued."""
    sampler = DD.DevicePatchSampler(make_store(vols, dtype), 4, 2, (16, 16), seed=9)
    rng = random.Random(4)
    drawn, got = [], []
    for n in (3, 5, 1, 4, 2, 5):
        rows = sampler.draw([rng.randrange(len(vols)) for _ in range(n)])
        drawn.append(rows)
        got.append(sampler.sample(rows))
    torch.cuda.synchronize()
    for rows, (thick, thin) in zip(drawn, got):
        want_thick, want_thin = PR.batch(vols, rows, 4, 2, 16, 16, dtype)
        assert torch.equal(thin.cpu(), want_thin)
        assert float((thick.cpu().double() - want_thick).abs().max()) <= PR.THICK_TOL


@pytest.mark.parametrize("profile", [None, dict(kind="gaussian", fwhm=1.0)], ids=["box", "gaussian"])
def test_measure_mode_is_the_slice_profile_of_the_thin_patch(vols, profile):
    store = make_store(vols, torch.float32, thick=False)
    sampler = DD.DevicePatchSampler(store, 6, 2, (16, 16), thick="measure", profile=profile, seed=1)
    rows = sampler.draw([0, 1, 2, 3, 4])
    thick, thin = sampler.sample(rows)
    _, want_thin = PR.batch(vols, rows, 6, 2, 16, 16, torch.float32, with_thick=False)
    assert torch.equal(thin.cpu(), want_thin) and tuple(thick.shape) == (5, 1, 2, 16, 16)
    assert torch.equal(thick, CS.SliceProfile(2, 6, **(profile or {})).measure(thin))
    W = torch.from_numpy(sampler.profile.W)
    ref = torch.einsum("kj,ncjhw->nckhw", W, want_thin.double())
    assert float((thick.cpu().double() - ref).abs().max()) <= 1e-6
    with pytest.raises(ValueError, match="no thick acquisition"):
        DD.DevicePatchSampler(store, 6, 2, (16, 16)).draw([0])


def test_store_bookkeeping_and_the_capacity_error(vols, tmp_path):
    store = make_store(vols[:2])
    assert len(store) == 2 and store.categories == ["c0", "c1"] and store.patient_ids == ["p0", "p1"]
    assert store.nbytes == sum((dk + dt) * h * w for dk, dt, h, w in SHAPES[:2]) * 2
    torch.save({"thick": vols[2][0], "thin": vols[2][1], "category": "APE", "patient_id": "case_7"}, tmp_path / "case_7.pt")
    assert store.add_file(tmp_path / "case_7.pt") == 2 and store.patient_ids[2] == "case_7" and store.shape(2) == (16, 8, 33, 21)
    assert torch.equal(store.thin[2].cpu(), vols[2][1][0].half())
    with pytest.raises(ValueError, match="differ in H, W"):
        store.add(vols[0][0], vols[1][1])
    with pytest.raises(ValueError, match=r"\(1, D, H, W\)"):
        store.add(vols[0][0][0], vols[0][1])
    # asking is enough: a meta tensor has a shape and no bytes, and the check comes before any allocation
    free, total = torch.cuda.mem_get_info(torch.device(DEV))
    huge = torch.empty((1, total // (512 * 512) + 1, 512, 512), device="meta")         # more than the whole device as fp16
    held, count = store.nbytes, len(store)
    with pytest.raises(CtsiError, match=r"thin volume of patient 'big'.*holds \d+ bytes in 3 volumes.*\d+ bytes free"):
        store.add(None, huge, patient_id="big")
    assert store.nbytes == held and len(store) == count
    assert torch.cuda.mem_get_info(torch.device(DEV))[0] >= free - (64 << 20)
