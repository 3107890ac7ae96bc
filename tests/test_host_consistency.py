"""CPU: the slice profile of the data-consistency layer (video-to-video-diffusion_amd/consistency.py) --
W, P = W^T (W W^T)^-1 and the band tables in float64, the refusals, the config section, the plain attributes on the model and
the samplers (never in the module tree or the state dict), the unchanged public signatures, and the CPU fallback of
`SliceProfile.measure` under gradcheck."""
import importlib
import inspect

import numpy as np
import pytest
import torch

from tests.helpers import TINY_CFG, TINY_UNET

CS = importlib.import_module("video-to-video-diffusion_amd.consistency")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")

DEPTHS = [(2, 12), (8, 48), (50, 300), (3, 8), (4, 10)]
PROFILES = {"box": dict(kind="box"), "pick": dict(kind="pick"), "gauss1.0": dict(kind="gaussian", fwhm=1.0),
            "gauss1.5": dict(kind="gaussian", fwhm=1.5)}


@pytest.mark.parametrize("depths", DEPTHS, ids=lambda d: f"{d[0]}to{d[1]}")
@pytest.mark.parametrize("name", sorted(PROFILES))
def test_profile_tables(depths, name):
    d_in, d_out = depths
    p = CS.SliceProfile(d_in, d_out, **PROFILES[name])
    assert p.W.shape == (d_in, d_out) and p.W.dtype == np.float64 and p.P.shape == (d_out, d_in) and p.P.dtype == np.float64
    assert (p.W >= 0).all() and np.abs(p.W.sum(axis=1) - 1.0).max() <= 1e-15
    err = np.abs(p.W @ p.P - np.eye(d_in)).sum(axis=1).max()
    print(f"{name} {d_in}->{d_out}: ||W P - I||inf = {err:.2e}, cond(W W^T) = {p.cond:.3g}")
    assert err <= 1e-12 and p.cond <= 28
    # the band tables bound the non-zeros exactly: first and last non-zero column, (0, -1) for an all-zero row
    for M, band in ((p.W, p.band_w), (p.P, p.band_p)):
        assert band.dtype == np.int32 and band.shape == (M.shape[0], 2)
        for row, (lo, hi) in zip(M, band):
            nz = np.flatnonzero(row)
            assert (lo, hi) == ((nz[0], nz[-1]) if nz.size else (0, -1))
    assert (p.band_w[:, 1] >= p.band_w[:, 0]).all()          # every row of W reads something
    # fp32 copies: each rounded once from float64
    assert p.W32.dtype == np.float32 and np.array_equal(p.W32, p.W.astype(np.float32))
    assert p.P32.dtype == np.float32 and np.array_equal(p.P32, p.P.astype(np.float32))
    r = d_out / d_in
    if name == "box":
        # centre of mass of row k = the centre of thick slice k in thin coordinates: the trilinear (align_corners=False) alignment
        # -- exactly, for every row whose slab ends on cell edges (all rows at an integer ratio) or mirrors itself about its
        # centre.  A slab edge inside a cell moves the row's discrete centre of mass: the cell counts at its own centre j, not at
        # the centre of the overlapped part, a shift of (f / r) (1 - f) / 2 <= 1 / (8 r) for an overlapped fraction f.  3 -> 8,
        # row 0: weights (1, 1, 2/3) / (8/3) give 0.875 against the slab centre 0.8333 (f = 2/3: 0.0417 <= 0.0469).
        com = p.W @ np.arange(d_out, dtype=np.float64)
        centre = (np.arange(d_in) + 0.5) * r - 0.5
        on_edges = np.array([(k * d_out) % d_in == 0 and ((k + 1) * d_out) % d_in == 0 for k in range(d_in)])
        mirrored = np.array([np.allclose(p.W[k], p.W[d_in - 1 - k][::-1], rtol=0, atol=1e-15) and 2 * k == d_in - 1
                             for k in range(d_in)])
        exact = on_edges | mirrored
        assert exact.all() or d_out % d_in != 0
        assert np.abs(com - centre)[exact].max(initial=0.0) <= 1e-12
        assert np.abs(com - centre).max() <= 1.0 / (8.0 * r) + 1e-12
        # the mass-weighted centres of the overlapped parts meet the slab centre for every row, fractional edges included
        jj = np.arange(d_out, dtype=np.float64)
        for k in range(d_in):
            lo, hi = np.maximum(jj - 0.5, k * r - 0.5), np.minimum(jj + 0.5, (k + 1) * r - 0.5)
            assert abs(float(np.sum(p.W[k] * np.where(p.W[k] > 0, 0.5 * (lo + hi), 0.0))) - centre[k]) <= 1e-12
        if d_out % d_in == 0:
            want = np.zeros((d_in, d_out))
            for k in range(d_in):
                want[k, k * int(r):(k + 1) * int(r)] = 1.0 / int(r)
            assert np.array_equal(p.W, want)
        else:
            assert ((p.W > 0) & (p.W < 1.0 / np.ceil(r))).any()      # fractional edge weights
    if name == "pick":
        centres = np.floor((np.arange(d_in) + 0.5) * r - 0.5 + 0.5).astype(int)
        assert np.array_equal(np.argmax(p.W, axis=1), centres) and (p.W.max(axis=1) == 1.0).all()


def test_gaussian_rows_in_closed_form():
    """The gaussian profile stated independently: row k is exp(-(j - c_k)^2 / (2 sigma^2)) around c_k = (k + 0.5) r - 0.5, its
    full width at half maximum is `fwhm` thick slices = fwhm * r thin ones, entries below 1e-4 of the peak are dropped, and the
    row is normalised."""
    import math
    for (d_in, d_out), fwhm, k in (((8, 48), 1.0, 3), ((2, 12), 1.5, 0), ((3, 8), 1.0, 1), ((50, 300), 1.5, 49)):
        p = CS.SliceProfile(d_in, d_out, kind="gaussian", fwhm=fwhm)
        r = d_out / d_in
        c = (k + 0.5) * r - 0.5
        sigma = fwhm * r / (2.0 * math.sqrt(2.0 * math.log(2.0)))          # FWHM = 2 sqrt(2 ln 2) sigma = 2.35482 sigma
        row = [math.exp(-0.5 * ((j - c) / sigma) ** 2) for j in range(d_out)]
        row = [v if v >= 1e-4 * max(row) else 0.0 for v in row]
        want = np.array(row) / sum(row)
        # 2.35482 against 2 sqrt(2 ln 2) = 2.3548200450...: 2e-8 relative in sigma, at most (d / sigma)^2 times that in a weight
        assert np.abs(p.W[k] - want).max() <= 1e-6 * want.max(), (d_in, d_out, fwhm)
        assert np.array_equal(p.W[k] > 0, want > 0)
        # the width recovered from two entries of the row itself: ln(W[j1] / W[j2]) = (d2^2 - d1^2) / (2 sigma^2)
        j1, j2 = int(math.floor(c)), int(math.floor(c)) + 2
        s2 = ((j2 - c) ** 2 - (j1 - c) ** 2) / (2.0 * math.log(p.W[k, j1] / p.W[k, j2]))
        assert abs(2.35482 * math.sqrt(s2) - fwhm * r) <= 1e-9 * fwhm * r
    # the cut-off: at 8 -> 48, fwhm 1.0, sigma = 2.548 thin slices and sqrt(2 ln 1e4) sigma = 10.94, so row 3 (c = 20.5) keeps 10 .. 31
    p = CS.SliceProfile(8, 48, kind="gaussian", fwhm=1.0)
    assert tuple(p.band_w[3]) == (10, 31) and p.W[3, 9] == 0.0 and p.W[3, 32] == 0.0
    assert abs(p.W[3, 10] / p.W[3, 20] - math.exp(-0.5 * (10.5 ** 2 - 0.5 ** 2) / (6.0 / 2.35482) ** 2)) <= 1e-12


def test_custom_matrix_is_validated_and_normalised():
    M = np.zeros((2, 6))
    M[0, :4], M[1, 2:] = 2.0, 1.0
    p = CS.SliceProfile(2, 6, matrix=M)
    assert p.kind == "matrix" and np.allclose(p.W.sum(axis=1), 1.0) and np.allclose(p.W[0, :4], 0.25)
    assert np.abs(p.W @ p.P - np.eye(2)).max() <= 1e-12
    assert np.array_equal(CS.SliceProfile(2, 6, matrix=torch.from_numpy(M)).W, p.W)
    for bad, msg in ((np.zeros((3, 6)), "shape"), (-M, "non-negative"), (M * np.nan, "finite"),
                     (np.vstack([M[0], np.zeros(6)]), "all zero")):
        with pytest.raises(ValueError, match=msg):
            CS.SliceProfile(2, 6, matrix=bad)


def test_refusals():
    with pytest.raises(ValueError, match="nothing to project"):
        CS.SliceProfile(8, 8)
    with pytest.raises(ValueError, match="d_in=9 > d_out=8"):
        CS.SliceProfile(9, 8)
    M = np.ones((2, 6))                                        # two equal rows: singular
    with pytest.raises(ValueError, match=r"cond = .*(inf|e\+)"):
        CS.SliceProfile(2, 6, matrix=M)
    with pytest.raises(ValueError, match=r"cond = \d\.\d+e\+\d+"):      # gaussian fwhm 4 at 50 -> 300: cond > 1e6
        CS.SliceProfile(50, 300, kind="gaussian", fwhm=4.0)
    with pytest.raises(L.CtsiError, match="d_in=65.*64"):
        CS.SliceProfile(65, 130)
    with pytest.raises(L.CtsiError, match="d_out=513.*512"):
        CS.SliceProfile(8, 513)
    for kw in (dict(kind="triangle"), dict(kind="gaussian"), dict(kind="gaussian", fwhm=-1.0), dict(kind="box", fwhm=1.0),
               dict(kind="gaussian", fwhm=True)):
        with pytest.raises(ValueError):
            CS.SliceProfile(2, 12, **kw)
    for kw in (dict(iterations=0), dict(iterations=1.5), dict(iterations=True), dict(clamp=(1.0, -1.0)), dict(clamp=(0.0,)),
               dict(clamp="x"), dict(clamp=(0.0, float("nan"))), dict(final="both"), dict(final="clamp"), dict(kind="nope"),
               dict(kind="gaussian")):
        with pytest.raises(ValueError):
            CS.DataConsistency(**kw)
    assert [CS.DataConsistency().clamp_mode, CS.DataConsistency(clamp=(-1, 1)).clamp_mode,
            CS.DataConsistency(clamp=(-1, 1), final="clamp").clamp_mode] == [0, 1, 2]
    dc = CS.DataConsistency()
    assert dc.last_stats is None and dc.profile(2, 12) is dc.profile(2, 12)
    with pytest.raises(L.CtsiError, match="ROCm"):
        dc.project(torch.zeros(1, 1, 4, 2, 2), torch.zeros(1, 1, 2, 2, 2))


def test_config_section(pkg):
    assert pkg.VideoToVideoDiffusion(TINY_CFG).data_consistency is None
    for sec in ({"enabled": False, "kind": "nope"}, {"enabled": "true", "kind": "nope"}, {"kind": "nope"}, "box"):
        assert pkg.VideoToVideoDiffusion(dict(TINY_CFG, data_consistency=sec)).data_consistency is None
    m = pkg.VideoToVideoDiffusion(dict(TINY_CFG, data_consistency={
        "enabled": True, "kind": "gaussian", "fwhm": 1.5, "iterations": 3, "clamp": [-1, 1], "final": "clamp"}))
    dc = m.data_consistency
    assert isinstance(dc, CS.DataConsistency) and (dc.kind, dc.fwhm, dc.iterations, dc.clamp, dc.final, dc.clamp_mode) == \
        ("gaussian", 1.5, 3, (-1.0, 1.0), "clamp", 2)
    assert pkg.VideoToVideoDiffusion(dict(TINY_CFG, data_consistency={"enabled": True})).data_consistency.kind == "box"
    for bad in ({"kind": "nope"}, {"kind": "gaussian"}, {"iterations": 0}, {"clamp": [1, -1]}, {"clamp": [0]},
                {"final": "clamp"}, {"final": "x"}, {"fwhm": 2.0}, {"colour": "red"}):
        with pytest.raises(ValueError):
            pkg.VideoToVideoDiffusion(dict(TINY_CFG, data_consistency=dict(bad, enabled=True)))


def test_attribute_is_plain(pkg):
    model = pkg.VideoToVideoDiffusion(TINY_CFG)
    keys, mods = set(model.state_dict()), [n for n, _ in model.named_modules()]
    model.data_consistency = CS.DataConsistency(clamp=(-1, 1))
    assert isinstance(model.data_consistency, CS.DataConsistency)
    assert set(model.state_dict()) == keys and [n for n, _ in model.named_modules()] == mods
    assert not any("consistency" in k for k in keys) and "data_consistency" not in dict(model.named_children())
    model.data_consistency = None
    assert model.data_consistency is None
    for bad in ("box", 1, lambda v, t: v, torch.nn.Identity()):
        with pytest.raises(ValueError, match="data_consistency must be None or a DataConsistency"):
            model.data_consistency = bad
    assert model.data_consistency is None
    g, un = pkg.GaussianDiffusion("cosine", 1000), pkg.UNet3D(**TINY_UNET)
    for sm in (S.DDIMSampler(g, un), S.DDPMSampler(g, un), S.DPMSolverSampler(g, un), S.HeunSampler(g, un)):
        assert sm.data_consistency is None
        sm.data_consistency = "box"         # a plain attribute: checked where it is used, before anything is sampled
        args = (torch.zeros(1, 1, 4, 32, 32), object()) if isinstance(sm, S.DDPMSampler) else (torch.zeros(1, 1, 4, 32, 32), object(), 3)
        for fusion in ("pixel",):
            with pytest.raises(ValueError, match="data_consistency must be None or a DataConsistency"):
                sm.sample_with_stitching(*args, patch_size=(4, 16, 16), target_patch_size=(12, 16, 16), stride=(2, 8, 8),
                                         device="cuda", progress=False, fusion=fusion)


def test_sharding_is_refused_before_any_work(pkg):
    model = pkg.VideoToVideoDiffusion(TINY_CFG)
    model.data_consistency = CS.DataConsistency()
    model.unet.depth_shard_comm = object()
    try:
        with pytest.raises(L.CtsiError, match="depth sharding"):
            model.generate(torch.zeros(1, 1, 2, 16, 16), "ddim", num_inference_steps=2, target_depth=4)
        sm = S.DDIMSampler(model.diffusion, model.unet)
        sm.data_consistency = CS.DataConsistency()
        with pytest.raises(L.CtsiError, match="depth sharding"):
            sm.sample_with_stitching(torch.zeros(1, 1, 4, 32, 32), model.vae, 3, patch_size=(4, 16, 16),
                                     target_patch_size=(12, 16, 16), stride=(2, 8, 8), device="cuda", progress=False)
    finally:
        del model.unet.depth_shard_comm
    # a target depth below the input depth is refused before any work as well (a CPU tensor never reaches the device check)
    with pytest.raises(ValueError, match="target_depth=1.*2 input slices"):
        model.generate(torch.zeros(1, 1, 2, 16, 16), "ddim", num_inference_steps=2, target_depth=1)
    with pytest.raises(ValueError, match="target patch depth 2.*4"):
        sm.sample_with_stitching(torch.zeros(1, 1, 4, 32, 32), model.vae, 3, patch_size=(4, 16, 16),
                                 target_patch_size=(2, 16, 16), stride=(2, 8, 8), device="cuda", progress=False)


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_public_signatures_are_what_they_were(pkg):
    E = inspect.Parameter.empty
    assert _params(pkg.VideoToVideoDiffusion.generate) == [
        ("self", E), ("v_in", E), ("sampler", E), ("num_inference_steps", 20), ("guidance_scale", 1.0), ("target_depth", None),
        ("noise_fn", None), ("precision", None), ("guidance_rescale", 0.0)]
    assert [n for n, _ in _params(S.run_sampler)] == [
        "diffusion", "model", "shape", "conditioning", "device", "kind", "t_desc", "progress", "eta", "noise_fn", "z_init",
        "trajectory", "order", "eps_trajectory", "heun", "guidance_scale", "guidance_rescale"]
    geo = [("patch_size", (8, 192, 192)), ("target_patch_size", (48, 192, 192)), ("stride", (4, 96, 96)), ("device", "cuda")]
    guided = [("guidance_scale", 1.0), ("guidance_rescale", 0.0)]
    tail = [("fusion", "pixel"), ("decode", None)]
    head = [("self", E), ("v_thick_full", E), ("vae", E)]
    assert _params(S.DDIMSampler.sample_with_stitching) == head + [("num_inference_steps", 20)] + geo + [
        ("eta", 0.0), ("progress", True), ("window_batch", None), ("dp_group", None)] + guided + tail
    for cls in (S.DPMSolverSampler, S.HeunSampler):
        assert _params(cls.sample_with_stitching) == head + [("num_inference_steps", 20)] + geo + [
            ("progress", True), ("window_batch", None), ("dp_group", None)] + guided + tail
    assert _params(S.DDPMSampler.sample_with_stitching) == head + geo + [("progress", True), ("dp_group", None)] + guided + [
        ("num_inference_steps", None), ("clip_denoised", True)] + tail


def test_measure_cpu_fallback_gradcheck():
    torch.manual_seed(0)
    for depths, kw in (((3, 8), PROFILES["box"]), ((2, 12), PROFILES["gauss1.5"])):
        p = CS.SliceProfile(*depths, **kw)
        x = torch.randn(2, 1, depths[1], 3, 2, dtype=torch.float64, requires_grad=True)
        assert torch.autograd.gradcheck(p.measure, (x,)) and torch.autograd.gradgradcheck(p.measure, (x,))
        y = p.measure(x.detach())
        assert y.shape == (2, 1, depths[0], 3, 2)
        assert torch.allclose(y, torch.einsum("kj,ncjhw->nckhw", torch.from_numpy(p.W), x.detach()), rtol=0, atol=1e-15)
        with pytest.raises(ValueError, match="measure"):
            p.measure(torch.zeros(1, 1, depths[1] + 1, 2, 2))
