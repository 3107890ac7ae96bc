"""GPU: the bf16x3 inference mode through the public interface (engine_x3.py on csrc/conv_bf16x3.hip).

Truth is the oracle in float64 on the device.  For every network-level output, with
  e32     = the fp32 oracle's rel-L2 distance to the truth,
  e_split = the float64 oracle's, with every convolution restated as the three split products (tests/x3_restatement.py),
  ebf     = the bf16 engine's on the same inputs,
  e       = the bf16x3 engine's,
the criterion is   e <= 2 e_split + max(4 e32, 2e-7)   and   e <= ebf / 32.
The factor 2: the engine's roundings and the restatement's are different draws of the same error process, equal in size only
statistically.  4 x e32 with the 2e-7 floor is the fp32 mode's rule (tests/test_gpu_fp32_mode.py); 32 leaves a factor 16 under
the ratio of about 500 between one-term bf16 and the split.  Trajectories add 1e-6 to both, as the fp32 mode's do.

DDIM and DDPM trajectories use the oracle's own float64 samplers.  The oracle has no DPM-Solver++, Heun, guidance or v-prediction
sampler: for those the truth runs the package's generic-callable loop (sampler._run_generic) around the float64 oracle U-Net --
the network evaluation, which is what this mode changes, is float64; the elementwise update is the fp32 mode's ctsi_*_step_f32,
whose own tests check it against float64 to a few 2^-24.  e32 and e_split run the same loop, so all four numbers share it."""
import contextlib
import importlib

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops as R
from tests import fwd_audit as FA
from tests import resblock_restatement as RR
from tests.helpers import (FULL_UNET_CFG, MID_UNET, TINY_UNET, build_prod_vae, formula_input, load_formula, rel_l2,
                           tiny_model_sd, unet_cfg)
from tests.x3_restatement import split, x3_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = importlib.import_module("video-to-video-diffusion_amd.engine")
EX = importlib.import_module("video-to-video-diffusion_amd.engine_x3")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
FLOOR = 2e-7
F64 = torch.float64


@pytest.fixture(autouse=True)
def _convt_as_forward_conv(monkeypatch):
    monkeypatch.setattr(R, "CONVT_AS_CONV", True)     # (see tests/test_gpu_fullsize.py: MIOpen's fp32 ConvT search)


@contextlib.contextmanager
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


@contextlib.contextmanager
def _precision(*modules, value="bf16x3"):
    old = [m.inference_precision for m in modules]
    for m in modules:
        m.inference_precision = value
    try:
        yield
    finally:
        for m, o in zip(modules, old):
            m.inference_precision = o


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale


def _noise_fn(i, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 + i), dtype=torch.float32).to(DEV)


def _cast(sd, dtype):
    return {k: (v.to(device=DEV, dtype=dtype) if v.is_floating_point() else v.to(DEV)) for k, v in sd.items()}


KINDS = ("f64", "f32", "split")          # the truth, the fp32 oracle, the float64 oracle under the split shim


@contextlib.contextmanager
def _oracle(kind):
    with contextlib.ExitStack() as st:
        if kind != "f32":
            st.enter_context(float64_default())
        if kind == "split":
            st.enter_context(x3_oracle())
        yield torch.float32 if kind == "f32" else F64


def _three(fn):
    """fn(sd caster, dtype) evaluated as the truth, the fp32 oracle and the split restatement."""
    out = {}
    for kind in KINDS:
        with _oracle(kind) as dt:
            out[kind] = fn(dt)
    return out["f64"], out["f32"], out["split"]


def _criterion(tag, got, got_bf, t64, o32, osp, extra=0.0):
    e32, es, ebf, e = rel_l2(o32, t64), rel_l2(osp, t64), rel_l2(got_bf, t64), rel_l2(got, t64)
    print(f"{tag}: bf16x3 engine {e:.3g}, split restatement {es:.3g}, fp32 oracle {e32:.3g}, bf16 engine {ebf:.3g} "
          f"(bf16 / bf16x3 = {ebf / max(e, 1e-30):.0f})")
    assert bool(torch.isfinite(got).all())
    assert e <= 2.0 * es + max(4.0 * e32, FLOOR) + extra, f"{tag}: {e:.3g} > 2 x {es:.3g} + max(4 x {e32:.3g}, {FLOOR}) + {extra}"
    assert e <= ebf / 32.0 + extra, f"{tag}: {e:.3g} > bf16 engine {ebf:.3g} / 32 + {extra}"


# ---------------------------------------------------------------------------------------------------------------------
# 1. U-Net forward
# ---------------------------------------------------------------------------------------------------------------------
def _unet_case(un, sd, cfg, shape, tvals, tag):
    x, c = _randn(shape, 5).to(DEV), _randn(shape, 6).to(DEV)
    t = torch.tensor(tvals, device=DEV)
    with _precision(un):
        got = un(x, t, c)
    got_bf = un(x, t, c)
    t64, o32, osp = _three(lambda dt: R.unet_forward(_cast(sd, dt), cfg, x.to(dt), t, c.to(dt)))
    _criterion(tag, got, got_bf, t64, o32, osp)


@pytest.mark.parametrize("kw, shape, tvals", [(TINY_UNET, (2, 8, 4, 8, 8), [500, 37]), (MID_UNET, (1, 4, 4, 16, 16), [500])],
                         ids=["tiny", "mid"])
def test_unet_forward(pkg, kw, shape, tvals):
    un = pkg.UNet3D(**kw)
    sd = load_formula(un, 8)
    un.to(DEV)
    _unet_case(un, sd, unet_cfg(kw), shape, tvals, f"U-Net {shape}")
    E.invalidate_engine_cache(un)


@pytest.fixture(scope="module")
def prod_unet(pkg):
    torch.manual_seed(0)
    un = pkg.UNet3D(latent_dim=8, model_channels=128, num_res_blocks=2, attention_levels=[1, 2], channel_mult=(1, 2, 4, 4),
                    num_heads=4, time_embed_dim=512).to(DEV).eval()
    yield un, {k: v.detach() for k, v in un.state_dict().items()}
    E.invalidate_engine_cache(un)


@pytest.mark.parametrize("tval", [500, 999])
def test_unet_forward_production_widths(prod_unet, tval):
    un, sd = prod_unet
    _unet_case(un, sd, FULL_UNET_CFG, (1, 8, 6, 16, 16), [tval], f"production U-Net t={tval}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. VAE
# ---------------------------------------------------------------------------------------------------------------------
def _vae_case(vae, sd, prefix, v, tag):
    with _precision(vae):
        z = vae.encode(v)
        out = vae.decode(z)
    z_bf = vae.encode(v)
    out_bf = vae.decode(z)          # the same latent for every decoder
    sf = float(vae.scaling_factor)
    _criterion(f"{tag} encode", z, z_bf, *_three(lambda dt: R.vae_encode(_cast(sd, dt), v.to(dt), sf, prefix)))
    _criterion(f"{tag} decode", out, out_bf, *_three(lambda dt: R.vae_decode(_cast(sd, dt), z.to(dt), sf, prefix)))


def test_vae_tiny(pkg):
    model, sd, _ = tiny_model_sd(pkg)
    model.to(DEV)
    v = (torch.rand((1, 1, 4, 16, 16), generator=torch.Generator().manual_seed(2)) * 2 - 1).to(DEV)
    _vae_case(model.vae, sd, "vae.", v, "tiny VAE")
    model.invalidate_engine_cache()


def test_vae_production_widths(pkg):
    """Encode (1,1,4,32,32) and decode (1,8,4,8,8): the 1-channel stem, the 1-channel tanh head and both strided geometries at
    128 / 256 / 512 channels."""
    vae = build_prod_vae(pkg, DEV)
    sd = {k: v.detach() for k, v in vae.state_dict().items()}
    v = (torch.rand((1, 1, 4, 32, 32), generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    _vae_case(vae, sd, "", v, "production VAE")
    E.invalidate_engine_cache(vae)


# ---------------------------------------------------------------------------------------------------------------------
# 3. trajectories on the tiny model
# ---------------------------------------------------------------------------------------------------------------------
SHAPE = (1, 8, 4, 8, 8)
STEPS = 4


@pytest.fixture(scope="module")
def tiny(pkg):
    model, sd, cfg = tiny_model_sd(pkg)
    model.to(DEV)
    yield model, sd, cfg
    model.invalidate_engine_cache()


def _net(sd, cfg, kind, prefix="unet.", wrap=contextlib.nullcontext):
    """The oracle U-Net as a callable for the package's generic loop; the default dtype and the shim are set per call only, so
    the loop around it runs as it always does."""
    dt = torch.float32 if kind == "f32" else F64
    sdx = _cast(sd, dt)

    def net(z, t, c):
        with _oracle(kind), wrap():
            return R.unet_forward(sdx, cfg, z.to(dt), t.to(dt) if t.is_floating_point() else t, c.to(dt), prefix)
    return net


def _check_traj(tag, traj, traj_bf, refs):
    r64, r32, rsp = refs
    assert len(traj) == len(traj_bf) == len(r64) == len(r32) == len(rsp) and len(traj) >= STEPS
    for i in range(len(traj)):
        _criterion(f"{tag} latent {i}", traj[i], traj_bf[i], r64[i], r32[i], rsp[i], extra=1e-6)


def _engine_traj(unet, run):
    """run(trajectory) under bf16x3 and under bf16."""
    traj, traj_bf = [], []
    with _precision(unet):
        run(traj)
    run(traj_bf)
    return traj, traj_bf


@pytest.mark.parametrize("kind", ["ddim", "ddim_eta", "ddpm"])
def test_oracle_sampler_trajectories(pkg, tiny, kind):
    """DDIM, DDIM eta = 0.7 and DDPM, 4 steps from t = T - 1, against the oracle's float64 samplers."""
    model, sd, cfg = tiny
    cond = _randn(SHAPE, 21).to(DEV)
    eta = 0.7 if kind == "ddim_eta" else 0.0

    def run(traj):
        if kind == "ddpm":
            pkg.DDPMSampler(model.diffusion, model.unet).sample(SHAPE, cond, DEV, progress=False, noise_fn=_noise_fn,
                                                                num_steps=STEPS, trajectory=traj)
        else:
            pkg.DDIMSampler(model.diffusion, model.unet).sample(SHAPE, cond, STEPS, DEV, eta=eta, progress=False,
                                                                noise_fn=_noise_fn, trajectory=traj)

    def ref(dt):
        sdx = _cast(sd, dt)
        bufs = {k[len("diffusion."):]: v for k, v in sdx.items() if k.startswith("diffusion.")}
        net = lambda z, t, c: R.unet_forward(sdx, cfg, z, t, c, "unet.")
        nf = lambda i, shp: _noise_fn(i, shp).to(dt)
        traj = []
        if kind == "ddpm":
            R.ddpm_sample(net, bufs, SHAPE, cond.to(dt), noise_fn=nf, num_steps=STEPS, trajectory=traj)
        else:
            R.ddim_sample(net, bufs, SHAPE, cond.to(dt), STEPS, eta=eta, noise_fn=nf, trajectory=traj)
        return traj

    traj, traj_bf = _engine_traj(model.unet, run)
    _check_traj(kind, traj, traj_bf, _three(ref))


def _generic_refs(make_sampler, sd, cfg, sample, prefix="unet.", wrap=contextlib.nullcontext):
    """The package's generic-callable loop around the oracle U-Net in float64, fp32 and float64 under the split shim."""
    out = []
    for kind in KINDS:
        traj = []
        sample(make_sampler(_net(sd, cfg, kind, prefix, wrap)), traj)
        out.append(traj)
    return tuple(out)


@pytest.mark.parametrize("kind", ["dpmpp_2m", "heun", "guided"])
def test_generic_sampler_trajectories(pkg, tiny, kind):
    """DPM-Solver++(2M), Heun, and a guided DDIM run (guidance_scale 3, guidance_rescale 0.7) on the captured step graph."""
    model, sd, cfg = tiny
    cond, z_t = formula_input(SHAPE, 60).to(DEV), _randn(SHAPE, 61).to(DEV)
    cls = dict(dpmpp_2m=pkg.DPMSolverSampler, heun=pkg.HeunSampler, guided=pkg.DDIMSampler)[kind]
    kw = dict(guidance_scale=3.0, guidance_rescale=0.7) if kind == "guided" else {}
    sample = lambda sampler, traj: sampler.sample(SHAPE, cond, STEPS, DEV, progress=False, z_init=z_t, trajectory=traj, **kw)
    traj, traj_bf = _engine_traj(model.unet, lambda tr: sample(cls(model.diffusion, model.unet), tr))
    keys = [k for k in model.unet._ctsi_programs if "bf16x3" in k]
    assert keys and all(k[0].startswith("sampler") for k in keys)              # the captured step program, not the generic loop
    _check_traj(kind, traj, traj_bf, _generic_refs(lambda net: cls(model.diffusion, net), sd, cfg, sample))


def test_v_prediction_x0_form_on_the_rescaled_schedule(pkg):
    base, sd, cfg = tiny_model_sd(pkg)
    m = pkg.VideoToVideoDiffusion({**base.config, 'prediction_type': 'v_prediction', 'zero_terminal_snr': True}).eval()
    full = base.state_dict()
    full.update({"diffusion." + k: v for k, v in m.diffusion.state_dict().items()})
    m.load_state_dict(full, strict=True)
    m.to(DEV)
    assert m.diffusion.update_form == "x0" and float(m.diffusion.alphas_cumprod[-1]) == 0.0
    cond, z_t = formula_input(SHAPE, 62).to(DEV), _randn(SHAPE, 63).to(DEV)
    sample = lambda sampler, traj: sampler.sample(SHAPE, cond, STEPS, DEV, progress=False, z_init=z_t, trajectory=traj)
    traj, traj_bf = _engine_traj(m.unet, lambda tr: sample(pkg.DDIMSampler(m.diffusion, m.unet), tr))
    keys = [k for k in m.unet._ctsi_programs if "bf16x3" in k]
    assert keys and all("x0" in k for k in keys)
    _check_traj("v-prediction x0", traj, traj_bf,
                _generic_refs(lambda net: pkg.DDIMSampler(m.diffusion, net), sd, cfg, sample))
    m.invalidate_engine_cache()


def test_scale_shift_resblocks(pkg):
    """use_scale_shift_norm=True: the middle pass is ctsi_gn_apply_mod_f32 between two bf16x3 convs."""
    un = pkg.UNet3D(**TINY_UNET, use_scale_shift_norm=True)
    sd = load_formula(un, 9)
    un.to(DEV)
    g = pkg.GaussianDiffusion().to(DEV)
    cfg = unet_cfg(TINY_UNET)
    cond, z_t = formula_input(SHAPE, 64).to(DEV), _randn(SHAPE, 65).to(DEV)
    sample = lambda sampler, traj: sampler.sample(SHAPE, cond, STEPS, DEV, progress=False, z_init=z_t, trajectory=traj)
    traj, traj_bf = _engine_traj(un, lambda tr: sample(pkg.DDIMSampler(g, un), tr))
    _check_traj("scale-shift", traj, traj_bf,
                _generic_refs(lambda net: pkg.DDIMSampler(g, net), sd, cfg, sample, prefix="", wrap=RR.resblock_options))
    # and the single-step API on the same model
    x, c = _randn(SHAPE, 66).to(DEV), _randn(SHAPE, 67).to(DEV)
    t = torch.tensor([321], device=DEV)
    with _precision(un):
        got = un(x, t, c)
    got_bf = un(x, t, c)
    _criterion("scale-shift forward", got, got_bf,
               *_three(lambda dt: RR.unet_forward(_cast(sd, dt), cfg, x.to(dt), t, c.to(dt))))
    E.invalidate_engine_cache(un)


# ---------------------------------------------------------------------------------------------------------------------
# 4. stitching, isolation, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_stitching_equals_window_by_window(pkg, tiny):
    model = tiny[0]
    with _precision(model.unet, model.vae):
        sampler = pkg.DDIMSampler(model.diffusion, model.unet)
        vol = (torch.rand((1, 1, 4, 32, 48), generator=torch.Generator().manual_seed(4)) * 2 - 1).to(DEV)   # 2 windows along w
        kw = dict(num_inference_steps=3, patch_size=(4, 32, 32), target_patch_size=(4, 32, 32), stride=(4, 16, 16),
                  device=DEV, progress=False)
        torch.manual_seed(9)
        batched = sampler.sample_with_stitching(vol, model.vae, window_batch=0, **kw)
        torch.manual_seed(9)
        single = sampler.sample_with_stitching(vol, model.vae, window_batch=1, **kw)
    err = rel_l2(batched, single)
    print(f"bf16x3 stitching: two windows as one batch vs one by one rel-L2 {err:.3g}")
    assert bool(torch.isfinite(batched).all()) and err < 1e-5          # the fp32 mode's batch-invariance bound
    assert any("bf16x3" in k and k[0].startswith("sampler") for k in model.unet._ctsi_programs)


def test_precision_isolation_in_one_process(pkg):
    v = (torch.rand((1, 1, 4, 32, 32), generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)

    def fresh():
        model, _, _ = tiny_model_sd(pkg)
        return model.to(DEV)

    run = lambda model, prec: model.generate(v, 'ddim', num_inference_steps=4, target_depth=8, noise_fn=_noise_fn,
                                             precision=prec)
    alone = {}
    for prec in ("bf16", "fp32", "bf16x3"):
        E._PACKED.clear()                       # no packed image survives from another precision
        m = fresh()
        alone[prec] = run(m, prec)
        m.invalidate_engine_cache()
        del m
    E._PACKED.clear()
    model = fresh()
    together = {prec: run(model, prec) for prec in ("fp32", "bf16x3", "bf16")}
    assert model.unet.inference_precision == "bf16" and model.vae.inference_precision == "bf16"
    for prec in alone:
        assert torch.equal(alone[prec], together[prec]), prec
    assert not torch.equal(together["bf16x3"], together["fp32"]) and not torch.equal(together["bf16x3"], together["bf16"])
    assert torch.equal(run(model, "bf16x3"), together["bf16x3"])
    # every weight image a bf16x3 program reads sits in the cache under a key led by "bf16x3"; no other program reads one
    by_ptr = {t.data_ptr(): key for cache in E._PACKED.values() for key, t in cache.items()}
    seen = 0
    for mod in (model.unet, model.vae):
        for key, prog in mod._ctsi_programs.items():
            for meta in prog._pack_meta:
                img = meta["holder"][0]
                if img is None or not prog.weight_cache:
                    continue
                lead = by_ptr[img.data_ptr()][0][0]
                assert (lead == "bf16x3") == ("bf16x3" in key), (key, lead)
                seen += "bf16x3" in key
    assert seen > 0
    model.invalidate_engine_cache()


def test_refusals_name_the_precision(pkg, tiny):
    model = tiny[0]
    x = torch.zeros(SHAPE, device=DEV)
    t = torch.tensor([10], device=DEV)
    with _precision(model.unet, model.vae):
        for mode in ("exact", "softmax"):
            model.unet.attention_mode = mode
            try:
                with pytest.raises(L.CtsiError, match="bf16x3.*fast"):
                    model.unet(x, t, x)
                with pytest.raises(L.CtsiError, match="bf16x3.*fast"):
                    pkg.DDIMSampler(model.diffusion, model.unet).sample(SHAPE, x, 2, DEV, progress=False)
            finally:
                model.unet.attention_mode = "fast"

        class _Comm:
            world, rank = 2, 0

        model.unet.depth_shard_comm = _Comm()
        model.vae.depth_shard_comm = _Comm()
        try:
            with pytest.raises(L.CtsiError, match="bf16x3.*sharding"):
                pkg.DDIMSampler(model.diffusion, model.unet).sample(SHAPE, x, 2, DEV, progress=False)
            with pytest.raises(L.CtsiError, match="bf16x3.*sharding"):
                model.vae.decode(torch.zeros(SHAPE, device=DEV))
        finally:
            del model.unet.depth_shard_comm, model.vae.depth_shard_comm
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope():
        with pytest.raises(L.CtsiError, match="bf16x3.*sharding"):
            EX.UNetProgramX3(ctx, model.unet, 1, 4, 8, 8, 1, "fast", shard=object())
        with pytest.raises(L.CtsiError, match="bf16x3.*sharding"):
            EX.VAEDecodeProgramX3(ctx, model.vae, 1, 4, 8, 8, shard=object())


def test_training_keeps_the_bf16_programs(pkg):
    from tests.helpers import formula_noise
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    v_in = formula_input((1, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    v_gt = formula_input((1, 1, 4, 16, 16), 19).clamp(-1, 1).to(DEV)
    t, nz = torch.tensor([612], device=DEV), formula_noise(-1, (1, 8, 4, 4, 4)).to(DEV)
    loss = lambda: float(model(v_in, v_gt, t=t, noise=nz)[0].detach())
    base = loss()
    model.set_inference_precision("bf16x3")
    try:
        pinned = loss()
    finally:
        model.set_inference_precision("bf16")
    assert pinned == base
    for m in (model.unet, model.vae):
        keys = list(m.__dict__.get("_ctsi_programs", {}))
        assert keys and not any("bf16x3" in k for k in keys), keys
    model.invalidate_engine_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 5. every conv launch of a program, from its own operands
# ---------------------------------------------------------------------------------------------------------------------
def _chk_conv_fwd_x3(rec, sn, R_, ctx):
    """One conv_fwd_x3 launch against the split restatement of that layer (criteria 1-3 of tests/test_gpu_bf16x3_conv.py)."""
    x = sn["x1"] if sn["x2"] is None else torch.cat([sn["x1"], sn["x2"]], -1)
    x = x.permute(0, 4, 1, 2, 3)
    w = sn["weight"].detach().to(torch.float32)
    conv = lambda a, b: FA.conv64(a, b, rec["s"], rec["p"], rec["transposed"], ctx["budget"])
    (xh, xl), (wh, wl) = split(x.to(F64)), split(w.to(F64))
    ybf = conv(xh, wh)
    ys = ybf + (conv(xh, wl) + conv(xl, wh))
    y64 = conv(x, w)
    fn = F.conv_transpose3d if rec["transposed"] else F.conv3d
    with torch.backends.cudnn.flags(enabled=False):
        y32 = fn(x.contiguous(), w, None, stride=(1,) + tuple(rec["s"]), padding=tuple(rec["p"])).to(F64)
    refs = [y64, y32, ys, ybf]
    if sn["bias"] is not None:
        refs = [y + sn["bias"].to(F64)[:y.shape[1]].view(1, -1, 1, 1, 1) for y in refs]
    rows = []
    if sn.get("residual") is not None:
        refs = [y + sn["residual"].to(F64).permute(0, 4, 1, 2, 3) for y in refs]
    if rec["act"] == 1:
        refs = [torch.tanh(y) for y in refs]
    y64, y32, ys, ybf = refs
    if rec["f32_out"] is not None:
        out = torch.as_strided(rec["f32_out"], tuple(y64.shape), rec["f32_strides"])
    else:
        out = FA.act_ndhwc(rec["out"]).permute(0, 4, 1, 2, 3)
    if rec["stats"] is not None:           # the slab holds the sums of the stored values: a float64 reduction of them, 1e-5
        st = rec["stats"]
        s1, s2 = FA._slab_totals(FA._val(rec["colsum"]), 0, y64.shape[0], st["tps"], st["cpad"], st["nclass"], y64.shape[1])
        o64 = out.to(F64)
        for what, got, ref in (("colsum1", s1, o64.sum((2, 3, 4))), ("colsum2", s2, (o64 * o64).sum((2, 3, 4)))):
            err = rel_l2(got, ref)
            rows.append(R_(what, got, dict(cls="sum", rel_l2=err, max_rel=err, ulps=float("nan"), ok=err < 1e-5)))
    e32, es, ebf = rel_l2(y32, y64), rel_l2(ys, y64), rel_l2(ybf, y64)
    e, eacc = rel_l2(out, y64), rel_l2(out, ys)
    ok = e <= es + max(4.0 * e32, FLOOR) and eacc <= es and e <= ebf / 32.0
    print(f"    conv_fwd_x3 {tuple(out.shape)}: e {e:.3g}, to the restatement {eacc:.3g}, e_split {es:.3g}, e32 {e32:.3g}, "
          f"one-term {ebf:.3g}  {'ok' if ok else 'FAIL'}")
    rows.append(R_("y", out, dict(cls="x3", rel_l2=e, max_rel=eacc, ulps=float("nan"), ok=bool(ok))))
    return rows


def _audit(monkeypatch, prog, tag):
    monkeypatch.setitem(FA.REFS, "conv_fwd_x3", _chk_conv_fwd_x3)
    monkeypatch.setitem(FA._INPUTS, "conv_fwd_x3", FA._INPUTS["conv_fwd"])
    rows, missing = FA.audit_forward(prog)
    x3 = [r for r in rows if r["cls"] == "x3"]
    print(FA.format_table(f"{tag}: {len(x3)} bf16x3 conv launches, {len(rows)} checked outputs", [r for r in rows if not r["ok"]]))
    assert not missing, missing
    assert x3 and all(r["ok"] for r in rows), [(r["op"], r["name"], r["what"]) for r in rows if not r["ok"]]
    kinds = [a.get("kind") for a in prog.op_audit if a is not None]
    assert "conv_fwd" not in kinds                  # every layer runs on the bf16x3 kernel
    assert len(x3) == kinds.count("conv_fwd_x3")


def test_every_conv_launch_of_a_unet_program(pkg, tiny, monkeypatch):
    model = tiny[0]
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope():
        prog = EX.UNetProgramX3(ctx, model.unet, 2, 4, 8, 8, 2, "fast")
        prog.load_latents(_randn((2,) + SHAPE[1:], 70).to(DEV), _randn((2,) + SHAPE[1:], 71).to(DEV))
        prog.set_schedule([500, 37])
    _audit(monkeypatch, prog, "tiny U-Net")


def test_every_conv_launch_of_a_vae_decode_program(pkg, tiny, monkeypatch):
    model = tiny[0]
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope():
        prog = EX.VAEDecodeProgramX3(ctx, model.vae, 1, 3, 5, 6)
        prog(_randn((1, 8, 3, 5, 6), 72).to(DEV))
    _audit(monkeypatch, prog, "tiny VAE decode")
