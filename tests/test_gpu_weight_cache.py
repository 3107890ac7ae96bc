"""GPU: packed-weight images shared between programs (engine._PACKED, keyed by engine._pack_sig / engine_f32._f32_pack_sig).

A cache hit skips packing, so two plans that pack differently must never meet under one key: a program's output must not
depend on what was built before it in the same process, and every hit must hand out the bytes a fresh pack would write.
  * the pack-layout property: every conv the production networks emit, at three latent sizes, seven batch sizes and the
    depth-sharded views -- plans with equal keys pack byte-identical images (only pack kernels run here)
  * a full-width U-Net evaluated at two batch sizes whose level-0 convs take differently packed k32 tiles, in both orders,
    against the fp32 oracle and against the same evaluation on a fresh cache
  * the user-facing case: sample_with_stitching (13 windows per batch) after generate() on one 192^2 patch
"""
import ctypes as C
import gc
import importlib

import pytest
import torch

from oracle import ref_ops as R
from tests.helpers import LEGACY163_UNET, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NET_TOL = 3e-2
UNET_CFG = dict(model_channels=128, num_res_blocks=2, attention_levels=[1, 2], channel_mult=[1, 2, 4, 4], num_heads=4,
                scaling_factor=1.0)
FULL_CFG = {'model': {'in_channels': 1, 'latent_dim': 8, 'vae_base_channels': 128, 'vae_scaling_factor': 1.0},
            'pretrained': {'use_pretrained': True, 'vae': {'enabled': True, 'checkpoint_path': 'unused'}},
            'noise_schedule': 'cosine', 'diffusion_timesteps': 1000}
E = importlib.import_module("video-to-video-diffusion_amd.engine")
EF = importlib.import_module("video-to-video-diffusion_amd.engine_f32")
L = importlib.import_module("video-to-video-diffusion_amd.lib")

BATCHES = (1, 2, 4, 8, 13, 16, 25)
SCALES = ((1, 1), (2, 1), (16, 3))          # latent 48 x 24^2 (one 192^2 window) -> 48 x 48^2 -> 48 x 128^2
SHARD_DEPTHS = (3, 6, 8, 12, 14, 24, 26)     # depth-sharded views (halo_d = 1): 3-slice boundaries, interiors 6 / 12 / 24 (+2)
DESC_FIELDS = [f for f, _ in L.ConvDesc._fields_]


@pytest.fixture(autouse=True)
def _convt_as_forward_conv(monkeypatch):
    # the oracle's zero-insertion + Conv3d form of ConvTranspose3d (MIOpen's fp32 backward-data path is minutes per shape)
    monkeypatch.setattr(R, "CONVT_AS_CONV", True)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _old_key(sig):
    """The cache key as it was before the pack-layout id: the kernel family only (low 4 bits of the id)."""
    return (sig[0] & 0xF,) + tuple(sig[1:])


def _crossings(recs_a, recs_b):
    """Layers the family-only key merges although the library packs them into different images: (sig, pack layout) records
    of two programs, the layout read from ctsi_conv_plan_pack_layout itself (not from the key under test)."""
    by_old = {}
    for sig, lay in recs_a:
        by_old.setdefault(_old_key(sig), set()).add(lay)
    return sorted({(_old_key(sig), la, lay) for sig, lay in recs_b for la in by_old.get(_old_key(sig), ()) if la != lay})


class _ConvRecorder:
    """Records every conv plan the engine creates (descriptor, weight cin, streaming tail) while installed."""

    def __init__(self, lib, monkeypatch):
        self.convs, live = [], {}
        create, set_cin, set_tail = lib.conv_plan_create, lib.conv_plan_set_weight_cin, lib.conv_plan_set_stream_tail

        def rec_create(pp, pdesc):
            rc = create(pp, pdesc)
            d = pdesc._obj
            ent = {f: getattr(d, f) for f in DESC_FIELDS}
            ent.update(cin_w=None, tail=0)
            self.convs.append(ent)
            live[pp._obj.value] = ent
            return rc

        def rec_cin(plan, cin_w):
            live[plan.value]["cin_w"] = cin_w
            return set_cin(plan, cin_w)

        def rec_tail(plan, on):
            live[plan.value]["tail"] = on
            return set_tail(plan, on)

        monkeypatch.setattr(lib, "conv_plan_create", rec_create)
        monkeypatch.setattr(lib, "conv_plan_set_weight_cin", rec_cin)
        monkeypatch.setattr(lib, "conv_plan_set_stream_tail", rec_tail)


class _SigRecorder:
    """Records (cache key, ctsi_conv_plan_pack_layout) of every bf16 conv the engine emits while installed."""

    def __init__(self, monkeypatch):
        self.recs = []
        orig = E._pack_sig

        def rec(lib, plan, *a, **kw):
            s = orig(lib, plan, *a, **kw)
            self.recs.append((s, lib.conv_plan_pack_layout(plan)))
            return s

        monkeypatch.setattr(E, "_pack_sig", rec)

    def take(self):
        out, self.recs = self.recs, []
        return out


def _production_convs(pkg, lib, monkeypatch):
    """Every distinct conv the production networks emit, recorded at the 48 x 24^2 latent of one 192^2 window: the full-width
    U-Net (128 x (1,2,4,4)), the legacy 163 M U-Net and the production VAE encoder (8 thick slices) and decoder."""
    with monkeypatch.context() as mp:
        rec = _ConvRecorder(lib, mp)
        with torch.no_grad():
            torch.manual_seed(0)
            un = pkg.UNet3D(latent_dim=8).eval().to(DEV)
            z = torch.randn(1, 8, 48, 24, 24, device=DEV)
            un(z, torch.tensor([500], device=DEV), z)
            del un
            un = pkg.UNet3D(**LEGACY163_UNET).eval().to(DEV)
            z = torch.randn(1, 4, 48, 24, 24, device=DEV)
            un(z, torch.tensor([500], device=DEV), z)
            del un
            vae = pkg.VideoVAE(in_channels=1, latent_dim=8, base_channels=128, scaling_factor=1.0).eval().to(DEV)
            vae.encode(torch.rand(1, 1, 8, 192, 192, device=DEV) * 2 - 1)
            vae.decode(torch.randn(1, 8, 48, 24, 24, device=DEV))
            del vae
        torch.cuda.synchronize()
    _free()
    uniq = {}
    for c in rec.convs:
        uniq[tuple(sorted((k, v) for k, v in c.items() if k != "n"))] = c
    convs = list(uniq.values())
    kinds = {(c["transposed"], c["kd"], c["kh"], c["sh"]) for c in convs}
    assert {(0, 3, 3, 1), (0, 1, 1, 1), (0, 3, 4, 2), (1, 3, 4, 2)} <= kinds, kinds     # 3^3, 1^3, strided, ConvT
    assert any(c["cin_w"] == 1 for c in convs) and any(c["tail"] for c in convs) and any(c["cout"] <= 8 for c in convs)
    return convs


def _sweep_plans(convs):
    """(descriptor, cin_w, tail) of every plan the sweep packs."""
    out = []
    for c in convs:
        for num, den in SCALES:
            assert c["hi"] * num % den == 0 and c["wi"] * num % den == 0, c
            base = dict(c, hi=c["hi"] * num // den, wi=c["wi"] * num // den)
            for n in BATCHES:
                out.append(dict(base, n=n))
            if c["kd"] == 3 and c["pd"] == 1:
                for di in SHARD_DEPTHS:
                    out.append(dict(base, n=1, di=di, halo_d=1))
    return out


def _weight(c, cache):
    cin = c["cin_w"] if c["cin_w"] is not None else c["c1"] + c["c2"]
    shape = ((cin, c["cout"]) if c["transposed"] else (c["cout"], cin)) + (c["kd"], c["kh"], c["kw"])
    if shape not in cache:
        cache[shape] = _randn(shape, len(cache) + 1).to(DEV).contiguous()
    return cache[shape]


def _check_groups(groups, what):
    """groups: key -> list of (plan description, image).  Images under one key must be byte-identical."""
    bad = []
    for key, ents in groups.items():
        ref_desc, ref = ents[0]
        for desc, img in ents[1:]:
            if not torch.equal(img, ref):
                bad.append((key, ref_desc, desc, int((img != ref).sum())))
    for key, a, b, nd in bad[:8]:
        print(f"{what}: key {key}\n    {a}\n    {b}\n    pack different images ({nd} bytes differ)")
    assert not bad, f"{len(bad)} plan(s) share a {what} cache key with a plan that packs a different image (first: {bad[0]})"


def test_pack_layout_property_sweep(pkg, monkeypatch):
    lib = pkg.get_lib()
    convs = _production_convs(pkg, lib, monkeypatch)
    plans = _sweep_plans(convs)
    sptr = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    weights, groups, layouts = {}, {}, set()
    for c in plans:
        desc = L.ConvDesc(**{f: c[f] for f in DESC_FIELDS})
        plan = C.c_void_p()
        try:
            lib.conv_plan_create(C.byref(plan), C.byref(desc))
        except L.CtsiError:
            assert c["halo_d"], c          # (only a depth-sharded view the engine never builds may be refused)
            continue
        try:
            if c["cin_w"] is not None:
                lib.conv_plan_set_weight_cin(plan, c["cin_w"])
            if c["tail"]:
                lib.conv_plan_set_stream_tail(plan, c["tail"])
            sig = E._pack_sig(lib, plan, c["transposed"], (c["kd"], c["kh"], c["kw"]), (c["sh"], c["sw"]), c["c1"], c["c2"],
                              c["cout"], c["cin_w"])
            lay = lib.conv_plan_pack_layout(plan)
            layouts.add(lay)
            w = _weight(c, weights)
            img = torch.zeros(lib.conv_plan_weight_bytes(plan), dtype=torch.uint8, device=DEV)
            lib.conv_plan_pack_weights(plan, C.c_void_p(w.data_ptr()), C.c_void_p(img.data_ptr()), sptr)
            tag = dict(n=c["n"], di=c["di"], hi=c["hi"], wi=c["wi"], halo_d=c["halo_d"], layout=hex(lay))
            ents = groups.setdefault(sig, [])
            if not ents or not torch.equal(img, ents[0][1]):
                ents.append((tag, img))        # keep the first image of a key and every one that differs from it
        finally:
            lib.conv_plan_destroy(plan)
    torch.cuda.synchronize()
    print(f"bf16 sweep: {len(convs)} convs, {len(plans)} plans, {len(groups)} keys, layouts {sorted(hex(x) for x in layouts)}")
    fams = {x & 0xF for x in layouts}
    assert {1, 4, 5, 6, 7} <= fams, fams                                   # gather, k32, head, stream tail, stem all swept
    assert {x & 0x4F for x in layouts if x & 0xF == 4} >= {0x04, 0x44}     # both k32 image layouts met
    _check_groups(groups, "bf16")
    del groups
    _free()

    # the fp32 family (engine_f32): the same descriptors, keyed by engine_f32._f32_pack_sig
    groups = {}
    nf = 0
    for c in plans:
        if c["halo_d"] or c["tail"] or c["cin_w"] is not None:
            continue
        desc = L.ConvDesc(**{f: c[f] for f in DESC_FIELDS})
        if not lib.conv_f32_supported(C.byref(desc)):
            continue
        g = [C.c_int() for _ in range(6)]
        lib.conv_f32_geometry(C.byref(desc), *[C.byref(v) for v in g])
        wbytes = lib.conv_f32_weight_bytes(C.byref(desc))
        key = EF._f32_pack_sig(desc, g[5].value, wbytes)
        w = _weight(c, weights)
        img = torch.zeros(wbytes, dtype=torch.uint8, device=DEV)
        lib.conv_f32_pack_weights(C.byref(desc), C.c_void_p(w.data_ptr()), C.c_void_p(img.data_ptr()), sptr)
        nf += 1
        ents = groups.setdefault(key, [])
        if not ents or not torch.equal(img, ents[0][1]):
            ents.append((dict(n=c["n"], di=c["di"], hi=c["hi"], wi=c["wi"]), img))
    torch.cuda.synchronize()
    print(f"fp32 sweep: {nf} plans, {len(groups)} keys")
    assert nf > 100
    _check_groups(groups, "fp32")


def _unet_inputs(n, seed):
    x, c = _randn((n, 8, 48, 24, 24), seed), _randn((n, 8, 48, 24, 24), seed + 1)
    t = torch.randint(0, 1000, (n,), generator=torch.Generator().manual_seed(seed + 2))
    return x, t, c


def _live_keys(dev_index):
    gc.collect()
    return set(E._PACKED.get(dev_index, {}).keys())


@pytest.mark.parametrize("order", [(2, 13), (13, 2)], ids=["2-then-13", "13-then-2"])
def test_unet_output_independent_of_programs_built_before(pkg, monkeypatch, order):
    """Two batch sizes of one full-width U-Net whose 48 x 24^2 level-0 convs run on differently packed k32 tiles (n = 2:
    staged 384-voxel tiles, natural cout order; n = 13: direct-store 4x4x24 tiles, cout-permuted), in one process."""
    torch.manual_seed(0)
    un = pkg.UNet3D(latent_dim=8).eval().to(DEV)
    sd = {"unet." + k: v.detach() for k, v in un.state_dict().items()}
    dev_index = torch.device(DEV).index or 0
    before = _live_keys(dev_index)
    inputs = {n: _unet_inputs(n, 10 * n) for n in order}
    rec = _SigRecorder(monkeypatch)

    def run(n):
        x, t, c = inputs[n]
        with torch.no_grad():
            out = un(x.to(DEV), t.to(DEV), c.to(DEV))
        torch.cuda.synchronize()
        prog = next(p for k, p in un.__dict__["_ctsi_programs"].items() if k[0] == "unet" and k[2] == n)
        return out, dict(prog.pack_stats), rec.take()

    first, _, sig_a = run(order[0])
    second, stats_b, sig_b = run(order[1])
    cross = _crossings(sig_a, sig_b)
    print(f"order {order}: {len(cross)} conv key(s) cross image layouts, second program {stats_b}")
    assert cross, "no layer crosses k32 image layouts between the two batch sizes: the test would prove nothing"
    assert stats_b["shared"] > 0, "the second program found none of the first one's images: sharing was lost"
    # both against the fp32 oracle
    for n, out in ((order[0], first), (order[1], second)):
        x, t, c = inputs[n]
        with torch.no_grad():
            ref = R.unet_forward(sd, UNET_CFG, x.to(DEV), t.to(DEV), c.to(DEV), "unet.")
        e = rel_l2(out, ref)
        print(f"n = {n} ({'first' if n == order[0] else 'second'}): rel-L2 vs fp32 oracle {e:.3g}")
        assert e < NET_TOL, f"n = {n} (order {order}): rel-L2 {e:.3g} vs the fp32 oracle"
        del ref
    # the second batch size alone, on a fresh cache: bit-identical
    un.invalidate_engine_cache()
    _free()
    assert _live_keys(dev_index) <= before, "dropping the programs left packed images in the cache"
    alone, _, _ = run(order[1])
    assert torch.equal(alone, second), f"n = {order[1]} after n = {order[0]} differs from n = {order[1]} alone"
    un.invalidate_engine_cache()
    del un
    _free()


def test_stitching_after_generate_equals_a_fresh_cache(pkg, monkeypatch):
    """sample_with_stitching batching 13 windows of 48 x 192^2 (latent 48 x 24^2, n = 13) after generate() on one 192^2 patch
    (the same latent at n = 1) in one process: bit-identical to the same stitching on a fresh cache."""
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(FULL_CFG).eval().to(DEV)
    vol = (torch.rand((1, 1, 56, 192, 192), generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)  # 13 windows
    sampler = pkg.DDIMSampler(model.diffusion, model.unet)
    kw = dict(patch_size=(8, 192, 192), target_patch_size=(48, 192, 192), stride=(4, 96, 96), device=DEV, progress=False,
              window_batch=13)
    rec = _SigRecorder(monkeypatch)
    with torch.no_grad():
        torch.manual_seed(7)
        fresh = sampler.sample_with_stitching(vol, model.vae, 2, **kw)
        torch.cuda.synchronize()
        sig_st = rec.take()
        model.invalidate_engine_cache()
        _free()
        torch.manual_seed(8)
        patch = model.generate(vol[:, :, :8], "ddim", num_inference_steps=2, target_depth=48)
        torch.cuda.synchronize()
        sig_gen = rec.take()
        torch.manual_seed(7)
        after = sampler.sample_with_stitching(vol, model.vae, 2, **kw)
        torch.cuda.synchronize()
    cross = _crossings(sig_gen, sig_st)
    print(f"generate() (n = 1) vs stitching (n = 13): {len(cross)} conv key(s) cross image layouts")
    assert cross, "no layer crosses k32 image layouts between generate() and the stitching batch: the test would prove nothing"
    assert tuple(fresh.shape) == (1, 1, 336, 192, 192) and tuple(patch.shape) == (1, 1, 48, 192, 192)
    assert torch.isfinite(fresh).all()
    diff = float((after - fresh).abs().max())
    assert torch.equal(after, fresh), f"stitching after generate() differs from a fresh cache: max |d| {diff:.3g}"
    model.invalidate_engine_cache()
    del model
    _free()
