"""CPU: the ResBlock options (UNet3D(use_scale_shift_norm=, dropout=)) where no GPU is needed -- the Philox generator through its
host entry point, the keep rule against a numpy restatement written here, module construction and state dicts, config keys and
their errors, and the float64 restatement's backward formulas against autograd."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

from tests import resblock_restatement as RR
from tests.helpers import TINY_CFG, TINY_UNET

L = importlib.import_module("video-to-video-diffusion_amd.lib")
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


@pytest.fixture(scope="module")
def lib():
    if not L.LIB_PATH.exists():
        L.build()
    return L.get_lib()


# ---- numpy restatement of the generator and of the chunk / lane rule ------------------------------------------------------
def philox_np(ctr, key):
    """Philox4x32-10 on arrays of counters: ctr (..., 4), key (..., 2) uint32 -> (..., 4) uint32."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0 = np.asarray(key[..., 0], dtype=np.uint64)
    k1 = np.asarray(key[..., 1], dtype=np.uint64)
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0 = (k0 + np.uint64(W0)) & mask
        k1 = (k1 + np.uint64(W1)) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def keep_mask_np(seed: int, layer_id: int, thr: int, count: int) -> np.ndarray:
    """Keep bytes of the first `count` elements of a layer's logical NDHWC tensor: one call per 8 elements, counter
    (lo32(g), hi32(g), layer_id, 0), key (seed_lo, seed_hi); element j of chunk g takes lane (out[j >> 1] >> 16 (j & 1)) & 0xffff
    and is kept iff lane >= thr."""
    chunks = (count + 7) // 8
    g = np.arange(chunks, dtype=np.uint64)
    ctr = np.stack([g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), np.full(chunks, layer_id, np.uint64),
                    np.zeros(chunks, np.uint64)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64), (chunks, 2))
    out = philox_np(ctr, key)
    lanes = np.stack([(out[:, j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xFFFF) for j in range(8)], axis=1)
    return (lanes >= thr).astype(np.uint8).reshape(-1)[:count]


def _host_philox(lib, ctr, key):
    c = np.array(ctr, dtype=np.uint32)
    k = np.array(key, dtype=np.uint32)
    o = np.zeros(4, dtype=np.uint32)
    lib.philox4x32_10_host(c.ctypes.data, k.ctypes.data, o.ctypes.data)
    return " ".join("%08x" % v for v in o)


KAT = [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(lib, ctr, key, want):
    """Random123's known-answer vectors, through the library's host entry point and through the numpy restatement."""
    assert _host_philox(lib, ctr, key) == want
    got = philox_np(np.array([ctr], dtype=np.uint64), np.array([key], dtype=np.uint64))[0]
    assert " ".join("%08x" % v for v in got) == want


def test_host_mask_equals_the_numpy_restatement(lib):
    for seed, layer, thr, count in [(0, 0, 1, 64), (0x123456789ABCDEF0, 7, int(0.25 * 65536), 4099), (2 ** 64 - 1, 3, 65535, 800)]:
        out = np.zeros(count, dtype=np.uint8)
        lib.dropout_mask_host(C.c_ulonglong(seed), layer, thr, count, out.ctypes.data)
        assert np.array_equal(out, keep_mask_np(seed, layer, thr, count)), (seed, layer, thr)


def test_keep_fraction_and_layer_independence():
    """Keep fraction within 5 sigma of q = 1 - thr / 65536; two layer ids agree on a fraction within 5 sigma of
    q^2 + (1 - q)^2 (what independent masks give)."""
    p, n = 0.1, 32000
    thr = int(p * 65536)
    q = 1.0 - thr / 65536.0
    a, b = keep_mask_np(20240607, 0, thr, n), keep_mask_np(20240607, 5, thr, n)
    bound = 5 * math.sqrt(q * (1 - q) / n)
    print(f"keep fraction {a.mean():.5f} / {b.mean():.5f} against {q:.5f}, bound {bound:.4f}")
    assert abs(a.mean() - q) <= bound and abs(b.mean() - q) <= bound
    r = q * q + (1 - q) * (1 - q)
    agree = float((a == b).mean())
    print(f"two layers agree on {agree:.5f} against {r:.5f}, bound {5 * math.sqrt(r * (1 - r) / n):.4f}")
    assert abs(agree - r) <= 5 * math.sqrt(r * (1 - r) / n)
    assert not np.array_equal(a, keep_mask_np(20240608, 0, thr, n))          # another seed, another mask
    assert np.array_equal(a[:1000], keep_mask_np(20240607, 0, thr, 1000))     # a prefix does not depend on the count


def test_threshold_and_scale():
    U = importlib.import_module("video-to-video-diffusion_amd.unet3d")
    assert U.dropout_threshold(0.0) == 0 and U.dropout_threshold(1e-6) == 0        # thr == 0: the default kernels
    assert U.dropout_threshold(0.1) == 6553 and U.dropout_threshold(0.25) == 16384 and U.dropout_threshold(0.5) == 32768
    T = importlib.import_module("video-to-video-diffusion_amd.train_engine")
    st = T.DropoutState(torch.zeros(1, dtype=torch.int64))
    st.set(0.2, -1)
    assert st.thr == 13107 and st.inv == 65536.0 / (65536.0 - 13107) and st.seed_value == 2 ** 64 - 1


# ---- module and config --------------------------------------------------------------------------------------------------
def test_state_dict_shapes_in_both_modes(pkg):
    a, b = pkg.UNet3D(**TINY_UNET), pkg.UNet3D(**TINY_UNET, use_scale_shift_norm=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    differing = [k for k in sa if sa[k].shape != sb[k].shape]
    blocks = [n for n, m in b.named_modules() if type(m).__name__ == "ResBlock3D"]
    assert sorted(differing) == sorted(f"{n}.time_mlp.1.{w}" for n in blocks for w in ("weight", "bias"))
    for k in differing:
        assert sb[k].shape[0] == 2 * sa[k].shape[0] and sb[k].shape[1:] == sa[k].shape[1:]
    assert a.use_scale_shift_norm is False and b.use_scale_shift_norm is True and a.dropout == 0.0
    assert all(m.scale_shift for m in b.modules() if type(m).__name__ == "ResBlock3D")
    with pytest.raises(RuntimeError):
        b.load_state_dict(sa, strict=True)


def test_default_construction_is_unchanged(pkg):
    """The default arguments consume the same random numbers in the same order: the weights equal those of a construction
    that spells the defaults out, the generator ends in the same state, and a default state dict loads strictly.  (The same
    seed gives the module tree of the parent commit: nothing before or between the layers draws.)"""
    torch.manual_seed(5)
    a = pkg.UNet3D(**TINY_UNET)
    after_a = torch.random.get_rng_state()
    torch.manual_seed(5)
    b = pkg.UNet3D(**TINY_UNET, use_scale_shift_norm=False, dropout=0.0)
    assert torch.equal(after_a, torch.random.get_rng_state())
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    # the draw order of the reference's tree: a ResBlock's own Linear is (time_dim -> C) and is drawn between conv1 and conv2
    torch.manual_seed(5)
    c = pkg.UNet3D(**TINY_UNET, use_scale_shift_norm=True)
    sc = c.state_dict()
    first = next(k for k in sa if k.endswith("time_mlp.1.weight") and "time_embed" not in k)
    before = list(sa)[:list(sa).index(first)]
    assert all(torch.equal(sa[k], sc[k]) for k in before)            # identical up to the first widened projection
    pkg.UNet3D(**TINY_UNET).load_state_dict(sa, strict=True)
    c2 = pkg.UNet3D(**TINY_UNET, use_scale_shift_norm=True)
    c2.load_state_dict(sc, strict=True)


def test_dropout_attribute_validation(pkg):
    for bad in (-0.1, 1.0, 1.5, "0.1", None, True, float("nan")):
        with pytest.raises(ValueError):
            pkg.UNet3D(**TINY_UNET, dropout=bad)
    u = pkg.UNet3D(**TINY_UNET, dropout=0.3)
    assert u.dropout == 0.3
    u.dropout = 0.0          # a plain attribute


def test_config_keys(pkg):
    m = pkg.VideoToVideoDiffusion(dict(TINY_CFG))
    assert m.unet.use_scale_shift_norm is False and m.unet.dropout == 0.0
    m = pkg.VideoToVideoDiffusion(dict(TINY_CFG, unet_use_scale_shift_norm=True, unet_dropout=0.1))
    assert m.unet.use_scale_shift_norm is True and m.unet.dropout == 0.1
    c = m.unet.down_blocks[0][0][0].conv1.conv.out_channels
    assert m.unet.down_blocks[0][0][0].time_mlp[1].out_features == 2 * c
    for bad in ({"unet_use_scale_shift_norm": "false"}, {"unet_use_scale_shift_norm": 1}, {"unet_dropout": 1.0},
                {"unet_dropout": -0.5}, {"unet_dropout": "0.1"}):
        with pytest.raises(ValueError):
            pkg.VideoToVideoDiffusion(dict(TINY_CFG, **bad))


def test_scale_shift_refuses_depth_sharding(pkg):
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    E.check_resblock_options_unsharded(pkg.UNet3D(**TINY_UNET), True)
    E.check_resblock_options_unsharded(pkg.UNet3D(**TINY_UNET, use_scale_shift_norm=True), False)
    with pytest.raises(pkg.CtsiError, match="use_scale_shift_norm"):
        E.check_resblock_options_unsharded(pkg.UNet3D(**TINY_UNET, use_scale_shift_norm=True), True)


def test_training_on_host_tensors_still_raises_before_drawing_a_seed(pkg):
    """dropout > 0 changes nothing about where training runs: host tensors are a CtsiError, and a bad `dropout` attribute a
    ValueError at the forward that reads it."""
    u = pkg.UNet3D(**TINY_UNET, dropout=0.2).train()
    g = pkg.GaussianDiffusion()
    z = torch.zeros(1, 8, 2, 4, 4)
    t, noise = torch.zeros(1, dtype=torch.long), torch.zeros_like(z)
    state = torch.random.get_rng_state()
    with pytest.raises(pkg.CtsiError):
        g.training_loss(u, z, z, t=t, noise=noise)
    assert torch.equal(state, torch.random.get_rng_state())           # no seed was drawn
    u.dropout = 1.0
    with pytest.raises(ValueError):
        g.training_loss(u, z, z)


def test_new_entry_points_validate_arguments(lib):
    """Host-side argument checks (no launch): the option pass is the ResBlock's middle pass only, dropout needs the seed buffer."""
    one = C.c_void_p(16)
    base = [one, one, one, one, one, 1, 32, 2, 4, 4, 2, 8, C.c_float(1e-5)]
    tail_ok = [1, one, 64, None, None, 0]
    assert lib.raw["ctsi_gn_apply_mod"](*base, 0, one, 64, None, None, 0, 1, 0, C.c_float(1.0), None, 0, None) != 0   # no SiLU
    assert lib.raw["ctsi_gn_apply_mod"](*base, 1, None, 64, None, None, 0, 1, 0, C.c_float(1.0), None, 0, None) != 0  # no time row
    assert lib.raw["ctsi_gn_apply_mod"](*base, 1, one, 64, None, one, 0, 1, 0, C.c_float(1.0), None, 0, None) != 0    # residual
    assert lib.raw["ctsi_gn_apply_mod"](*base, 1, one, 32, None, None, 0, 1, 0, C.c_float(1.0), None, 0, None) != 0   # 2c row
    assert lib.raw["ctsi_gn_apply_mod"](*base, *tail_ok, 1, 100, C.c_float(1.0), None, 0, None) != 0                   # no seed
    assert lib.raw["ctsi_gn_apply_mod"](*base, *tail_ok, 1, 65536, C.c_float(1.0), one, 0, None) != 0                  # threshold
    assert b"seed" in lib.last_error() or b"p_thr16" in lib.last_error()
    assert lib.raw["ctsi_gn_apply_mod_f32"](*base, 1, one, 64, None, None, 1, 1, None) != 0                            # outer SiLU
    assert lib.gn_bwd_mod_workspace_floats(2, 32, 3, 5, 7, 8) >= 2 * 4 * 32 + 2 * 8 * 2 + 2 * 4 * 32
    assert lib.raw["ctsi_dropout_mask"](None, 0, 1, 8, one, None) != 0


# ---- the restatement's backward formulas ------------------------------------------------------------------------------------
@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("drop", [False, True])
def test_restated_backward_equals_autograd(film, drop):
    g = torch.Generator().manual_seed(3)
    n, c, d, h, w, groups = 2, 16, 2, 3, 5, 4
    x = torch.randn((n, d, h, w, c), generator=g, dtype=torch.float64)
    dy = torch.randn((n, d, h, w, c), generator=g, dtype=torch.float64)
    gamma = (1 + 0.3 * torch.randn(c, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = (0.3 * torch.randn(c, generator=g, dtype=torch.float64)).requires_grad_(True)
    row = (0.5 * torch.randn((n, 2 * c if film else c), generator=g, dtype=torch.float64)).requires_grad_(True)
    keep = (torch.rand((n, d, h, w, c), generator=g) > 0.25).double() if drop else None
    inv = 4.0 / 3.0 if drop else 1.0
    eps = 1e-5
    xr = x.clone().requires_grad_(True)
    # autograd through GroupNorm proper (the statistics are functions of x)
    xn = torch.nn.functional.group_norm(xr.permute(0, 4, 1, 2, 3), groups, None, None, eps).permute(0, 2, 3, 4, 1)
    hh = xn * gamma + beta
    r = row[:, None, None, None, :]
    y = RR._silu(hh * (1 + r[..., :c]) + r[..., c:]) if film else RR._silu(hh) + r
    if drop:
        y = y * keep * inv
    (y * dy).sum().backward()
    sums = RR.group_sums(x, groups)
    assert torch.allclose(RR.pass_fwd64(x, sums, gamma.detach(), beta.detach(), row.detach(), groups, eps, film, keep, inv),
                          y.detach(), rtol=1e-10, atol=1e-12)
    ref = RR.pass_bwd64(x, dy, sums, gamma.detach(), beta.detach(), row.detach(), groups, eps, film, keep, inv)
    for name, want in (("dx", xr.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad), ("drow", row.grad),
                       ("dxsum", xr.grad.sum((0, 1, 2, 3)))):
        assert torch.allclose(ref[name], want, rtol=1e-8, atol=1e-10), name


# ---- which launches a block gets ----------------------------------------------------------------------------------------------
def test_dropout_zero_and_threshold_zero_select_the_default_path(pkg):
    """`dropout_active` decides whether a training forward builds the dropout program: off at 0, at a probability whose
    threshold floor(p * 65536) is 0, and in eval mode."""
    N = importlib.import_module("video-to-video-diffusion_amd.norm_mod")
    u = pkg.UNet3D(**TINY_UNET).train()
    assert not N.dropout_active(u)
    u.dropout = 1e-6                       # thr == 0
    assert not N.dropout_active(u)
    u.dropout = 0.2
    assert N.dropout_active(u)
    assert not N.dropout_active(u.eval())
    u.dropout = 1.0
    with pytest.raises(ValueError):
        N.dropout_active(u)


class _Recorder:
    """Stands in for a train program: records what TrainProgram.t_gn hands to gn_apply and which backward it would emit."""

    def __init__(self):
        self.calls, self.tape, self.tbias, self.total_out = [], [], torch.zeros(1, 4), 4
        self.lib, self.ctx = None, type("Ctx", (), {"sptr": None})()

    def gn_apply(self, x, slot, gn, **kw):
        self.calls.append(kw)
        return type("Out", (), {"grad": None})()

    def dev_f32(self, fn):
        return fn()


@pytest.mark.parametrize("film,drop,mod", [(False, None, False), (True, None, True), (False, ("state", 3), True)])
def test_t_gn_routes_to_the_option_launches_only_when_asked(film, drop, mod):
    """Without scale-shift and without dropout, t_gn calls gn_apply exactly as before (no `film` / `drop` keyword reaches it, so
    ctsi_gn_apply and ctsi_gn_bwd are emitted); with either, both keywords travel."""
    T = importlib.import_module("video-to-video-diffusion_amd.train_engine")
    rec = _Recorder()
    gn = torch.nn.GroupNorm(2, 4)
    T.TrainProgram.t_gn(rec, object(), 0, gn, silu_pre=True, tb_off=0, film=film, drop=drop)
    kw = rec.calls[0]
    assert ("film" in kw) == mod and ("drop" in kw) == mod
    if mod:
        assert kw["film"] == film and kw["drop"] == drop
    assert len(rec.tape) == 1
