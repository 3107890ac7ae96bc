"""CPU: attention_mode='softmax' -- the restatement the GPU tests compare with (tests/attn_restatement.py), the mode's
validation and configuration, and the argument checks of the new C entry points."""
import ctypes as C
import importlib
import re

import pytest
import torch

from oracle import ref_ops as R
from tests import attn_restatement as AR
from tests.helpers import TINY_CFG, TINY_UNET, formula_input, formula_sd, load_formula, rel_l2, unet_cfg

L = importlib.import_module("video-to-video-diffusion_amd.lib")
E = importlib.import_module("video-to-video-diffusion_amd.engine")
F64 = torch.float64


def _qkv(d, hd, seed):
    g = torch.Generator().manual_seed(seed)
    q, k = (torch.randn((2, 3, d, hd), generator=g, dtype=F64) * 2.0 ** 0.5 for _ in range(2))
    v, da = (torch.randn((2, 3, d, hd), generator=g, dtype=F64) for _ in range(2))
    return q, k, v, da


@pytest.mark.parametrize("d,hd", [(4, 16), (17, 8), (48, 64), (72, 128)])
def test_backward_formulas_equal_autograd(d, hd):
    q, k, v, da = _qkv(d, hd, 7 + d)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    a, _ = AR.core_fwd64(qa, ka, va)
    a.backward(da)
    r = AR.core_bwd64(q, k, v, da)
    for name, ref in (("dq", qa.grad), ("dk", ka.grad), ("dv", va.grad)):
        assert float((r[name] - ref).abs().max()) <= 1e-13 * float(ref.abs().max()), name
    # peaked scores: far from what a kernel that ignored them would return
    if d > 1:
        assert rel_l2(AR.core_uniform64(v), a.detach()) > 0.5


def test_head_split_round_trip_and_layout():
    t = torch.arange(2 * 3 * 2 * 2 * 24, dtype=torch.float32).reshape(2, 3, 2, 2, 24)
    assert torch.equal(AR.merge_heads(AR.split_heads(t, 4)), t)
    q, k, v = AR.split_qkv(t, 2)
    assert tuple(q.shape) == (2, 2, 2, 2, 3, 4)
    # head 1 of k, depth 2, position (1, 0), channel 3 of the head: NDHWC channel c + 1 * hd + 3
    assert float(k[1, 1, 0, 1, 2, 3]) == float(t[1, 2, 1, 0, 8 + 4 + 3])


def test_restated_unet_differs_widely_from_the_reference_einsum():
    import models
    un = models.UNet3D(**TINY_UNET)
    sd = load_formula(un, 8)
    x, c, t = formula_input((2, 8, 4, 8, 8), 10), formula_input((2, 8, 4, 8, 8), 11), torch.tensor([500, 37])
    ref = R.unet_forward(sd, unet_cfg(TINY_UNET), x, t, c)
    out = AR.unet_forward(sd, unet_cfg(TINY_UNET), x, t, c)
    assert rel_l2(out, ref) > 0.5
    assert R.temporal_attention is not AR.temporal_attention_softmax       # the swap ended with the call
    assert torch.equal(R.unet_forward(sd, unet_cfg(TINY_UNET), x, t, c), ref)


def test_constant_values_along_depth_pass_through():
    """With V constant along depth every softmax row averages equal rows: the block is x + proj_out(v), whatever q and k."""
    from models.unet3d import TemporalAttention
    ch, heads = 64, 4
    at = TemporalAttention(ch, heads)
    sd = {"a." + k: v for k, v in formula_sd(at, 4).items()}
    sd["a.qkv.weight"][2 * ch:] = 0.0                    # v = its bias: constant along depth (and everywhere)
    x = formula_input((1, ch, 5, 3, 2), 5)
    out = AR.temporal_attention_softmax(sd, "a", x, heads)
    v = sd["a.qkv.bias"][2 * ch:].view(1, ch, 1, 1, 1).expand(1, ch, 5, 3, 2)
    assert rel_l2(out, x + R.conv3d(sd, "a.proj_out", v)) < 1e-5


def test_unknown_mode_is_a_value_error(pkg):
    assert [E.check_attention_mode(m) for m in ("fast", "exact", "softmax")] == ["fast", "exact", "softmax"]
    for bad in ("sofmax", "", None, "Softmax"):
        with pytest.raises(ValueError, match="attention_mode"):
            E.check_attention_mode(bad)
    un = pkg.UNet3D(**TINY_UNET)
    x = torch.zeros(1, 8, 2, 4, 4)
    un.attention_mode = "softmax"
    with pytest.raises(pkg.CtsiError):                      # a valid mode: still no CPU path
        un(x, torch.tensor([3]), x)
    un.attention_mode = "flash"
    with pytest.raises(ValueError, match="attention_mode"):
        un(x, torch.tensor([3]), x)
    with pytest.raises(ValueError, match="attention_mode"):
        pkg.DDIMSampler(pkg.GaussianDiffusion(), un).sample(tuple(x.shape), x, 2, "cpu", progress=False)
    with pytest.raises(ValueError, match="attention_mode"):
        pkg.GaussianDiffusion().training_loss(un, x, x)


def test_config_key(pkg):
    assert pkg.VideoToVideoDiffusion(TINY_CFG).unet.attention_mode == "fast"
    m = pkg.VideoToVideoDiffusion(dict(TINY_CFG, unet_attention_mode="softmax"))
    assert m.unet.attention_mode == "softmax"
    # same modules, same state-dict layout: a checkpoint loads in either mode
    ref = pkg.VideoToVideoDiffusion(TINY_CFG).state_dict()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.items()}
    m.load_state_dict(ref, strict=True)
    with pytest.raises(ValueError, match="attention_mode"):
        pkg.VideoToVideoDiffusion(dict(TINY_CFG, unet_attention_mode="true"))
    # like every U-Net key it is read from the top level only
    assert pkg.VideoToVideoDiffusion(dict(TINY_CFG, model=dict(unet_attention_mode="softmax"))).unet.attention_mode == "fast"


def test_entry_points_exist_and_reject_bad_arguments():
    if not L.LIB_PATH.exists():
        L.build()
    lib = L.get_lib()
    text = re.sub(r"/\*.*?\*/", "", L.HEADER_PATH.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(ctsi_[a-z0-9_]+)\s*\(", text))
    dll = C.CDLL(str(L.LIB_PATH))
    for s, nargs in (("ctsi_attn_core", 9), ("ctsi_attn_core_bwd", 10)):
        assert s in declared, f"{s} not declared in include/ctsi.h"
        assert hasattr(dll, s), f"{s} not exported"
        assert s in L.SIGNATURES and len(L.SIGNATURES[s][1]) == nargs
        assert hasattr(lib, s[len("ctsi_"):])
    one = C.c_void_p(16)     # never dereferenced: argument checks run before any launch
    with pytest.raises(L.CtsiError, match="null argument"):
        lib.attn_core(None, one, 1, 64, 4, 2, 2, 4, None)
    with pytest.raises(L.CtsiError, match="null argument"):
        lib.attn_core(one, None, 1, 64, 4, 2, 2, 4, None)
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        with pytest.raises(L.CtsiError, match="null argument"):
            lib.attn_core_bwd(*args, 1, 64, 4, 2, 2, 4, None)
    with pytest.raises(L.CtsiError, match="c=66.*heads=4"):
        lib.attn_core(one, one, 1, 66, 4, 2, 2, 4, None)
    with pytest.raises(L.CtsiError, match="c=66.*heads=4"):
        lib.attn_core_bwd(one, one, one, 1, 66, 4, 2, 2, 4, None)
    with pytest.raises(L.CtsiError, match="head dimension 12"):           # not a multiple of 8
        lib.attn_core(one, one, 1, 48, 4, 2, 2, 4, None)
    with pytest.raises(L.CtsiError, match="head dimension 256"):          # above the limit
        lib.attn_core_bwd(one, one, one, 1, 1024, 4, 2, 2, 4, None)
    with pytest.raises(L.CtsiError, match="depth 4096"):                  # more keys than one item's LDS image holds
        lib.attn_core(one, one, 1, 512, 4096, 1, 1, 4, None)
    with pytest.raises(L.CtsiError, match="bad shape"):
        lib.attn_core(one, one, 1, 64, 0, 2, 2, 4, None)
