"""GPU: SpatialAttention -- softmax(Q K^T / sqrt(hd)) V over the h * w positions of each (sample, depth slice, head)
(csrc/attention_plane.hip) from the kernel up to sampling and training, against tests/spatial_attn_restatement.py.

Core kernels: the criterion of tests/test_gpu_attn_softmax.py -- float64 from the kernel's own bf16 operands, `cmp_bf16` of
tests/train_audit.py (one bf16 ulp + its floor, rel-L2 4e-3 against bf16(ref)) plus one `extra` term per intermediate rounding
the source performs (half a bf16 ulp of x is at most 2^-8 |x|):

  forward   P is rounded to bf16 for the P V MFMA (the row sum is taken from the unrounded values):
                                                                     |d A[i][c]|  <= 2^-8 sum_j P[i][j] |V[j][c]|
  backward  P is rounded the same way for dV = P^T dA:               |d dV[j][c]| <= 2^-8 sum_i P[i][j] |dA[i][c]|
            dS is rounded to bf16 for dQ = dS K / sqrt(hd) and dK:   |d dQ[i][c]| <= 2^-8 sum_j |dS[i][j]| |K[j][c]| / sqrt(hd)
                                                                     |d dK[j][c]| <= 2^-8 sum_i |dS[i][j]| |Q[i][c]| / sqrt(hd)
            delta = rowsum(dA o A) is taken from the STORED bf16 A:  |d delta[i]| <= 2^-8 sum_c |dA[i][c]| |A[i][c]|, and
            dS = P o (dP - delta) carries it:                        |d dQ[i][c]| += sum_j P[i][j] |d delta[i]| |K[j][c]| / sqrt(hd)
                                                                     |d dK[j][c]| += sum_i P[i][j] |d delta[i]| |Q[i][c]| / sqrt(hd)
  Everything else is fp32 (scores, max, sum, exp2, lse, delta's sum, accumulation of exact bf16 products): ~1e-6 relative, under
  the floor.

lse (fp32, ln sum_j exp(s_ij)) against float64, u = 2^-24, first order, every term an upper bound:
  scores      hd exact bf16 products accumulated in fp32: (hd + 1) u max_j sum_c |q_ic k_jc| / sqrt(hd)   (lse is 1-Lipschitz in
              the sup norm of the scores)
  scaling     the rounded constant log2(e) / sqrt(hd), the product, the subtraction of the max (|s' - m| <= 2 max |s'|):
              4 u max_j |s_ij|
  exp / sum   v_exp_f32 (1 ulp = 2 u), N - 1 additions, per tile one rescale factor and its product (3 u):
              (N + 3 tiles + 2) u relative on the sum = absolute on its logarithm
  log / out   v_log_f32 (1 ulp), m + log2 l, the rounded constant ln 2 and its product: 6 u (|lse_i| + max_j |s_ij|)
so  |d lse_i| <= u [ (hd + 1) max_j sum_c |q_ic k_jc| / sqrt(hd) + 10 max_j |s_ij| + N + 3 ceil(N / 64) + 2 + 6 |lse_i| ].

Inputs have peaked scores (q, k ~ N(0, 2): scaled scores of std 2), and every case with N > 1 asserts that its float64 reference
is more than 0.5 rel-L2 away from uniform attention: a kernel that averaged V cannot pass.
"""
import importlib
import json
import os

import pytest
import torch

from oracle import ref_ops as R
from tests import attn_restatement as AR
from tests import poison as PZ
from tests import spatial_attn_restatement as SR
from tests.helpers import (MID_UNET, TINY_CFG, TINY_UNET, formula_input, formula_noise, formula_sd, load_formula, rel_l2,
                           unet_cfg)
from tests.train_audit import cmp_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
E = importlib.import_module("video-to-video-diffusion_amd.engine")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
SA = importlib.import_module("video-to-video-diffusion_amd.spatial_attention")
U = importlib.import_module("video-to-video-diffusion_amd.unet3d")
NET_TOL = 3e-2          # tests/test_gpu_network.py: the bf16 engine against the fp32 oracle
NAN, BIG = 0xFF, 0x7F
REL_HALF_ULP = 2.0 ** -8        # half a bf16 ulp of x is at most this much of |x|
U24 = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spatial_attn_default_launches.json")

# (n, C, heads, d, h, w): the smallest shapes at which each mechanism can fail
CORE_CASES = [
    (1, 32, 4, 1, 3, 3),          # hd 8, N = 9: below one key tile and one query block
    (2, 64, 4, 3, 1, 1),          # N = 1; several slices and samples
    (1, 64, 4, 2, 8, 8),          # hd 16, N = 64: exactly one key tile
    (1, 128, 4, 2, 5, 13),        # hd 32, N = 65: one key past a tile
    (1, 256, 4, 1, 13, 11),       # hd 64, N = 143: ragged tail in both keys and queries over several tiles
    (1, 512, 4, 1, 16, 16),       # hd 128, N = 256: exact multiples
    (1, 256, 4, 2, 24, 24),       # N = 576, the 192^2 level-1 plane: many tiles of online rescaling
    (2, 64, 2, 2, 6, 6),          # two heads, hd 32; the 6 x 6 training level
]
CORE_IDS = ["n%d_c%d_h%d_d%d_%dx%d" % c for c in CORE_CASES]
N143 = (1, 256, 4, 1, 13, 11)


@pytest.fixture(scope="module")
def G():
    from tests import gpu_utils
    return gpu_utils


def _operands(case):
    n, c, heads, d, h, w = case
    g = torch.Generator(device="cpu").manual_seed(2000 + h * w * 7 + c)
    qkv = torch.randn((n, d, h, w, 3 * c), generator=g)
    qkv[..., :2 * c] *= 2.0 ** 0.5       # q, k ~ N(0, 2): the scaled scores have std 2
    da = torch.randn((n, d, h, w, c), generator=g)
    return qkv.to(DEV, torch.bfloat16).contiguous(), da.to(DEV, torch.bfloat16).contiguous()


def _run_fwd(G, qkv, heads, with_lse=True):
    n, d, h, w, c3 = qkv.shape
    ctx = G.ctx()
    out = torch.full((n, d, h, w, c3 // 3), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((n, d, heads, h * w), float("nan"), dtype=torch.float32, device=DEV) if with_lse else None
    with ctx.scope():
        ctx.lib.attn_plane(G._ptr(qkv), G._ptr(out), None if lse is None else G._ptr(lse), n, c3 // 3, d, h, w, heads, ctx.sptr)
    torch.cuda.synchronize()
    return out, lse


def _run_bwd(G, qkv, a, da, lse, heads):
    n, d, h, w, c3 = qkv.shape
    ctx = G.ctx()
    out = torch.full((n, d, h, w, c3), float("nan"), dtype=torch.bfloat16, device=DEV)
    with ctx.scope():
        ctx.lib.attn_plane_bwd(G._ptr(qkv), G._ptr(a), G._ptr(da), G._ptr(lse), G._ptr(out), n, c3 // 3, d, h, w, heads,
                               ctx.sptr)
    torch.cuda.synchronize()
    return out


def _report(tag, res):
    print(f"{tag}: ulps {res['ulps']:.3f} rel_l2 {res['rel_l2']:.3e} max_rel {res['max_rel']:.3e} ok {res['ok']}")


def _core_ref(qkv, da, heads):
    """float64 forward and backward from the bf16 operands, with the rounding terms of the module docstring."""
    q, k, v = (t.to(F64) for t in SR.split_qkv_plane(qkv, heads))
    g = SR.split_plane(da, heads).to(F64)
    r = AR.core_bwd64(q, k, v, g)
    a, p = AR.core_fwd64(q, k, v)
    nq, hd = q.shape[-2], q.shape[-1]
    sc = hd ** -0.5
    s = q @ k.transpose(-1, -2) * sc
    lse = torch.logsumexp(s, dim=-1)
    sabs = (q.abs() @ k.abs().transpose(-1, -2) * sc).amax(-1)
    lse_tol = U24 * ((hd + 1) * sabs + 10 * s.abs().amax(-1) + nq + 3 * ((nq + 63) // 64) + 2 + 6 * lse.abs())
    ddl = REL_HALF_ULP * (g.abs() * a.abs()).sum(-1, keepdim=True)           # |d delta[i]|
    ex = dict(a=REL_HALF_ULP * (p @ v.abs()),
              dv=REL_HALF_ULP * (p.transpose(-1, -2) @ g.abs()),
              dq=REL_HALF_ULP * sc * (r["ds"].abs() @ k.abs()) + sc * ((p * ddl) @ k.abs()),
              dk=REL_HALF_ULP * sc * (r["ds"].abs().transpose(-1, -2) @ q.abs()) + sc * ((p * ddl).transpose(-1, -2) @ q.abs()))
    return dict(a=a, uni=AR.core_uniform64(v), dq=r["dq"], dk=r["dk"], dv=r["dv"], ex=ex, lse=lse, lse_tol=lse_tol)


@pytest.fixture(scope="module")
def core_refs():
    """Per case, computed once and left unchanged: operands and the float64 reference (on the device: N = 576 is 2.6 M scores
    per item in float64)."""
    cache = {}

    def get(case):
        if case not in cache:
            qkv, da = _operands(case)
            cache[case] = dict(qkv=qkv, da=da, **_core_ref(qkv, da, case[2]))
        return cache[case]

    return get


@pytest.mark.parametrize("case", CORE_CASES, ids=CORE_IDS)
def test_core_forward(G, core_refs, case):
    heads = case[2]
    ref = core_refs(case)
    if case[4] * case[5] > 1:   # (one key: softmax and a mean are the same function)
        assert rel_l2(ref["uni"], ref["a"]) > 0.5, "the reference must be far from uniform attention"
    out, lse = _run_fwd(G, ref["qkv"], heads)
    res = cmp_bf16(SR.split_plane(out, heads), ref["a"], ref["ex"]["a"])
    _report("fwd %s" % (case,), res)
    assert res["ok"], res
    lerr = ((lse.to(F64) - ref["lse"]).abs() / ref["lse_tol"]).max().item()
    print(f"lse {case}: max |err| / bound {lerr:.3f}")
    assert lerr <= 1.0, lerr
    out2, lse2 = _run_fwd(G, ref["qkv"], heads)
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16)) and torch.equal(lse2.view(torch.int32), lse.view(torch.int32))
    out3, _ = _run_fwd(G, ref["qkv"], heads, with_lse=False)       # inference passes no lse
    assert torch.equal(out3.view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("case", CORE_CASES, ids=CORE_IDS)
def test_core_backward(G, core_refs, case):
    heads = case[2]
    ref = core_refs(case)
    a, lse = _run_fwd(G, ref["qkv"], heads)
    out = _run_bwd(G, ref["qkv"], a, ref["da"], lse, heads)
    dq, dk, dv = SR.split_qkv_plane(out, heads)
    bad = []
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        res = cmp_bf16(got, ref[name], ref["ex"][name])
        _report("bwd %s %s" % (name, case), res)
        if not ref[name].any():
            # N = 1: P = 1 and dS = P o (dP - delta) = 0 exactly, so dQ = dK = 0 and a rel-L2 has no denominator; the kernel's
            # delta (from A) and dP (an MFMA) are two fp32 sums of the same products in different orders, so its dS is ~1e-7, not
            # 0.  The elementwise bound (the derived terms alone: one ulp of 0 and the floor of rms 0 are 0) is the criterion.
            assert case[4] * case[5] == 1 and name in ("dq", "dk")
            res["ok"] = res["ulps"] <= 1.0
        if not res["ok"]:
            bad.append((name, res))
    assert not bad, bad
    assert torch.equal(_run_bwd(G, ref["qkv"], a, ref["da"], lse, heads).view(torch.int16), out.view(torch.int16))


def _late_maximum_operands():
    """N = 143, hd 64, built: key j is s times the +-1 expansion of j's 8 bits, repeated 8 times (k_j . k_j' = 8 s^2 (8 - 2
    hamming(j, j'))), query i is key pi(i), pi(i) = (i + 64) mod 143.  Query i's score is 8 s^2 at pi(i) and at least 2 s^2 = 32
    lower everywhere else: A[i] = V[pi(i)] to e^-32.  79 of the 143 queries have their key in a later tile than their own, 15 of
    them in the last, ragged one: every such row builds its accumulator under a smaller maximum first."""
    n, c, heads, d, h, w = N143
    nq, hd, s = h * w, c // heads, 4.0
    j = torch.arange(nq)
    bits = ((j[:, None] >> torch.arange(8)[None, :]) & 1).float() * 2 - 1        # (N, 8)
    keys = s * bits.repeat(1, hd // 8)                                           # (N, hd)
    pi = (j + 64) % nq
    g = torch.Generator().manual_seed(77)
    v = torch.randn((nq, heads, hd), generator=g)
    qkv = torch.cat([keys[pi][:, None, :].expand(nq, heads, hd).reshape(nq, c),
                     keys[:, None, :].expand(nq, heads, hd).reshape(nq, c), v.reshape(nq, c)], dim=1)
    return qkv.reshape(n, d, h, w, 3 * c).to(DEV, torch.bfloat16).contiguous(), pi


def test_core_forward_late_maximum(G):
    heads = N143[2]
    qkv, pi = _late_maximum_operands()
    q, k, v = (t.to(F64) for t in SR.split_qkv_plane(qkv, heads))
    a, p = AR.core_fwd64(q, k, v)
    want = v[..., pi.to(DEV), :]
    assert (a - want).abs().max().item() < 1e-10
    out, _ = _run_fwd(G, qkv, heads)
    res = cmp_bf16(SR.split_plane(out, heads), want, REL_HALF_ULP * (p @ v.abs()))
    _report("fwd late maximum", res)
    assert res["ok"], res


# ---------------------------------------------------------------------------------------------------------------------
# block
# ---------------------------------------------------------------------------------------------------------------------
def _block(G, at, x):
    ctx = G.ctx()
    with ctx.scope():
        prog = E.Program(ctx)
        y, _ = SA.emit_spatial_attention(prog, at, G.to_act(prog, x))
        prog.finalize_layout()
        prog.run()
        out = G.from_act(prog, y)
    torch.cuda.synchronize()
    return out.cpu(), prog


def _formula_block(ch, heads, seed):
    at = U.SpatialAttention(ch, heads)
    sd = formula_sd(at, seed)
    sd["qkv.weight"][:2 * ch] *= 4.0     # the formula weights give almost flat scores: scale q / k so that the block attends
    sd["proj_out.weight"] *= 4.0         # ... and proj_out, so that the attention term is a sizeable part of the output
    sd["proj_out.bias"] *= 4.0
    at.load_state_dict(sd)
    return at, sd


@pytest.mark.parametrize("ch,heads,shape", [(64, 4, (2, 64, 3, 5, 4)), (256, 4, (1, 256, 2, 6, 6))])
def test_block_against_the_restatement(G, ch, heads, shape):
    at, sd = _formula_block(ch, heads, 4)
    assert float(sd["proj_out.weight"].abs().max()) > 0
    x = formula_input(shape, 5)
    out, prog = _block(G, at, x)
    ref = SR.spatial_attention({"a." + k: v for k, v in sd.items()}, "a", x, heads)
    e, moved = rel_l2(out, ref), rel_l2(ref, x)
    print(f"block {shape}: rel-L2 to the restatement {e:.3e}; the attention term is {moved:.3f} of the input")
    assert e < NET_TOL and moved > 10 * NET_TOL
    names = [m[0] for m in prog.op_meta]
    assert names == ["gn.colsum", "gn.finalize", "gn.apply", "sattn.qkv", "sattn.core", "sattn.proj", "sattn.residual_add"]
    kinds = [a["kind"] for a in prog.op_audit]
    assert kinds[4] == "attn_plane" and kinds[6] == "add"
    n, c, d, h, w = shape
    convs = 2.0 * n * d * h * w * (3 * c * c + c * c)
    assert prog.flops == pytest.approx(convs + 4.0 * n * d * (h * w) ** 2 * c, rel=0.05)      # (conv plans count padded tiles)
    assert {nm for nm, _ in prog.conv_flops} == {"sattn.qkv", "sattn.proj"}
    # the audit record is enough to re-derive the core launch from its own operands
    rec = prog.op_audit[4]
    assert rec["heads"] == heads and rec["qkv"].c == 3 * c and rec["out"].c == c and rec["lse"] is None


def test_block_with_zero_proj_out_is_the_identity(G):
    at, _ = _formula_block(64, 4, 4)
    torch.nn.init.zeros_(at.proj_out.weight)
    torch.nn.init.zeros_(at.proj_out.bias)
    x = formula_input((2, 64, 3, 5, 4), 5)
    out, _ = _block(G, at, x)
    assert torch.equal(out, x.to(torch.bfloat16).float())
    fresh = U.SpatialAttention(64, 4)           # as constructed: zero_module
    assert not fresh.proj_out.weight.any() and not fresh.proj_out.bias.any()
    out, _ = _block(G, fresh, x)
    assert torch.equal(out, x.to(torch.bfloat16).float())


# ---------------------------------------------------------------------------------------------------------------------
# network.  TINY_UNET: level 0 has no temporal attention, level 1 has, and level 1 is the deepest (mid_attn_spatial).  MID_UNET's
# level 0 has head dimension 32 / 8 = 4, which no attention core takes: its levels 1 and 2 (both with temporal attention) and the
# mid block carry the spatial blocks.
# ---------------------------------------------------------------------------------------------------------------------
NET_CASES = [(TINY_UNET, [0, 1], (2, 8, 4, 8, 8), (8, 10, 11), [500, 37]),
             (MID_UNET, [1, 2], (1, 4, 6, 12, 8), (9, 12, 13), [999])]


def _cfg(kw, levels):
    return dict(unet_cfg(kw), spatial_attention_levels=list(levels))


# per network, the smallest power of two at which the float32 restatement moves by more than 10 NET_TOL when the spatial blocks
# are skipped (computed on the CPU from the restatement alone: at 1 -- the formula weights as they are -- tiny moves by 0.324
# and mid by 0.287; at 2 mid moves by 0.511)
PROJ_GAIN = {"tiny": 1.0, "mid": 2.0}


def _boost_spatial_proj(root, sd, gain, prefix=""):
    """Formula weights leave the new blocks a small term: scale every SpatialAttention's proj_out (weight and bias) so that
    the blocks carry weight in the output."""
    for n, m in root.named_modules():
        if type(m).__name__ == "SpatialAttention":
            for leaf in ("weight", "bias"):
                sd[f"{prefix}{n}.proj_out.{leaf}"] = sd[f"{prefix}{n}.proj_out.{leaf}"] * gain
    return sd


def _spatial_model(pkg, kw, levels, seed):
    un = pkg.UNet3D(**kw, spatial_attention_levels=levels)
    # every key of the default model keeps the formula weights the default model has at this seed (the networks of
    # tests/test_gpu_network.py, whose engine error is known to be inside NET_TOL); only the new keys are drawn for this model.
    # (The formula depends on the whole key set: drawn over the larger set, the MID network WITHOUT any spatial contribution --
    # proj_out = 0 -- is already 3.4e-2 from its restatement on the engine and 4.7e-2 under torch's own bf16 autocast.)
    sd = formula_sd(un, seed)
    sd.update(formula_sd(pkg.UNet3D(**kw), seed))
    sd = _boost_spatial_proj(un, sd, PROJ_GAIN["tiny" if kw is TINY_UNET else "mid"])
    un.load_state_dict(sd, strict=True)
    un.eval()
    return un, sd


@pytest.mark.parametrize("kw,levels,shape,seeds,t", NET_CASES, ids=["tiny", "mid"])
def test_unet_forward_against_the_restatement(pkg, kw, levels, shape, seeds, t):
    un, sd = _spatial_model(pkg, kw, levels, seeds[0])
    un.to(DEV)
    x, c, t = formula_input(shape, seeds[1]), formula_input(shape, seeds[2]), torch.tensor(t)
    out = un(x.to(DEV), t.to(DEV), c.to(DEV)).cpu()
    ref = SR.unet_forward(sd, _cfg(kw, levels), x, t, c)
    without = SR.unet_forward(sd, _cfg(kw, ()), x, t, c)          # the same weights, the spatial blocks skipped
    e, gap = rel_l2(out, ref), rel_l2(ref, without)
    print(f"U-Net {shape}: rel-L2 to the restatement {e:.3e}; without the spatial blocks the reference moves by {gap:.3f}")
    assert e < NET_TOL, e
    assert gap > 10 * NET_TOL, gap
    assert torch.equal(un(x.to(DEV), t.to(DEV), c.to(DEV)).cpu(), out)
    names = [m[0] for m in next(p for k, p in un._ctsi_programs.items() if k[0] == "unet").op_meta]
    nblocks = sum(1 for m in un.modules() if type(m).__name__ == "SpatialAttention")
    assert names.count("sattn.core") == nblocks > 0
    # every attention_mode honours the blocks
    un.attention_mode = "softmax"
    with AR.softmax_attention():
        ref_sm = SR.unet_forward(sd, _cfg(kw, levels), x, t, c)
    assert rel_l2(un(x.to(DEV), t.to(DEV), c.to(DEV)).cpu(), ref_sm) < NET_TOL


@pytest.mark.parametrize("kw,levels,shape,seeds,t", NET_CASES, ids=["tiny", "mid"])
def test_zero_proj_out_gives_the_default_models_bits(pkg, kw, levels, shape, seeds, t):
    base = pkg.UNet3D(**kw)
    sd0 = load_formula(base, seeds[0])
    un = pkg.UNet3D(**kw, spatial_attention_levels=levels)
    res = un.load_state_dict(sd0, strict=False)                   # a checkpoint of the default model
    assert not res.unexpected_keys and all("proj_out" in k or ".norm." in k or ".qkv." in k for k in res.missing_keys)
    un.eval()
    base.to(DEV)
    un.to(DEV)
    x, c, t = formula_input(shape, seeds[1]).to(DEV), formula_input(shape, seeds[2]).to(DEV), torch.tensor(t, device=DEV)
    assert torch.equal(un(x, t, c), base(x, t, c))


# ---------------------------------------------------------------------------------------------------------------------
# sampling: the criterion of tests/test_gpu_attn_softmax.py::test_ddim_captured_equals_eager_and_the_restated_oracle
# ---------------------------------------------------------------------------------------------------------------------
LEVELS = [0, 1]


def _noise_fn(i, shape):
    return formula_noise(i, shape)


def _tiny_spatial_model(pkg):
    """tests.helpers.tiny_model_sd with spatial blocks on both levels and the mid block: the formula weights as they are (every
    proj_out non-zero; without the blocks the restated 4-step DDIM latent moves by 0.36 rel-L2)."""
    model = pkg.VideoToVideoDiffusion({**TINY_CFG, "unet_spatial_attention_levels": LEVELS})
    sd = formula_sd(model, 11)
    for k, v in pkg.GaussianDiffusion('cosine', 1000).state_dict().items():
        sd["diffusion." + k] = v
    assert all(float(sd[k].abs().max()) > 0 for k in sd if "mid_attn_spatial.proj_out" in k)
    model.load_state_dict(sd, strict=True)
    model.eval()
    cfg = dict(model_channels=32, num_res_blocks=1, attention_levels=[1], channel_mult=[1, 2], num_heads=4,
               scaling_factor=1.0, spatial_attention_levels=LEVELS)
    return model, sd, cfg


@pytest.fixture(scope="module")
def tiny_spatial(pkg):
    model, sd, cfg = _tiny_spatial_model(pkg)
    model.to(DEV)
    return model, sd, cfg


def _restated_ddim(sd, cfg, shape, cond, n_steps, s=1.0, autocast=False):
    bufs = R.diffusion_buffers("cosine", 1000)

    def net(z, t, c):
        out = SR.unet_forward(sd, cfg, z, t, c, "unet.")
        if s != 1.0:
            un = SR.unet_forward(sd, cfg, z, t, torch.zeros_like(c), "unet.")
            out = un + s * (out - un)
        return out

    def run():
        return R.ddim_sample(net, bufs, shape, cond, n_steps, eta=0.0, noise_fn=_noise_fn).float()

    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            return run()
    return run()


def _sampler_criterion(tag, z, ref, zb):
    e_hip, e_bf = rel_l2(z, ref), rel_l2(zb, ref)
    p_hip, p_bf = R.psnr(z, ref, 20.0), R.psnr(zb, ref, 20.0)
    print(f"{tag}: final latent rel-L2 hip {e_hip:.3e} vs restated autocast {e_bf:.3e}; PSNR {p_hip:.2f} vs {p_bf:.2f} dB")
    assert torch.isfinite(z).all()
    assert p_hip >= p_bf - 0.1, (p_hip, p_bf)


def test_ddim_captured_equals_eager_and_the_restated_oracle(pkg, tiny_spatial):
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    model, sd, cfg = tiny_spatial
    shape, n_steps = (1, 8, 4, 8, 8), 4
    cond = formula_input(shape, 15)
    sp = pkg.DDIMSampler(model.diffusion, model.unet)
    runs = [sp.sample(shape, cond.to(DEV), n_steps, DEV, eta=0.0, progress=False, noise_fn=_noise_fn) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    progs = [p for k, p in model.unet._ctsi_programs.items() if k[0] == "sampler"]
    assert len(progs) == 1 and progs[0].graph is not None
    assert [m[0] for m in progs[0].op_meta[:progs[0].unet_op_count]].count("sattn.core") == 7
    g = model.diffusion
    t_desc = [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(n_steps)]
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope():       # the same steps eagerly: a separately built program, launch by launch (no graph)
        prog = E.UNetProgram(ctx, model.unet, 1, 4, 8, 8, g.timesteps + 1, "fast")
        prog.add_sampler_step("ddim", False)
        prog.load_latents(_noise_fn(-1, shape).to(DEV), cond.to(DEV))
        prog.set_schedule(t_desc, S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0).to(DEV))
        for _ in t_desc:
            prog.run()
        eager = prog.z_ncdhw()
    torch.cuda.synchronize()
    assert torch.equal(eager, runs[0])
    ref = _restated_ddim(sd, cfg, shape, cond, n_steps)
    _sampler_criterion("ddim", runs[0].cpu(), ref, _restated_ddim(sd, cfg, shape, cond, n_steps, autocast=True))
    flat = _restated_ddim(sd, dict(cfg, spatial_attention_levels=[]), shape, cond, n_steps)
    assert rel_l2(ref, flat) > NET_TOL          # the sample depends on the spatial blocks


def test_ddim_with_guidance(pkg, tiny_spatial):
    model, sd, cfg = tiny_spatial
    shape, n_steps = (1, 8, 4, 8, 8), 4
    cond = formula_input(shape, 15)
    z = pkg.DDIMSampler(model.diffusion, model.unet).sample(shape, cond.to(DEV), n_steps, DEV, eta=0.0, progress=False,
                                                            noise_fn=_noise_fn, guidance_scale=2.0).cpu()
    ref = _restated_ddim(sd, cfg, shape, cond, n_steps, s=2.0)
    _sampler_criterion("ddim, guidance 2", z, ref, _restated_ddim(sd, cfg, shape, cond, n_steps, s=2.0, autocast=True))


# ---------------------------------------------------------------------------------------------------------------------
# training: the set-up and criterion of tests/test_gpu_train.py::test_training_step_gradients (formula weights, no mask)
# ---------------------------------------------------------------------------------------------------------------------
T_FIX = torch.tensor([37, 812])


def _train_inputs():
    v_in = formula_input((2, 1, 2, 32, 32), 18).clamp(-1, 1)
    v_gt = formula_input((2, 1, 6, 32, 32), 19).clamp(-1, 1)
    return v_in, v_gt, formula_noise(-1, (2, 8, 6, 8, 8))


def _train_oracle(sd, cfg, autocast=False):
    sd = {k: v.clone() for k, v in sd.items()}
    names = [k for k in sd if k.startswith("unet.")]
    for k in names:
        sd[k].requires_grad_(True)
    v_in, v_gt, noise = _train_inputs()
    with SR.spatial_unet():
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                loss = R.model_training_forward(sd, cfg, v_in, v_gt, T_FIX, noise, None)
        else:
            loss = R.model_training_forward(sd, cfg, v_in, v_gt, T_FIX, noise, None)
        loss.float().backward()
    return float(loss.detach()), {k[len("unet."):]: sd[k].grad.float() for k in names}


def test_training_step_gradients(pkg):
    """Per parameter tensor err_hip <= 2 err_autocast + 2e-2 against the restated fp32 autograd, loss within 2 %; the three thirds
    of every spatial qkv weight are compared on their own and are all non-zero."""
    model, sd, cfg = _tiny_spatial_model(pkg)
    model.to(DEV)
    v_in, v_gt, noise = _train_inputs()
    for p in model.parameters():
        p.grad = None
    loss, _ = model(v_in.to(DEV), v_gt.to(DEV), t=T_FIX.to(DEV), noise=noise.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    ref_loss, ref_g = _train_oracle(sd, cfg)
    ac_loss, ac_g = _train_oracle(sd, cfg, autocast=True)
    print(f"loss: hip {loss.item():.6f}  restated fp32 {ref_loss:.6f}  restated bf16-autocast {ac_loss:.6f}")
    assert abs(loss.item() - ref_loss) <= 2e-2 * abs(ref_loss)
    spatial = {n for n, m in model.unet.named_modules() if type(m).__name__ == "SpatialAttention"}
    assert len(spatial) == 7
    gmax = max(float(g.norm()) for g in ref_g.values())
    rows, nthirds = [], 0
    for name, p in model.unet.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        g = p.grad.float().cpu()
        parts = [("", slice(None))]
        if name.rsplit(".", 2)[0] in spatial and ".qkv." in name:
            c = p.shape[0] // 3
            parts = [("[q]", slice(0, c)), ("[k]", slice(c, 2 * c)), ("[v]", slice(2 * c, 3 * c))]
        for tag, sl in parts:
            r = ref_g[name][sl]
            if tag and name.endswith("weight"):
                nthirds += 1
                assert float(g[sl].norm()) > 0 and float(r.norm()) > 0, (name, tag)
            if float(r.norm()) < 1e-5 * gmax:         # (the k bias: softmax is invariant to a shift of every score of a row)
                assert float(g[sl].norm()) <= 1e-3 * gmax, (name, tag)
                continue
            e_h, e_a = rel_l2(g[sl], r), rel_l2(ac_g[name][sl], r)
            rows.append((e_h / (2 * e_a + 2e-2), e_h, e_a, float(r.norm()) / gmax, name + tag))
    rows.sort(reverse=True)
    for ratio, e_h, e_a, rn, name in rows[:8] + [r for r in rows[8:] if r[4].endswith(("[q]", "[k]", "[v]"))]:
        print(f"  {name:50s} hip {e_h:.3e}  autocast {e_a:.3e}  |g| / max |g| {rn:.3e}")
    assert nthirds == 3 * len(spatial)
    assert rows[0][0] <= 1.0, rows[0]
    for p in model.parameters():
        p.grad = None


def test_two_fused_adamw_steps_equal_a_torch_adamw_twin(pkg):
    """FusedAdamW (fast_repack over the new conv images) against a twin stepped by torch.optim.AdamW through the generic
    re-pack: the losses of two steps are bit-identical."""
    model, _, _ = _tiny_spatial_model(pkg)
    twin, _, _ = _tiny_spatial_model(pkg)
    model.to(DEV)
    twin.to(DEV)
    v_in = formula_input((2, 1, 2, 16, 16), 16).clamp(-1, 1).to(DEV)
    v_gt = formula_input((2, 1, 4, 16, 16), 19).clamp(-1, 1).to(DEV)
    t, nz = torch.tensor([612, 77], device=DEV), formula_noise(-1, (2, 8, 4, 4, 4)).to(DEV)
    for p in list(model.vae.parameters()) + list(twin.vae.parameters()):
        p.requires_grad_(False)
    o1 = pkg.FusedAdamW(model.unet.parameters(), lr=2e-3, weight_decay=0.01, engine_modules=[model.unet])
    o2 = torch.optim.AdamW(twin.unet.parameters(), lr=2e-3, weight_decay=0.01)
    losses = []
    for it in range(2):
        l1, _ = model(v_in, v_gt, t=t, noise=nz)
        l2, _ = twin(v_in, v_gt, t=t, noise=nz)
        losses.append((float(l1), float(l2)))
        l1.backward()
        l2.backward()
        o1.step()
        o2.step()
        o1.zero_grad(set_to_none=True)
        o2.zero_grad(set_to_none=True)
        prog = [pr for k, pr in model.unet.__dict__["_ctsi_programs"].items() if k[0] == "unet-train"][0]
        assert prog._fast is not None and prog._fingerprint() == prog._versions      # nothing left to re-pack
        assert len(prog._fast["slow"]) == 0
    print("losses (fused / torch twin):", losses)
    assert losses[1][0] != losses[0][0]
    for a, b in losses:
        assert a == b, losses


# ---------------------------------------------------------------------------------------------------------------------
# the default path: the launches of the parent commit, name for name
# ---------------------------------------------------------------------------------------------------------------------
def test_default_path_issues_the_parents_launches(pkg):
    with open(GOLDEN) as f:
        want = json.load(f)
    un = pkg.UNet3D(**TINY_UNET)
    load_formula(un, 8)
    un.to(DEV)
    shape = (1, 8, 4, 8, 8)
    x, c = formula_input(shape, 10).to(DEV), formula_input(shape, 11).to(DEV)
    un(x, torch.tensor([500], device=DEV), c)
    g = pkg.GaussianDiffusion()
    pkg.DDIMSampler(g, un).sample(shape, c, 10, DEV, eta=0.0, progress=False, noise_fn=_noise_fn)
    un.train()
    tshape = (2, 8, 2, 6, 6)
    z0, cond, noise = formula_input(tshape, 31).to(DEV), formula_input(tshape, 32).to(DEV), formula_noise(-1, tshape).to(DEV)
    loss, _ = g.to(DEV).training_loss(un, z0, cond, t=T_FIX.to(DEV), noise=noise)
    loss.backward()
    torch.cuda.synchronize()
    got = {}
    for key, prog in un._ctsi_programs.items():
        if key[0] in ("unet", "sampler", "unet-train"):
            assert key[0] not in got
            got[key[0]] = [m[0] for m in prog.op_meta]
    assert set(got) == set(want) == {"unet", "sampler", "unet-train"}
    for k in want:
        assert got[k] == want[k], k
        assert not any(n.startswith("sattn") for n in got[k])


# ---------------------------------------------------------------------------------------------------------------------
# limits: what is not supported is an error with the numbers in it, never a fallback
# ---------------------------------------------------------------------------------------------------------------------
def test_limits(pkg):
    P = importlib.import_module("video-to-video-diffusion_amd.parallel")
    un = pkg.UNet3D(**TINY_UNET, spatial_attention_levels=[1])
    un.to(DEV).eval()
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope():
        with pytest.raises(L.CtsiError, match="shard"):
            E.UNetProgram(ctx, un, 1, 2, 8, 8, 8, "fast", shard=P.ShardSpec(0, 2, P.LocalComm(2), 4))
    x = formula_input((1, 8, 4, 8, 8), 10).to(DEV)
    for prec in ("fp32", "bf16x3"):
        un.inference_precision = prec
        with pytest.raises(L.CtsiError, match=prec):
            un(x, torch.tensor([5], device=DEV), x)
        with pytest.raises(L.CtsiError, match=prec):
            pkg.DDIMSampler(pkg.GaussianDiffusion(), un).sample(tuple(x.shape), x, 2, DEV, progress=False)
    un.inference_precision = "bf16"
    lib = ctx.lib
    q = torch.zeros(2 * 2 * 2 * 3 * 1024, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(4096, dtype=torch.float32, device=DEV)
    with pytest.raises(L.CtsiError, match="head dimension 4 "):
        lib.attn_plane(E._ptr(q), E._ptr(q), None, 1, 16, 2, 2, 2, 4, ctx.sptr)
    with pytest.raises(L.CtsiError, match="head dimension 256 "):
        lib.attn_plane(E._ptr(q), E._ptr(q), None, 1, 1024, 2, 1, 1, 4, ctx.sptr)
    with pytest.raises(L.CtsiError, match="head dimension 4 "):
        lib.attn_plane_bwd(E._ptr(q), E._ptr(q), E._ptr(q), E._ptr(f), E._ptr(q), 1, 16, 2, 2, 2, 4, ctx.sptr)
    with pytest.raises(L.CtsiError, match="head dimension 256 "):
        lib.attn_plane_bwd(E._ptr(q), E._ptr(q), E._ptr(q), E._ptr(f), E._ptr(q), 1, 1024, 2, 1, 1, 4, ctx.sptr)
    small = pkg.UNet3D(**dict(TINY_UNET, num_heads=8), spatial_attention_levels=[0]).to(DEV).eval()     # 32 / 8 = 4
    with pytest.raises(L.CtsiError, match="head dimension 4 "):
        small(x, torch.tensor([5], device=DEV), x)


# ---------------------------------------------------------------------------------------------------------------------
# poison: bit-identical under every fill, guards untouched (tests/poison.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_poison_core(G):
    heads = N143[2]
    qkv, da = _operands(N143)
    n, d, h, w, c3 = qkv.shape
    c = c3 // 3
    ctx = G.ctx()

    def f():
        out = torch.empty((n, d, h, w, c), dtype=torch.bfloat16, device=DEV)
        lse = torch.empty((n, d, heads, h * w), dtype=torch.float32, device=DEV)
        dqkv = torch.empty((n, d, h, w, c3), dtype=torch.bfloat16, device=DEV)
        with ctx.scope():
            ctx.lib.attn_plane(G._ptr(qkv), G._ptr(out), G._ptr(lse), n, c, d, h, w, heads, ctx.sptr)
            ctx.lib.attn_plane_bwd(G._ptr(qkv), G._ptr(out), G._ptr(da), G._ptr(lse), G._ptr(dqkv), n, c, d, h, w, heads,
                                   ctx.sptr)
        torch.cuda.synchronize()
        return {"a": out, "lse": lse, "dqkv": dqkv}

    PZ.run_scenario(f, name="attn_plane[N=143]", engine=False)


def test_poison_unet_forward_and_training_step(pkg):
    un, _ = _spatial_model(pkg, MID_UNET, [1, 2], 9)
    diff = pkg.GaussianDiffusion('cosine', 1000)
    un.to(DEV)
    diff.to(DEV)
    shape = (3, 4, 5, 12, 8)
    z0, cond, noise = (t.to(DEV) for t in (formula_input(shape, 31), formula_input(shape, 32), formula_noise(-1, shape)))
    t = torch.tensor([5, 400, 990], device=DEV)

    def fwd():
        out = un(z0, t, cond)
        torch.cuda.synchronize()
        return out

    PZ.run_scenario(fwd, name="unet[spatial]", modules=[un], ragged=True, inside=PZ.reevaluate(fwd),
                    no_reuse_fills=(NAN, BIG))

    def step():
        for p in un.parameters():
            p.grad = None
        loss, _ = diff.training_loss(un, z0, cond, t=t, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
        g = {k: p.grad for k, p in un.named_parameters() if p.grad is not None}
        assert len(g) == len(list(un.parameters()))
        return {"loss": loss.detach(), "grad": g}

    PZ.run_scenario(step, name="train[spatial]", modules=[un], ragged=True, inside=PZ.reevaluate(step),
                    no_reuse_fills=(NAN, BIG))
    for p in un.parameters():
        p.grad = None
