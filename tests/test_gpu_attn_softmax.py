"""GPU: attention_mode='softmax' -- softmax(Q K^T / sqrt(hd)) V over depth (csrc/attention_core.hip) from the kernel up to
sampling and training, against tests/attn_restatement.py.

Core kernels: float64 from the kernel's own bf16 operands, `cmp_bf16` of tests/train_audit.py (one bf16 ulp + its floor,
rel-L2 4e-3 against bf16(ref)) plus one `extra` term per intermediate rounding the source performs:

  forward   the probabilities are rounded to bf16 for the P V MFMA (ac_pack4 in the kernel; the row sum is taken from the
            unrounded values): half a bf16 ulp of p is at most 2^-8 |p| (8 significant bits, worst at a power of two), whatever
            power-free factor the online rescaling applies afterwards, so |dA[q][c]| <= 2^-8 sum_k P[q][k] |V[k][c]|.
  backward  P is rounded the same way for dV = P^T dA:               |d dV[k][c]| <= 2^-8 sum_q P[q][k] |dA[q][c]|
            dS is rounded to bf16 for dQ = dS K / sqrt(hd) and dK:   |d dQ[q][c]| <= 2^-8 sum_k |dS[q][k]| |K[k][c]| / sqrt(hd)
                                                                     |d dK[k][c]| <= 2^-8 sum_q |dS[q][k]| |Q[q][c]| / sqrt(hd)
  Everything else is fp32 (scores, max, sum, exp2, delta, accumulation of exact bf16 products): ~1e-6 relative, under the floor.

Inputs have peaked scores (q, k ~ N(0, 2): scaled scores of std 2), and every case asserts that its float64 reference is more
than 0.5 rel-L2 away from uniform attention: a kernel that averaged V cannot pass.
"""
import ctypes as C
import importlib

import pytest
import torch

from tests import attn_restatement as AR
from tests.helpers import rel_l2
from tests.train_audit import cmp_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64

# (n, C, heads, D, h, w): hd 16 / 32 / 64 / 128, D below, at and beyond one 64-key pass with remainders, a position count
# that does not fill a block of four items, one production shape, and hd 8
CORE_CASES = [
    (2, 64, 4, 4, 3, 5),
    (1, 64, 4, 1, 3, 5),
    (1, 64, 2, 17, 3, 5),
    (1, 128, 4, 48, 4, 4),
    (1, 256, 4, 64, 2, 3),
    (1, 512, 4, 48, 2, 2),
    (1, 64, 4, 72, 3, 5),
    (1, 128, 4, 130, 2, 2),
    (1, 256, 4, 48, 64, 64),
    (1, 64, 8, 6, 3, 5),          # hd 8 (the mid test network's first attention level): a zero-padded K = 16 MFMA step
]
CORE_IDS = ["n%d_c%d_h%d_d%d_%dx%d" % c for c in CORE_CASES]
REL_HALF_ULP = 2.0 ** -8        # half a bf16 ulp of x is at most this much of |x|


@pytest.fixture(scope="module")
def G():
    from tests import gpu_utils
    return gpu_utils


def _operands(case):
    n, c, heads, d, h, w = case
    g = torch.Generator(device="cpu").manual_seed(1000 + d * 7 + c)
    big = n * d * h * w > 100000
    dev = DEV if big else "cpu"
    if big:
        g = torch.Generator(device=DEV).manual_seed(1000 + d * 7 + c)
    qkv = torch.randn((n, d, h, w, 3 * c), generator=g, device=dev)
    qkv[..., :2 * c] *= 2.0 ** 0.5       # q, k ~ N(0, 2): the scaled scores have std 2
    da = torch.randn((n, d, h, w, c), generator=g, device=dev)
    return qkv.to(DEV, torch.bfloat16).contiguous(), da.to(DEV, torch.bfloat16).contiguous()


def _run_core(G, qkv, heads):
    n, d, h, w, c3 = qkv.shape
    ctx = G.ctx()
    out = torch.full((n, d, h, w, c3 // 3), float("nan"), dtype=torch.bfloat16, device=DEV)
    with ctx.scope():
        ctx.lib.attn_core(G._ptr(qkv), G._ptr(out), n, c3 // 3, d, h, w, heads, ctx.sptr)
    torch.cuda.synchronize()
    return out


def _run_core_bwd(G, qkv, da, heads):
    n, d, h, w, c3 = qkv.shape
    ctx = G.ctx()
    out = torch.full((n, d, h, w, c3), float("nan"), dtype=torch.bfloat16, device=DEV)
    with ctx.scope():
        ctx.lib.attn_core_bwd(G._ptr(qkv), G._ptr(da), G._ptr(out), n, c3 // 3, d, h, w, heads, ctx.sptr)
    torch.cuda.synchronize()
    return out


def _report(tag, res):
    print(f"{tag}: ulps {res['ulps']:.3f} rel_l2 {res['rel_l2']:.3e} max_rel {res['max_rel']:.3e} ok {res['ok']}")


@pytest.fixture(scope="module")
def core_refs(G):
    """Per case, computed once and left unchanged: operands, float64 forward and backward with their rounding terms."""
    cache = {}

    def get(case):
        if case not in cache:
            heads = case[2]
            qkv, da = _operands(case)
            q, k, v = (t.to(F64) for t in AR.split_qkv(qkv, heads))
            g = AR.split_heads(da, heads).to(F64)
            r = AR.core_bwd64(q, k, v, g)
            a, p = AR.core_fwd64(q, k, v)
            sc = q.shape[-1] ** -0.5
            ex = dict(a=REL_HALF_ULP * (p @ v.abs()),
                      dv=REL_HALF_ULP * (p.transpose(-1, -2) @ g.abs()),
                      dq=REL_HALF_ULP * sc * (r["ds"].abs() @ k.abs()),
                      dk=REL_HALF_ULP * sc * (r["ds"].abs().transpose(-1, -2) @ q.abs()))
            cache[case] = dict(qkv=qkv, da=da, a=a, uni=AR.core_uniform64(v), dq=r["dq"], dk=r["dk"], dv=r["dv"], ex=ex)
        return cache[case]

    return get


@pytest.mark.parametrize("case", CORE_CASES, ids=CORE_IDS)
def test_core_forward(G, core_refs, case):
    heads = case[2]
    ref = core_refs(case)
    if case[3] > 1:   # (one key: softmax and a mean are the same function)
        assert rel_l2(ref["uni"], ref["a"]) > 0.5, "the reference must be far from uniform attention"
    out = _run_core(G, ref["qkv"], heads)
    got = AR.split_heads(out, heads)
    res = cmp_bf16(got, ref["a"], ref["ex"]["a"])
    _report("fwd %s" % (case,), res)
    assert res["ok"], res
    assert torch.equal(_run_core(G, ref["qkv"], heads).view(torch.int16), out.view(torch.int16))


@pytest.mark.parametrize("case", CORE_CASES, ids=CORE_IDS)
def test_core_backward(G, core_refs, case):
    heads = case[2]
    ref = core_refs(case)
    out = _run_core_bwd(G, ref["qkv"], ref["da"], heads)
    dq, dk, dv = AR.split_qkv(out, heads)
    bad = []
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        res = cmp_bf16(got, ref[name], ref["ex"][name])
        _report("bwd %s %s" % (name, case), res)
        if not res["ok"]:
            bad.append((name, res))
    assert not bad, bad
    assert torch.equal(_run_core_bwd(G, ref["qkv"], ref["da"], heads).view(torch.int16), out.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------
# block and network
# ---------------------------------------------------------------------------------------------------------------------
from oracle import ref_ops as R                                                                            # noqa: E402
from tests import poison as PZ                                                                             # noqa: E402
from tests.helpers import (MID_UNET, TINY_UNET, formula_input, formula_noise, formula_sd, load_formula,    # noqa: E402
                           tiny_model_sd, unet_cfg)

E = importlib.import_module("video-to-video-diffusion_amd.engine")
L = importlib.import_module("video-to-video-diffusion_amd.lib")
NET_TOL = 3e-2          # tests/test_gpu_network.py: the bf16 engine against the fp32 oracle
NAN, BIG = 0xFF, 0x7F


def _block(G, at, x, mode):
    ctx = G.ctx()
    with ctx.scope():
        prog = E.Program(ctx)
        y = prog.attention(at, G.to_act(prog, x), mode)
        prog.finalize_layout()
        prog.run()
        out = G.from_act(prog, y)
    torch.cuda.synchronize()
    return out.cpu(), prog


@pytest.mark.parametrize("ch,heads,shape", [(64, 4, (2, 64, 6, 5, 4)), (256, 4, (1, 256, 5, 3, 3))])
def test_block_against_the_restatement(G, ch, heads, shape):
    U = importlib.import_module("video-to-video-diffusion_amd.unet3d")
    at = U.TemporalAttention(ch, heads)
    sd = formula_sd(at, 4)
    # the formula weights give almost flat scores: scale the q / k rows so that the block really attends
    sd["qkv.weight"][:2 * ch] *= 4.0
    at.load_state_dict(sd)
    x = formula_input(shape, 5)
    out, prog = _block(G, at, x, "softmax")
    ref = AR.temporal_attention_softmax({"a." + k: v for k, v in sd.items()}, "a", x, heads)
    old = R.temporal_attention({"a." + k: v for k, v in sd.items()}, "a", x, heads)
    e, apart = rel_l2(out, ref), rel_l2(ref - x, old - x)
    print(f"block {shape}: rel-L2 to the restatement {e:.3e}; the two blocks' attention terms are {apart:.3f} apart")
    assert e < NET_TOL and apart > 0.5
    names = [m[0] for m in prog.op_meta]
    assert names == ["gn.colsum", "gn.finalize", "gn.apply", "attn.qkv", "attn.core", "attn.proj", "attn.residual_add"]
    assert all(a is not None and "kind" in a for a in prog.op_audit)
    assert prog.flops > 0 and {n for n, _ in prog.conv_flops} == {"attn.qkv", "attn.proj"}


@pytest.mark.parametrize("kw,shape,seeds,t", [(TINY_UNET, (2, 8, 4, 8, 8), (8, 10, 11), [500, 37]),
                                              (MID_UNET, (1, 4, 6, 12, 8), (9, 12, 13), [999])], ids=["tiny", "mid"])
def test_unet_forward_against_the_restatement(pkg, kw, shape, seeds, t):
    un = pkg.UNet3D(**kw)
    sd = load_formula(un, seeds[0])
    un.to(DEV)
    x, c, t = formula_input(shape, seeds[1]), formula_input(shape, seeds[2]), torch.tensor(t)
    fast = un(x.to(DEV), t.to(DEV), c.to(DEV)).cpu()
    un.attention_mode = "softmax"
    out = un(x.to(DEV), t.to(DEV), c.to(DEV)).cpu()
    ref = AR.unet_forward(sd, unet_cfg(kw), x, t, c)
    e, apart = rel_l2(out, ref), rel_l2(out, fast)
    print(f"U-Net {shape}: rel-L2 to the restatement {e:.3e}, to the fast mode of the same model {apart:.3f}")
    assert e < NET_TOL, e
    assert apart > 0.5, apart
    assert torch.equal(un(x.to(DEV), t.to(DEV), c.to(DEV)).cpu(), out)
    un.attention_mode = "fast"
    assert torch.equal(un(x.to(DEV), t.to(DEV), c.to(DEV)).cpu(), fast)      # switching back returns the earlier bits


# ---------------------------------------------------------------------------------------------------------------------
# sampling: the criterion of tests/test_gpu_network.py (rmse_hip <= 1.0116 rmse_autocast, i.e. PSNR within 0.1 dB of the
# oracle under PyTorch's own bf16 autocast), with the restated oracle as reference and as autocast yardstick
# ---------------------------------------------------------------------------------------------------------------------
def _noise_fn(i, shape):
    return formula_noise(i, shape)


@pytest.fixture(scope="module")
def tiny_softmax(pkg):
    model, sd, cfg = tiny_model_sd(pkg)
    model.to(DEV)
    model.unet.attention_mode = "softmax"
    return model, sd, cfg


def _restated_ddim(model, sd, cfg, shape, cond, n_steps, s=1.0, autocast=False):
    """The oracle's DDIM loop on the restated U-Net; `s` != 1: classifier-free guidance on the zero conditioning; a
    v-prediction model's output is converted to eps from the loop's own z and t."""
    bufs = R.diffusion_buffers("cosine", 1000)
    v_pred = model.diffusion.prediction_type == "v_prediction"
    ac = bufs["alphas_cumprod"].double()

    def net(z, t, c):
        out = R.unet_forward(sd, cfg, z, t, c, "unet.")
        if s != 1.0:
            un = R.unet_forward(sd, cfg, z, t, torch.zeros_like(c), "unet.")
            out = un + s * (out - un)
        if v_pred:
            a = ac[t].sqrt().view(-1, 1, 1, 1, 1).to(out.dtype)
            b = (1 - ac[t]).sqrt().view(-1, 1, 1, 1, 1).to(out.dtype)
            out = a * out + b * z
        return out

    def run():
        with AR.softmax_attention():
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


def test_ddim_captured_equals_eager_and_the_restated_oracle(pkg, tiny_softmax):
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    model, sd, cfg = tiny_softmax
    shape, n_steps = (1, 8, 4, 8, 8), 4
    cond = formula_input(shape, 15)
    sp = pkg.DDIMSampler(model.diffusion, model.unet)
    runs = [sp.sample(shape, cond.to(DEV), n_steps, DEV, eta=0.0, progress=False, noise_fn=_noise_fn) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    progs = [p for k, p in model.unet._ctsi_programs.items() if k[0] == "sampler" and "softmax" in k]
    assert len(progs) == 1 and progs[0].graph is not None
    assert "attn.core" in [m[0] for m in progs[0].op_meta[:progs[0].unet_op_count]]
    g = model.diffusion
    t_desc = [int(t) for t in S.DDIMSampler(g, None)._get_timesteps(n_steps)]
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope():       # the same steps eagerly: a separately built program, launch by launch (no graph)
        prog = E.UNetProgram(ctx, model.unet, 1, 4, 8, 8, g.timesteps + 1, "softmax")
        prog.add_sampler_step("ddim", False)
        prog.load_latents(_noise_fn(-1, shape).to(DEV), cond.to(DEV))
        prog.set_schedule(t_desc, S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0).to(DEV))
        for _ in t_desc:
            prog.run()
        eager = prog.z_ncdhw()
    torch.cuda.synchronize()
    assert torch.equal(eager, runs[0])
    ref = _restated_ddim(model, sd, cfg, shape, cond, n_steps)
    _sampler_criterion("ddim", runs[0].cpu(), ref, _restated_ddim(model, sd, cfg, shape, cond, n_steps, autocast=True))


def test_ddim_with_guidance(pkg, tiny_softmax):
    model, sd, cfg = tiny_softmax
    shape, n_steps = (1, 8, 4, 8, 8), 4
    cond = formula_input(shape, 15)
    z = pkg.DDIMSampler(model.diffusion, model.unet).sample(shape, cond.to(DEV), n_steps, DEV, eta=0.0, progress=False,
                                                            noise_fn=_noise_fn, guidance_scale=2.0).cpu()
    ref = _restated_ddim(model, sd, cfg, shape, cond, n_steps, s=2.0)
    _sampler_criterion("ddim, guidance 2", z, ref, _restated_ddim(model, sd, cfg, shape, cond, n_steps, s=2.0, autocast=True))


def test_ddim_with_v_prediction(pkg, tiny_softmax):
    model, sd, cfg = tiny_softmax
    shape, n_steps = (1, 8, 4, 8, 8), 4
    cond = formula_input(shape, 15)
    gv = pkg.GaussianDiffusion('cosine', 1000, prediction_type="v_prediction").to(DEV)

    class _M:
        diffusion = gv

    z = pkg.DDIMSampler(gv, model.unet).sample(shape, cond.to(DEV), n_steps, DEV, eta=0.0, progress=False,
                                               noise_fn=_noise_fn).cpu()
    ref = _restated_ddim(_M, sd, cfg, shape, cond, n_steps)
    _sampler_criterion("ddim, v-prediction", z, ref, _restated_ddim(_M, sd, cfg, shape, cond, n_steps, autocast=True))


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
    with AR.softmax_attention():
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                loss = R.model_training_forward(sd, cfg, v_in, v_gt, T_FIX, noise, None)
        else:
            loss = R.model_training_forward(sd, cfg, v_in, v_gt, T_FIX, noise, None)
        loss.float().backward()
    return float(loss.detach()), {k[len("unet."):]: sd[k].grad.float() for k in names}


def test_training_step_gradients(pkg):
    """Per parameter tensor err_hip <= 2 err_autocast + 2e-2 against the restated fp32 oracle, loss within 2 %; the q and k
    thirds of every qkv weight -- exactly zero in the other modes -- are compared on their own (measured with this input:
    0.8-1.9 % of the largest gradient norm, the restatement's own autocast error on them 3.8-4.5 %)."""
    model, sd, cfg = tiny_model_sd(pkg)
    model.to(DEV)
    model.unet.attention_mode = "softmax"
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
    gmax = max(float(g.norm()) for g in ref_g.values())
    rows, nqk = [], 0
    for name, p in model.unet.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        g = p.grad.float().cpu()
        parts = [("", slice(None))]
        if ".qkv." in name:
            c = p.shape[0] // 3
            parts = [("[q]", slice(0, c)), ("[k]", slice(c, 2 * c)), ("[v]", slice(2 * c, 3 * c))]
        for tag, sl in parts:
            r = ref_g[name][sl]
            if tag in ("[q]", "[k]") and name.endswith("weight"):
                nqk += 1
                assert float(g[sl].norm()) > 0 and float(r.norm()) > 1e-3 * gmax, (name, tag)
            if float(r.norm()) < 1e-5 * gmax:         # (the k bias: softmax is invariant to a shift of every score of a row)
                assert float(g[sl].norm()) <= 1e-3 * gmax, (name, tag)
                continue
            e_h, e_a = rel_l2(g[sl], r), rel_l2(ac_g[name][sl], r)
            rows.append((e_h / (2 * e_a + 2e-2), e_h, e_a, float(r.norm()) / gmax, name + tag))
    rows.sort(reverse=True)
    for ratio, e_h, e_a, rn, name in rows[:8] + [r for r in rows[8:] if r[4].endswith(("[q]", "[k]"))]:
        print(f"  {name:50s} hip {e_h:.3e}  autocast {e_a:.3e}  |g| / max |g| {rn:.3e}")
    assert nqk == 2 * sum(1 for n, _ in model.unet.named_parameters() if n.endswith("qkv.weight")) > 0
    assert rows[0][0] <= 1.0, rows[0]
    for p in model.parameters():
        p.grad = None


# ---------------------------------------------------------------------------------------------------------------------
# limits
# ---------------------------------------------------------------------------------------------------------------------
def test_limits(pkg):
    P = importlib.import_module("video-to-video-diffusion_amd.parallel")
    un = pkg.UNet3D(**TINY_UNET)
    load_formula(un, 8)
    un.to(DEV)
    un.attention_mode = "softmax"
    ctx = E.Ctx.get(torch.device(DEV))
    with ctx.scope():
        with pytest.raises(L.CtsiError, match="shard"):
            E.UNetProgram(ctx, un, 1, 2, 8, 8, 8, "softmax", shard=P.ShardSpec(0, 2, P.LocalComm(2), 4))
    x = formula_input((1, 8, 4, 8, 8), 10).to(DEV)
    un.inference_precision = "fp32"
    with pytest.raises(L.CtsiError, match="fp32"):
        un(x, torch.tensor([5], device=DEV), x)
    un.inference_precision = "bf16"
    un.attention_mode = "sofmax"
    with pytest.raises(ValueError, match="attention_mode"):
        un(x, torch.tensor([5], device=DEV), x)
    with pytest.raises(ValueError, match="attention_mode"):
        pkg.DDIMSampler(pkg.GaussianDiffusion(), un).sample(tuple(x.shape), x, 2, DEV, progress=False)
    with pytest.raises(ValueError, match="attention_mode"):
        pkg.GaussianDiffusion().to(DEV).training_loss(un, x, x)
    # what the kernels do not take is an error with the numbers in it, never a wrong answer
    lib = ctx.lib
    q = torch.zeros(1 * 2 * 2 * 2 * 3 * 96, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.CtsiError, match="24"):
        lib.attn_core(E._ptr(q), E._ptr(q), 1, 96, 2, 2, 2, 4, ctx.sptr)          # hd 24
    with pytest.raises(L.CtsiError, match="1024"):
        lib.attn_core(E._ptr(q), E._ptr(q), 1, 1024, 2, 1, 1, 4, ctx.sptr)        # hd 256: above the limit


# ---------------------------------------------------------------------------------------------------------------------
# poison: bit-identical under every fill, guards untouched (tests/poison.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_poison_block(G):
    U = importlib.import_module("video-to-video-diffusion_amd.unet3d")
    ctx = G.ctx()
    cases = []
    for ch, seed, shape, k in [(64, 4, (2, 64, 6, 5, 4), 5), (256, 5, (1, 256, 5, 3, 3), 6)]:
        at = U.TemporalAttention(ch, 4)
        at.load_state_dict(formula_sd(at, seed))
        cases.append((at, formula_input(shape, k)))

    def f():
        outs = []
        for at, x in cases:
            with ctx.scope():
                prog = E.Program(ctx)
                y = prog.attention(at, G.to_act(prog, x), "softmax")
                prog.finalize_layout()
                prog.run()
                outs.append(G.from_act(prog, y))
            torch.cuda.synchronize()
        return outs

    PZ.run_scenario(f, name="attention[softmax]", ragged=True, no_reuse_fills=(NAN, BIG))


def test_poison_unet_forward_and_training_step(pkg):
    un = pkg.UNet3D(**MID_UNET)
    load_formula(un, 9)
    diff = pkg.GaussianDiffusion('cosine', 1000)
    un.to(DEV)
    diff.to(DEV)
    un.attention_mode = "softmax"
    shape = (3, 4, 5, 12, 8)
    z0, cond, noise = (t.to(DEV) for t in (formula_input(shape, 31), formula_input(shape, 32), formula_noise(-1, shape)))
    t = torch.tensor([5, 400, 990], device=DEV)

    def fwd():
        out = un(z0, t, cond)
        torch.cuda.synchronize()
        return out

    PZ.run_scenario(fwd, name="unet[softmax]", modules=[un], ragged=True, inside=PZ.reevaluate(fwd),
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

    PZ.run_scenario(step, name="train[softmax]", modules=[un], ragged=True, inside=PZ.reevaluate(step),
                    no_reuse_fills=(NAN, BIG))
    for p in un.parameters():
        p.grad = None
