"""GPU: no kernel reads memory nobody wrote, and none stores outside its buffer (tests/poison.py).

Every scenario `f() -> public results` runs (1) twice plainly: bit-identical; (2) with every torch.empty / zeros allocation
inside a block pre-filled with 0x00, 0xFF (NaN) and 0x7F (3.4e38): bit-identical to the plain run; (3) with the 1 MiB guard
bands around every allocation intact afterwards; (4) where one program is launched repeatedly, again after its scratch (the
activation pool and the column-sum slab) was refilled with the fill byte, captured-graph replay included; (5) at the small
shapes and config 1, with buffer reuse switched off (every activation in a poisoned buffer of its own).  The engine has no
floating-point atomics, so "bit-identical" needs no tolerance.  Nothing here consults the oracle: the engine is compared
with itself.  The module prints a table of kernel names against the scenarios that ran them poisoned."""
import contextlib
import importlib
import time

import pytest
import torch
import torch.nn.functional as F

from tests import poison as PZ
from tests import test_gpu_ops as OPS
from tests.helpers import (MID_UNET, TINY_UNET, bf16_round, build_full_model, build_prod_vae, formula_input, formula_noise,
                           formula_sd, load_formula, tiny_model_sd)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = importlib.import_module("video-to-video-diffusion_amd.engine")
PAR = importlib.import_module("video-to-video-diffusion_amd.parallel")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
NAN, BIG = 0xFF, 0x7F
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _coverage_table():
    yield
    print("\n\n==== kernels run under poison (Program.op_meta name) -> scenarios ====")
    for k in sorted(PZ.COVERAGE):
        sc = sorted(PZ.COVERAGE[k])
        print(f"  {k:34s} {len(sc):3d}  {', '.join(sc[:6])}{', ...' if len(sc) > 6 else ''}")
    print(f"==== {len(PZ.COVERAGE)} kernel names; module wall time {time.time() - _T0:.1f} s ====")


@pytest.fixture(scope="module")
def G():
    from tests import gpu_utils
    return gpu_utils


def _free():
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _case(table, name):
    return next(c for c in table if c[0] == name)


def _noise_fn(i, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 + i))


@contextlib.contextmanager
def _eager():
    """Programs built inside never capture: Program.launch() then runs the op list launch by launch."""
    real = E.Program.capture
    E.Program.capture = lambda self: None
    try:
        yield
    finally:
        E.Program.capture = real


# ---------------------------------------------------------------------------------------------------------------------
# the harness bites on this device too: the three planted defects, torch ops inside one guarded block
# ---------------------------------------------------------------------------------------------------------------------
def test_planted_defects_are_caught_on_the_device():
    for below in (True, False):
        with PZ.poisoned(NAN, engine=False) as P:
            PZ.toy_overrun(DEV, below)
            (site, off, cnt), = P.check_guards()
            assert "toy_overrun" in site and (off, cnt) == ((-4, 4) if below else (256, 4))

    def found(toy, fill):
        return PZ.evaluate_scenario(lambda: toy(DEV), name=toy.__name__, fills=(fill,), engine=False, reference_fill=0x00)[1]

    assert found(PZ.toy_read_unwritten, NAN) and found(PZ.toy_read_unwritten, BIG) and not found(PZ.toy_read_unwritten, 0)
    assert found(PZ.toy_times_zero, NAN) and not found(PZ.toy_times_zero, BIG)
    assert found(PZ.toy_max, BIG) and not found(PZ.toy_max, NAN)


def test_an_activation_nobody_wrote_reads_as_the_fill(G):
    """The poison reaches the engine's kernels: a pool activation that no op has written, read back through the layout
    kernel, is the fill pattern (bf16 NaN / 3.39e38 / 0) -- and the program's buffers all lie in guarded blocks."""
    ctx = G.ctx()
    for fill, check in ((NAN, lambda t: bool(torch.isnan(t).all())), (BIG, lambda t: bool((t > 3.3e38).all())),
                        (0x00, lambda t: bool((t == 0).all()))):
        with PZ.poisoned(fill) as P:
            with ctx.scope():
                prog = E.Program(ctx)
                a = prog.act(2, 24, 3, 5, 7)
                prog.finalize_layout()
                out = G.from_act(prog, a)
            torch.cuda.synchronize()
            assert check(out), fill
            assert P.block_of(a.t) is not None and P.check_guards() == []
            P.assert_wired()
            P.assert_guard_covers(ragged=True)
            assert (P.acts, P.max_row_pitch, P.max_slice_bytes) == (1, 7 * 24 * 2, 5 * 7 * 24 * 2)


# ---------------------------------------------------------------------------------------------------------------------
# single ops through gpu_utils.run_conv: every kernel form the op tests select by override, at the ragged case of its table
# ---------------------------------------------------------------------------------------------------------------------
def _conv_operands(c1, c2, cout, dims, kshape, seeds=(1, 2, 3, 4), transposed=False):
    n, d, h, w = dims
    x1 = bf16_round(formula_input((n, c1, d, h, w), seeds[0]))
    x2 = bf16_round(formula_input((n, c2, d, h, w), seeds[1])) if c2 else None
    wshape = (c1 + c2, cout) + kshape if transposed else (cout, c1 + c2) + kshape
    wt = bf16_round(OPS._w(wshape, seeds[2], transposed=transposed))
    return x1, x2, wt, formula_input((cout,), seeds[3]) * 0.1


def _conv_scenario(G, monkeypatch, name, env, operands, **kw):
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    x1, x2, wt, b = operands

    def f():
        y, sums = G.run_conv(x1, x2, wt, b, **kw)
        return {"y": y, "gn_sums": sums}

    PZ.run_scenario(f, name=name, ragged=True, no_reuse_fills=(NAN, BIG))


@pytest.mark.parametrize("tile", OPS.HALO3_TILES)
@pytest.mark.parametrize("case", ["ragged_edges_batch2", "cin32_cout_72_pad", "concat_64+32_cout256"])
def test_conv3_halo_tiles(G, monkeypatch, case, tile):
    _, c1, c2, cout, dims = _case(OPS.HALO3_CASES, case)
    _conv_scenario(G, monkeypatch, f"conv3[{tile}]:{case}", OPS.halo3_tile_env(tile),
                   _conv_operands(c1, c2, cout, dims, (3, 3, 3)), want_stats=True, groups=8)


@pytest.mark.parametrize("case", ["w24_256_256_ragged_depth", "w12_ragged_h_and_d", "w36_three_tiles_of_12"])
def test_conv3_narrow_plane_tiles(G, monkeypatch, case):
    _, c1, c2, cout, dims, _ = _case(OPS.NARROW_CASES, case)
    _conv_scenario(G, monkeypatch, f"conv3[narrow]:{case}", {"CTSI_CONV_K32_NARROW": "1"},
                   _conv_operands(c1, c2, cout, dims, (3, 3, 3)), want_stats=True, groups=8)


@pytest.mark.parametrize("name,env,c1,c2,cout,dims", [
    ("narrow-split-K:w12_concat_ragged", {"CTSI_CONV_K32_NARROW": "1", "CTSI_CONV_K32_NARROW_SK": "1"}, 128, 128, 72, (1, 11, 10, 12)),
    ("narrow-split-K:w24_256_256", {"CTSI_CONV_K32_NARROW": "1", "CTSI_CONV_K32_NARROW_SK": "1"}, 256, 0, 256, (2, 6, 8, 24)),
    ("k32-split-K:ragged_batch2_512_256", {"CTSI_CONV_FORCE_HALO3": "1", "CTSI_CONV_K32_SPLITK": "1"}, 512, 0, 256, (2, 7, 11, 16)),
], ids=lambda v: v if isinstance(v, str) else None)
def test_conv3_split_k(G, monkeypatch, name, env, c1, c2, cout, dims):
    _conv_scenario(G, monkeypatch, name, env, _conv_operands(c1, c2, cout, dims, (3, 3, 3)), want_stats=True, groups=8)
    E.check_device_errors(G.ctx())


@pytest.mark.parametrize("tile", OPS.DOWN_TILES)
@pytest.mark.parametrize("case", ["ragged_batch2_64_64", "cin16_cout72"])
def test_downsample_conv_tiles(G, monkeypatch, case, tile):
    _, cin, cout, dims = _case(OPS.DOWN_CASES, case)
    _conv_scenario(G, monkeypatch, f"down[{tile}]:{case}", OPS.down_tile_env(tile),
                   _conv_operands(cin, 0, cout, dims, (3, 4, 4)), k=(3, 4, 4), s=(2, 2), want_stats=True, groups=8)
    E.check_device_errors(G.ctx())


@pytest.mark.parametrize("tile", OPS.CONVT_TILES)
@pytest.mark.parametrize("case", ["ragged_batch2", "cout_72_pad_16ch"])
def test_conv_transpose_tiles(G, monkeypatch, case, tile):
    _, cin, cout, dims = _case(OPS.CONVT_CASES, case)
    _conv_scenario(G, monkeypatch, f"convT[{tile}]:{case}", OPS.convt_tile_env(tile),
                   _conv_operands(cin, 0, cout, dims, (3, 4, 4), seeds=(61, 61, 62, 63), transposed=True),
                   transposed=True, k=(3, 4, 4), s=(2, 2), want_stats=True, groups=8)


@pytest.mark.parametrize("case", ["forced_3_two_sources_ragged", "level_6x6_256_256", "forced_2_1x1x1_k1024"])
def test_gather_kernel_split_k(G, monkeypatch, case):
    _, c1, c2, cout, dims, k, force = _case(OPS.GSPLIT_CASES, case)
    env = {"CTSI_CONV_NO_HALO3": "1"}
    if force:
        env["CTSI_CONV_GSPLIT"] = force
    _conv_scenario(G, monkeypatch, f"gather-split-K:{case}", env, _conv_operands(c1, c2, cout, dims, (k, k, k)),
                   k=(k, k, k), p=(k // 2,) * 3, want_stats=True, groups=8)
    E.check_device_errors(G.ctx())


@pytest.mark.parametrize("tile", ["128x128", "256x128", "256x256"])
def test_gather_kernel_tile_variants(G, monkeypatch, tile):
    env = {"CTSI_CONV_TILE": tile}
    _conv_scenario(G, monkeypatch, f"gather[{tile}]:two_sources_ragged", env,
                   _conv_operands(128, 64, 256, (1, 5, 12, 10), (3, 3, 3)), want_stats=True, groups=32)
    x1, _, wt, _ = _conv_operands(128, 0, 128, (1, 5, 12, 10), (3, 4, 4), seeds=(1, 1, 5, 4), transposed=True)
    _conv_scenario(G, monkeypatch, f"gather[{tile}]:convT", env, (x1, None, wt, None), transposed=True, k=(3, 4, 4), s=(2, 2))


_FAMILY = {"k3": dict(), "k1": dict(k=(1, 1, 1), p=(0, 0, 0)), "down": dict(k=(3, 4, 4), s=(2, 2)),
           "up": dict(k=(3, 4, 4), s=(2, 2), transposed=True)}


@pytest.mark.parametrize("case", ["3x3x3_odd_edges_batch2", "3x3x3_concat_64+32_kpad", "3x3x3_small_cin16_two_sources",
                                  "3x3x3_small_cin32", "3x3x3_cout8_bn32", "1x1x1_two_sources", "1x1x1_small_8_8",
                                  "down_128_odd", "down_64_odd_planes_7x9", "down_128_cout32", "convT_small_cin32",
                                  "convT_256_128"])
def test_conv_family_default_plans(G, monkeypatch, case):
    _, c1, c2, cout, dims, kind = _case(OPS.CONV_CASES, case)
    kw = _FAMILY[kind]
    ops = _conv_operands(c1, c2, cout, dims, kw.get("k", (3, 3, 3)), transposed=kind == "up")
    _conv_scenario(G, monkeypatch, f"conv:{case}", {}, ops, want_stats=True,
                   groups=8 if cout % 8 == 0 and cout >= 8 else 1, **kw)


@pytest.mark.parametrize("cout,dims", [(128, (2, 5, 11, 37)), (72, (1, 3, 9, 33))], ids=["ragged_batch2", "cout72_padded"])
@pytest.mark.parametrize("stem", ["stem", "gather-small-cin"])
def test_one_channel_stem_with_padded_input(G, monkeypatch, stem, cout, dims):
    """c1_pad (8) > c1 (1): the 7 pad channels of the input are zero by contract (to_act's zero-initialised buffer) and the
    weights carry one input channel."""
    x1, _, wt, b = _conv_operands(1, 0, cout, dims, (3, 3, 3))
    _conv_scenario(G, monkeypatch, f"{stem}:cout{cout}", {} if stem == "stem" else {"CTSI_CONV_NO_STEM": "1"}, (x1, None, wt, b),
                   c1_pad=8, cin_w=1, want_stats=True, groups=8)


@pytest.mark.parametrize("case", ["vae_head_128_1_tanh", "ragged_batch2_64_4", "cout16_bf16_stats", "cout8_bf16_stats_deep"])
def test_conv3_head_kernel(G, monkeypatch, case):
    _, cin, cout, dims, f32, act = _case(OPS.HEAD_CASES, case)
    _conv_scenario(G, monkeypatch, f"head:{case}", {"CTSI_CONV_FORCE_HALO3": "1", "CTSI_CONV_NO_HEAD2": "1"},
                   _conv_operands(cin, 0, cout, dims, (3, 3, 3), seeds=(31, 31, 32, 33)), f32=f32, act=act, want_stats=not f32,
                   groups=1 if cout < 8 else cout // 4)


@pytest.mark.parametrize("case", ["vae_head_ragged", "unet_head_tiles_batch2_segments", "unet_head_bf16_out"])
def test_conv3_head2_kernel(G, monkeypatch, case):
    _, cout, dims, f32, act = _case(OPS.HEAD2_CASES, case)
    _conv_scenario(G, monkeypatch, f"head2:{case}", {"CTSI_CONV_FORCE_HALO3": "1"},
                   _conv_operands(128, 0, cout, dims, (3, 3, 3), seeds=(41, 41, 42, 43)), f32=f32, act=act)


def test_conv_fp32_strided_output_default_plans(G, monkeypatch):
    x1, _, wt, _ = _conv_operands(128, 0, 1, (1, 3, 6, 5), (3, 3, 3), seeds=(5, 5, 6, 4))
    _conv_scenario(G, monkeypatch, "f32-out:vae_head_tanh", {}, (x1, None, wt, torch.tensor([0.05])), f32=True, act=1)
    x1, _, wt, _ = _conv_operands(128, 0, 8, (1, 3, 6, 5), (3, 3, 3), seeds=(5, 5, 7, 4))
    _conv_scenario(G, monkeypatch, "f32-out:unet_head", {}, (x1, None, wt, None), f32=True)
    x1, _, wt, _ = _conv_operands(1, 0, 32, (2, 3, 9, 7), (3, 3, 3), seeds=(8, 8, 9, 4))
    _conv_scenario(G, monkeypatch, "c1_pad8:cin1_cout32", {}, (x1, None, wt, None), c1_pad=8, cin_w=1)


@pytest.mark.parametrize("case", ["128_to_256_ragged_voxels", "256+128_to_128_batch2", "512+256_to_256_6chunks", "128+128_to_128_nt4"])
@pytest.mark.parametrize("stream", ["stream", "gather-tail"])
def test_residual_tail(G, monkeypatch, stream, case):
    """out = silu?(gn(h) + W [x1 | x2] + b) written over h: the streaming 1x1x1 kernel and the gather kernel's fused tail."""
    _, c1, c2, cout, dims, silu, nt = _case(OPS.TAIL_CASES, case)
    n, d, h, w = dims
    ctx = G.ctx()
    x1, x2, wt, bias = _conv_operands(c1, c2, cout, dims, (1, 1, 1), seeds=(21, 22, 24, 25))
    hh = bf16_round(formula_input((n, cout, d, h, w), 23) * 1.5 + 0.25)
    gnm = torch.nn.GroupNorm(32, cout)
    with torch.no_grad():
        gnm.weight.copy_(1 + 0.2 * formula_input((cout,), 26))
        gnm.bias.copy_(0.1 * formula_input((cout,), 27))
    monkeypatch.setenv("CTSI_CONV1_STREAM", "2" if stream == "stream" else "0")
    if nt is not None:
        monkeypatch.setenv("CTSI_CONV1_STREAM_NT", str(nt))

    def f():
        with ctx.scope():
            prog = E.Program(ctx)
            a1 = G.to_act(prog, x1)
            a2 = G.to_act(prog, x2) if x2 is not None else None
            ah = G.to_act(prog, hh)
            slot = prog.gn_finalize(ah, 32, prog.gn_colsum(ah))
            y, _ = prog.conv("res1x1+gn", lambda: wt, lambda: bias, a1, a2, k=(1, 1, 1), p=(0, 0, 0), cout=cout, out=ah,
                             fuse_gn=(ah, slot, gnm, silu))
            prog.finalize_layout()
            prog.run()
            out = G.from_act(prog, y)
        torch.cuda.synchronize()
        return out

    PZ.run_scenario(f, name=f"tail[{stream}]:{case}", ragged=True, no_reuse_fills=(NAN, BIG))


@pytest.mark.parametrize("shape", [(2, 64, 3, 5, 7), (1, 192, 2, 3, 5)], ids=["c64-small", "c192-lds-coefficients"])
def test_groupnorm_apply_variants(G, shape):
    """All 16 option combinations of gn_apply (out of place: a fresh pool buffer), statistics through gn_colsum + gn_finalize."""
    ctx = G.ctx()
    n, c, d, h, w = shape
    x = bf16_round(formula_input(shape, 11) * 2 + 0.5)
    res = bf16_round(formula_input(shape, 12))
    gnm = torch.nn.GroupNorm(8, c)
    with torch.no_grad():
        gnm.weight.copy_(1 + 0.2 * formula_input((c,), 13))
        gnm.bias.copy_(0.1 * formula_input((c,), 14))
    tb = formula_input((3 * n, c + 16), 15)

    def f():
        outs = {}
        for bits in range(16):
            silu_pre, use_tb, use_res, silu_post = (bits >> 3) & 1, (bits >> 2) & 1, (bits >> 1) & 1, bits & 1
            with ctx.scope():
                prog = E.Program(ctx)
                a = G.to_act(prog, x)
                r = G.to_act(prog, res) if use_res else None
                slot = prog.gn_finalize(a, 8, prog.gn_colsum(a))
                tbd = tb.to(ctx.device)
                sp = torch.tensor([2], dtype=torch.int32, device=ctx.device)
                y = prog.gn_apply(a, slot, gnm, silu_pre=bool(silu_pre), tbias=tbd if use_tb else None, tbias_off=16,
                                  tbias_stride=c + 16, step_ptr=sp if use_tb else None, residual=r, silu_post=bool(silu_post))
                prog.finalize_layout()
                prog.run()
                outs[f"{bits:04b}"] = G.from_act(prog, y)
                outs[f"{bits:04b}.sums"] = prog._gn_sums.clone()
            torch.cuda.synchronize()
        return outs

    PZ.run_scenario(f, name=f"gn_apply:{shape}", ragged=True, no_reuse_fills=(NAN, BIG))


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("pv", ["fused-pv", "normsum+conv"])
def test_attention_block(G, monkeypatch, pv, mode):
    U = importlib.import_module("video-to-video-diffusion_amd.unet3d")
    ctx = G.ctx()
    if pv != "fused-pv":
        monkeypatch.setenv("CTSI_NO_ATTN_PV", "1")
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
                y = prog.attention(at, G.to_act(prog, x), mode)
                prog.finalize_layout()
                prog.run()
                outs.append(G.from_act(prog, y))
            torch.cuda.synchronize()
        return outs

    PZ.run_scenario(f, name=f"attention[{mode},{pv}]", ragged=True, no_reuse_fills=(NAN, BIG))


# ---------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------
def _sample(model, kind, shape, cond, steps, **kw):
    if kind == "ddpm":
        return S.DDPMSampler(model.diffusion, model.unet).sample(shape, cond, DEV, progress=False, noise_fn=_noise_fn,
                                                                 num_steps=steps, **kw)
    return S.SAMPLERS[kind](model.diffusion, model.unet, shape, cond, steps, DEV, progress=False, noise_fn=_noise_fn, **kw)


@pytest.fixture(scope="module")
def tiny(pkg):
    model, _, _ = tiny_model_sd(pkg)
    model.to(DEV)
    yield model
    model.invalidate_engine_cache()


SAMPLER_CASES = [("ddim", {}), ("ddpm", {}), ("dpmpp_2m", {}), ("heun", {}),
                 ("ddim", dict(guidance_scale=2.5)), ("heun", dict(guidance_scale=2.5, guidance_rescale=0.7)),
                 ("ddpm", dict(guidance_scale=0.0, guidance_rescale=0.5))]


@pytest.mark.parametrize("launch", ["graph", "eager"])
@pytest.mark.parametrize("kind,kw", SAMPLER_CASES, ids=[f"{k}{'-cfg' if kw else ''}{'-rescale' if 'guidance_rescale' in kw else ''}"
                                                        for k, kw in SAMPLER_CASES])
def test_tiny_sampling_odd_volume(tiny, kind, kw, launch):
    shape = (1, 8, 5, 6, 10)
    cond = formula_input(shape, 12).to(DEV)

    def f():
        traj = []
        with (_eager() if launch == "eager" else contextlib.nullcontext()):
            out = _sample(tiny, kind, shape, cond, 4, trajectory=traj, **kw)
        torch.cuda.synchronize()
        return {"z0": out, "trajectory": traj}

    PZ.run_scenario(f, name=f"tiny-sample[{kind},{launch}{',cfg' if kw else ''}{',rescale' if 'guidance_rescale' in kw else ''}]", modules=[tiny], ragged=True,
                    inside=PZ.reevaluate(f), no_reuse_fills=(NAN, BIG))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_tiny_generate_odd_volume(tiny, precision):
    """encode -> depth upsample -> DDIM -> decode on (1,1,3,24,40) -> 5 slices; 'fp32': the f32-MFMA programs (conv_f32, gn_*_f32,
    attn_*_f32) at the same odd shape."""
    v_in = formula_input((1, 1, 3, 24, 40), 16).clamp(-1, 1).to(DEV)

    def f():
        out = tiny.generate(v_in, "ddim", num_inference_steps=3, target_depth=5, noise_fn=_noise_fn, precision=precision)
        torch.cuda.synchronize()
        return out

    PZ.run_scenario(f, name=f"tiny-generate[{precision}]", modules=[tiny], ragged=True, inside=PZ.reevaluate(f),
                    no_reuse_fills=(NAN, BIG))


@pytest.fixture(scope="module")
def full_model(pkg):
    model = build_full_model(pkg, DEV)
    yield model
    model.invalidate_engine_cache()
    _free()


@pytest.mark.parametrize("kind,kw", [("ddim", {}), ("ddpm", {}), ("dpmpp_2m", {}), ("heun", {}),
                                     ("ddim", dict(guidance_scale=2.5, guidance_rescale=0.7)),
                                     ("dpmpp_2m", dict(guidance_scale=2.5))],
                         ids=["ddim", "ddpm", "dpmpp_2m", "heun", "ddim-cfg-rescale", "dpmpp_2m-cfg"])
def test_config1_sampling(full_model, kind, kw):
    """The production U-Net on the config-1 latent (1,8,48,48,48), 3 steps on the captured graph."""
    shape = (1, 8, 48, 48, 48)
    cond = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(DEV)

    def f():
        out = _sample(full_model, kind, shape, cond, 3, **kw)
        torch.cuda.synchronize()
        return out

    PZ.run_scenario(f, name=f"config1-sample[{kind}{',cfg' if kw else ''}{',rescale' if 'guidance_rescale' in kw else ''}]", modules=[full_model], inside=PZ.reevaluate(f),
                    no_reuse_fills=(NAN,) if kind == "ddim" and not kw else ())
    _free()


def test_config1_generate_eager_and_fp32(full_model):
    v_in = (torch.rand((1, 1, 8, 192, 192), generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    for tag, precision, eager in (("eager", None, True), ("fp32", "fp32", False)):
        def f():
            with (_eager() if eager else contextlib.nullcontext()):
                out = full_model.generate(v_in, "ddim", num_inference_steps=3, target_depth=48, noise_fn=_noise_fn,
                                          precision=precision)
            torch.cuda.synchronize()
            return out

        PZ.run_scenario(f, name=f"config1-generate[{tag}]", modules=[full_model], inside=PZ.reevaluate(f))
        _free()


def test_config2_generate(full_model):
    """512 x 512, 8 -> 48 slices: encode + DDIM-3 + decode, fills 0x00 and 0xFF."""
    v_in = (torch.rand((1, 1, 8, 512, 512), generator=torch.Generator().manual_seed(2)) * 2 - 1).to(DEV)

    def f():
        out = full_model.generate(v_in, "ddim", num_inference_steps=3, target_depth=48, noise_fn=_noise_fn)
        torch.cuda.synchronize()
        return out

    PZ.run_scenario(f, name="config2-generate[ddim]", modules=[full_model], fills=(0x00, NAN), inside=PZ.reevaluate(f))
    _free()


# ---------------------------------------------------------------------------------------------------------------------
# VAE encode / decode at production width
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dhw,ragged", [((3, 20, 36), True), ((8, 192, 192), False)], ids=["odd-small-plane", "192x192"])
def test_production_vae_encode_decode(pkg, dhw, ragged):
    vae = build_prod_vae(pkg, DEV)
    d, h, w = dhw
    v = (torch.rand((1, 1, d, h, w), generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)

    def f():
        z = vae.encode(v)
        out = vae.decode(z)
        torch.cuda.synchronize()
        return {"z": z, "decoded": out}

    PZ.run_scenario(f, name=f"prod-vae[{h}x{w}]", modules=[vae], ragged=ragged, inside=PZ.reevaluate(f),
                    no_reuse_fills=(NAN, BIG) if ragged else ())
    vae.invalidate_engine_cache()
    _free()


# ---------------------------------------------------------------------------------------------------------------------
# stitching
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_batch", [1, 3])
def test_stitching(tiny, window_batch):
    v_full = formula_input((1, 1, 6, 40, 24), 17).clamp(-1, 1).to(DEV)
    sampler = S.DDIMSampler(tiny.diffusion, tiny.unet)

    def f():
        torch.manual_seed(7)
        out = sampler.sample_with_stitching(v_full, tiny.vae, 3, patch_size=(4, 16, 16), target_patch_size=(4, 16, 16),
                                            stride=(2, 8, 8), device=DEV, progress=False, window_batch=window_batch)
        torch.cuda.synchronize()
        return out

    PZ.run_scenario(f, name=f"stitching[window_batch={window_batch}]", modules=[tiny], ragged=True, inside=PZ.reevaluate(f),
                    no_reuse_fills=(NAN,))


def test_blend_kernels():
    ctx = E.Ctx.get(torch.device(DEV))
    patch = formula_input((2, 1, 3, 4, 5), 3).to(DEV)
    wd, wh, ww = (S._axis_window(n).to(DEV) for n in (3, 4, 5))

    def f():
        acc = torch.zeros(2, 1, 5, 9, 7, device=DEV)
        ws = torch.zeros_like(acc)
        with ctx.scope():
            for (d0, h0, w0) in ((0, 0, 0), (2, 5, 2), (1, 3, 1)):
                ctx.lib.blend_accumulate(E._ptr(acc), E._ptr(ws), E._ptr(patch), E._ptr(wd), E._ptr(wh), E._ptr(ww), 2, 3, 4, 5,
                                         5, 9, 7, d0, h0, w0, ctx.sptr)
            ctx.lib.blend_normalize(E._ptr(acc), E._ptr(ws), acc.numel(), ctx.sptr)
        torch.cuda.synchronize()
        return {"acc": acc, "wsum": ws}

    PZ.run_scenario(f, name="blend-kernels", expect_programs=False)


# ---------------------------------------------------------------------------------------------------------------------
# training: loss and every gradient; then optimizer steps
# ---------------------------------------------------------------------------------------------------------------------
def _grads(module):
    return {k: p.grad for k, p in module.named_parameters() if p.grad is not None}


def test_training_step_latent4_three_levels_odd_patch(pkg):
    un = pkg.UNet3D(**MID_UNET)
    load_formula(un, 9)
    diff = pkg.GaussianDiffusion('cosine', 1000)
    un.to(DEV)
    diff.to(DEV)
    shape = (3, 4, 5, 12, 8)
    z0, cond, noise = (t.to(DEV) for t in (formula_input(shape, 31), formula_input(shape, 32), formula_noise(-1, shape)))
    t = torch.tensor([5, 400, 990], device=DEV)

    def f():
        for p in un.parameters():
            p.grad = None
        loss, _ = diff.training_loss(un, z0, cond, t=t, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
        g = _grads(un)
        assert len(g) == len(list(un.parameters()))
        return {"loss": loss.detach(), "grad": g}

    PZ.run_scenario(f, name="train[latent4,3 levels]", modules=[un], ragged=True, inside=PZ.reevaluate(f),
                    no_reuse_fills=(NAN, BIG))
    for p in un.parameters():
        p.grad = None


def test_training_microstep_config3(full_model):
    """B = 4 patches of 192x192, 8 -> 48 slices (test_gpu_fullsize.test_training_microstep_config3's inputs)."""
    B = 4
    g = torch.Generator().manual_seed(7)
    v_in = (torch.rand((B, 1, 8, 192, 192), generator=g) * 2 - 1).to(DEV)
    v_gt = (torch.rand((B, 1, 48, 192, 192), generator=g) * 2 - 1).to(DEV)
    t = torch.tensor([37, 412, 688, 951], device=DEV)
    noise = torch.randn((B, 8, 48, 48, 48), generator=torch.Generator().manual_seed(8)).to(DEV)

    def f():
        for p in full_model.parameters():
            p.grad = None
        loss, _ = full_model(v_in, v_gt, t=t, noise=noise)
        loss.backward()
        torch.cuda.synchronize()
        return {"loss": loss.detach(), "grad": _grads(full_model.unet)}

    PZ.run_scenario(f, name="config3-microstep", modules=[full_model], inside=PZ.reevaluate(f))
    for p in full_model.parameters():
        p.grad = None
    full_model.invalidate_engine_cache()
    _free()


def test_two_fused_optimizer_steps_with_ema_and_clipping(pkg):
    """forward, backward, FusedAdamW(ema=, max_grad_norm=).step() with the fast re-pack, twice, then the next forward."""
    v_in = formula_input((2, 1, 2, 16, 24), 16).clamp(-1, 1).to(DEV)
    v_gt = formula_input((2, 1, 5, 16, 24), 19).clamp(-1, 1).to(DEV)
    t, nz = torch.tensor([612, 77], device=DEV), formula_noise(-1, (2, 8, 5, 4, 6)).to(DEV)

    def f(between=None):
        model, _, _ = tiny_model_sd(pkg)
        model.to(DEV)
        for p in model.vae.parameters():
            p.requires_grad_(False)
        ema = pkg.EMAWeights(model.unet, decay=0.9, prefix="unet.")
        opt = pkg.FusedAdamW(model.unet.parameters(), lr=2e-3, weight_decay=0.01, engine_modules=[model.unet], ema=ema,
                             max_grad_norm=1.0)
        losses = []
        for i in range(2):
            loss, _ = model(v_in, v_gt, t=t, noise=nz)
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            losses.append(loss.detach())
            if between is not None:
                between()
        nxt, _ = model(v_in, v_gt, t=t, noise=nz)
        torch.cuda.synchronize()
        ps = dict(model.unet.named_parameters())
        return {"losses": losses, "next_loss": nxt.detach(), "param": {k: p.detach() for k, p in ps.items()},
                "exp_avg": {k: opt.state[p]["exp_avg"] for k, p in ps.items()},
                "exp_avg_sq": {k: opt.state[p]["exp_avg_sq"] for k, p in ps.items()}, "ema": list(ema.shadows)}

    def inside(P, res, ref):
        def between():
            torch.cuda.synchronize()
            for prog in P.programs:
                if prog._colsum is not None:
                    P.repoison_scratch(prog)
        return PZ.diff_bits(PZ.snapshot(f(between)), ref)

    PZ.run_scenario(f, name="fused-adamw[ema,clip] x2", ragged=True, inside=inside, no_reuse_fills=(NAN, BIG))


# ---------------------------------------------------------------------------------------------------------------------
# VAE training with MSE + MS-SSIM
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,shape,ragged", [(16, (1, 1, 3, 40, 24), True), (128, (1, 1, 48, 192, 192), False),
                                               (128, (1, 1, 8, 192, 192), False)], ids=["tiny-odd", "thin", "thick"])
def test_vae_training_step_mse_plus_ms_ssim(pkg, base, shape, ragged):
    ms_ssim = importlib.import_module("models.losses").MS_SSIM_Loss()
    vae = pkg.VideoVAE(in_channels=1, latent_dim=8, base_channels=base, scaling_factor=1.0)
    load_formula(vae, 68)
    vae.train().to(DEV)
    x = formula_input(shape, 45).clamp(-1, 1).to(DEV)

    def f():
        for p in vae.parameters():
            p.grad = None
        recon, z = vae(x)
        loss = F.mse_loss(recon, x) + 0.5 * ms_ssim(recon, x)
        loss.backward()
        torch.cuda.synchronize()
        g = _grads(vae)
        assert len(g) == len(list(vae.parameters()))
        return {"loss": loss.detach(), "z": z.detach(), "recon": recon.detach(), "grad": g}

    PZ.run_scenario(f, name=f"vae-train[{shape[2]}x{shape[3]}x{shape[4]}]", modules=[vae], ragged=ragged, inside=PZ.reevaluate(f),
                    no_reuse_fills=(NAN, BIG) if ragged else ())
    for p in vae.parameters():
        p.grad = None
    vae.invalidate_engine_cache()
    _free()


# ---------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------
def test_video_metrics():
    from utils.metrics import calculate_video_metrics
    a = formula_input((1, 1, 6, 200, 168), 23).clamp(-1, 1)
    b = (a + 0.05 * formula_input((1, 1, 6, 200, 168), 24)).clamp(-1, 1)
    ad, bd = a[0].to(DEV), b[0].to(DEV)

    def f():
        vm = calculate_video_metrics(ad, bd, max_val=2.0)
        return {k: ([float(x) for x in v] if isinstance(v, (list, tuple)) else float(v)) for k, v in vm.items()}

    PZ.run_scenario(f, name="video-metrics", expect_programs=False)


# ---------------------------------------------------------------------------------------------------------------------
# depth sharding in lock-step on one device: the halo slices are the feature
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,shape,world", [(TINY_UNET, (1, 8, 6, 8, 8), 2), (MID_UNET, (1, 4, 12, 12, 8), 4),
                                            (TINY_UNET, (1, 8, 10, 8, 8), 3)], ids=["world2-3+3", "world4-3x4", "world3-4+3+3"])
def test_sharded_unet_steps(pkg, cfg, shape, world):
    """Two lock-step sampler steps on `world` depth slabs: the result must not depend on what a halo slice held before its
    exchange or its zero_end_halos."""
    un = pkg.UNet3D(**cfg)
    load_formula(un, 8)
    un.to(DEV)
    g = pkg.GaussianDiffusion()
    n, L, d, h, w = shape
    x, c = formula_input(shape, 10), formula_input(shape, 11)
    t_desc = [999, 500, 0]
    coef = S.ddim_coef_rows(g.alphas_cumprod, t_desc, 0.0)
    ctx = E.Ctx.get(torch.device(DEV))

    def f(between=None):
        with ctx.scope():
            comm = PAR.LocalComm(world)
            progs = []
            for r in range(world):
                spec = PAR.ShardSpec(r, world, comm, d)
                pr = E.UNetProgram(ctx, un, n, spec.depth_local, h, w, 8, shard=spec)
                pr.add_sampler_step("ddim", False)
                pr.load_latents(x, c)
                pr.set_schedule(t_desc, coef.to(DEV))
                progs.append(pr)
            PAR.run_lockstep(progs)
            eps = torch.cat([p.eps_ncdhw() for p in progs], dim=2)
            z1 = torch.cat([p.z_ncdhw() for p in progs], dim=2)
            if between is not None:
                between(progs)
            PAR.run_lockstep(progs)
            z2 = torch.cat([p.z_ncdhw() for p in progs], dim=2)
        torch.cuda.synchronize()
        return {"eps": eps, "z1": z1, "z2": z2}

    def inside(P, res, ref):
        def between(progs):
            torch.cuda.synchronize()
            for prog in progs:
                P.repoison_scratch(prog)
        return PZ.diff_bits(PZ.snapshot(f(between)), ref)

    PZ.run_scenario(f, name=f"sharded-unet[world {world}]", modules=[un], ragged=True, inside=inside, no_reuse_fills=(NAN, BIG))


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_vae_decode(pkg, world):
    """The decoder on depth slabs (3 + 3 and 3 + 2 + 2 slices of 7 / 6): ConvTranspose and 3x3x3 convs over exchanged halos."""
    vae = pkg.VideoVAE(in_channels=1, latent_dim=8, base_channels=16, scaling_factor=0.5)
    load_formula(vae, 10)
    vae.to(DEV)
    d = 6 if world == 2 else 7
    z = formula_input((1, 8, d, 4, 3), 33)
    ctx = E.Ctx.get(torch.device(DEV))

    def f():
        with ctx.scope():
            comm = PAR.LocalComm(world)
            progs = []
            for r in range(world):
                spec = PAR.ShardSpec(r, world, comm, d)
                pr = E.VAEDecodeProgram(ctx, vae, 1, spec.depth_local, 4, 3, shard=spec)
                pr.load(z)
                progs.append(pr)
            PAR.run_lockstep(progs)
            out = torch.cat([p.out for p in progs], dim=2).clone()
        torch.cuda.synchronize()
        return out

    PZ.run_scenario(f, name=f"sharded-vae-decode[world {world}]", modules=[vae], ragged=True, no_reuse_fills=(NAN, BIG))
