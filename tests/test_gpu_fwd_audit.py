"""GPU: every forward launch of the programs against a float64 reference computed from that launch's own operands.

The unit tests (test_gpu_ops.py, test_gpu_fullsize.py) bound a conv by rel-L2 <= 3e-3 and max |d| <= 2e-2 max |ref|, the network
tests by rel-L2 <= 3e-2 against the fp32 oracle; one 8-channel chunk of one tap lost in one 512-voxel tile of a config-2 layer
(~1e-4 rel-L2) passes both (tests/test_host_fwd_audit.py shows it on the CPU).  Here each forward op of a program runs on its own,
with copies of exactly the operands it read (tests/fwd_audit.py), so the bound is the arithmetic of the launch itself: one bf16
ulp per bf16 output element, F32_REL_L2 / F32_MAX_REL for fp32 accumulations, 2 k 2^-24 sum|terms| for fp32 elementwise launches,
bit for bit for copies and casts -- each with its derivation in tests/fwd_audit.py.  The launches with fused epilogues (GroupNorm
column sums, the res1x1+gn tail, normalise-then-conv, the tanh / strided fp32 heads, the stem, the streaming tail) are met at
their real shapes with the operands they see inside a program: in-place outputs, padded channels, strided fp32 outputs.

Every forward op must carry a record (or be on fwd_audit.SKIP: launches that compute nothing), so a launch added later cannot go
unchecked.  The programs:
  * UNetProgram, production U-Net, at the benchmarked config-2 latent (1, 8, 48, 128, 128), with the DDIM update appended;
  * every SAMPLER_STEPS kind, with and without noise, on a small U-Net's program: the update launches alone, row after row of a
    real coefficient table (Heun: predictor, corrector with churn noise, final row), the last row with NaN / Inf in eps;
  * a guided (batch 2n, rescale on) program at the config-1 patch latent (1, 8, 48, 48, 48);
  * the two small U-Nets of the backward audit (exact attention; latent 4 padded to 8 channels, odd coarse planes, a 6x6
    level), with CTSI_NO_FUSE_RES on and off: both ResBlock tail forms;
  * the base-128 VAE encoder / decoder at 48 x 192 x 192 and at 8 x 512 x 512 (float64 convs in depth slabs);
  * the fp32 engine's U-Net at the config-1 patch latent;
  * the forward halves of the config-3 U-Net training program and of the VAE training program (thin and thick patches);
  * outputs of programs built with records equal, bit for bit, those of programs built with the records stripped.
Depth-sharded programs are out of scope (their Acts carry halos; fwd_audit.act_ndhwc refuses them)."""
import gc
import importlib
import time

import pytest
import torch

from tests import fwd_audit as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
E = importlib.import_module("video-to-video-diffusion_amd.engine")
E32 = importlib.import_module("video-to-video-diffusion_amd.engine_f32")
S = importlib.import_module("video-to-video-diffusion_amd.sampler")
T = importlib.import_module("video-to-video-diffusion_amd.train_engine")
V = importlib.import_module("video-to-video-diffusion_amd.vae_train_engine")

SMALL = dict(
    b1_6x6=dict(kw=dict(latent_dim=8, model_channels=32, num_res_blocks=1, attention_levels=[1, 2], channel_mult=(1, 2, 4),
                        num_heads=4, time_embed_dim=64), shape=(1, 5, 24, 24), seed=3),
    latent4_three_levels=dict(kw=dict(latent_dim=4, model_channels=32, num_res_blocks=2, attention_levels=[1, 2],
                                      channel_mult=(1, 2, 4), num_heads=8, time_embed_dim=128), shape=(3, 5, 12, 8), seed=9),
)


def _free():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _report(title, rows, missing, t0):
    print()
    print(A.format_table(title, rows))
    print(f"wall time of this case: {time.time() - t0:.1f} s")
    bad = [r for r in rows if not r["ok"]]
    assert not missing, f"forward ops without an audit record: {sorted(set(missing))}"
    assert rows, "no forward op was audited"
    assert not bad, "%d audited outputs out of bounds, first: %s" % (len(bad), bad[:3])


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _unet_program(pkg, unet, n, d, h, w, *, kind="ddim", eta=0.0, cls=None, guided=False, rescale=False, mode="fast", seed=0,
                  steps=4, churn=0.0):
    """A sampler program with its inputs loaded and a real coefficient table: returns (prog, evaluations)."""
    diff = pkg.GaussianDiffusion("cosine", 1000)
    ac = diff.alphas_cumprod
    t_desc = [int(v) for v in torch.linspace(999, 0, steps).round().tolist()]
    with_noise = kind == "ddpm" or (kind == "ddim" and eta > 0) or (kind == "heun" and churn > 0)
    if kind == "ddim":
        coef, t_rows = S.ddim_coef_rows(ac, t_desc, eta), t_desc
    elif kind == "ddpm":
        coef, t_rows = diff.ddpm_coef_rows(t_desc), t_desc
    elif kind == "dpmpp":
        coef, t_rows = S.dpm_coef_rows(ac, t_desc, 2), t_desc
    else:
        sig = S.karras_sigmas(steps, float(S.sigma_table(ac)[10]), float(S.sigma_table(ac)[-20]))
        hr = S.heun_coef_rows(ac, sig, order=2, s_churn=churn)
        coef, t_rows = hr.rows, [float(v) for v in hr.t]
    evals = len(t_rows)
    nb = 2 * n if guided else n
    ctx = E.Ctx.get(DEV)
    with ctx.scope():
        prog = (cls or E.UNetProgram)(ctx, unet, n, d, h, w, (evals + 1) * nb, mode, guided=guided, rescale=rescale)
        prog.add_sampler_step(kind, with_noise)
        L = unet.latent_dim
        prog.load_latents(_randn((n, L, d, h, w), seed + 1), _randn((n, L, d, h, w), seed + 2))
        prog.set_schedule([t for t in t_rows for _ in range(nb)], coef.to(DEV))
        if guided:
            prog.set_guidance(3.0, 0.7 if rescale else 0.0)
        if with_noise:
            prog.noise.copy_(_randn(tuple(prog.noise.shape), seed + 3))
    return prog, evals


# ---- U-Net programs -------------------------------------------------------------------------------------------------------
def test_unet_config2_forward_audit(pkg):
    """The production U-Net (UNet3D(latent_dim=8), default init, seed 0) at the benchmarked latent, DDIM update appended."""
    t0 = time.time()
    torch.manual_seed(0)
    un = pkg.UNet3D(latent_dim=8).to(DEV).eval()
    prog, _ = _unet_program(pkg, un, 1, 48, 128, 128)
    rows, missing = A.audit_forward(prog)
    del prog
    _free()
    _report("U-Net config 2 (1, 8, 48, 128, 128) + ddim: forward ops against float64 from their own operands", rows, missing, t0)


def test_unet_guided_config1_forward_audit(pkg):
    """Batch 2n, guidance scale 3, rescale 0.7, at the config-1 patch latent: cfg.stats / stats_finalize / combine / mirror."""
    t0 = time.time()
    torch.manual_seed(0)
    un = pkg.UNet3D(latent_dim=8).to(DEV).eval()
    prog, _ = _unet_program(pkg, un, 1, 48, 48, 48, guided=True, rescale=True, seed=20)
    rows, missing = A.audit_forward(prog)
    kinds = {r["name"] for r in rows}
    del prog
    _free()
    assert {"cfg.stats", "cfg.stats_finalize", "cfg.combine", "cfg.mirror"} <= kinds
    _report("guided U-Net (2 x 1, 8, 48, 48, 48), rescale on + ddim: forward ops against float64", rows, missing, t0)


@pytest.mark.parametrize("fuse", ["fused_tail", "CTSI_NO_FUSE_RES"])
@pytest.mark.parametrize("case", sorted(SMALL))
def test_unet_small_forward_audit(pkg, monkeypatch, case, fuse):
    """The shape families of the backward audit; `b1_6x6` runs the exact attention (softmax row sums, gn_apply of the block's
    input, the q / k conv), `latent4_three_levels` the latent padded to 8 channels and the odd coarse planes."""
    t0 = time.time()
    if fuse == "CTSI_NO_FUSE_RES":
        monkeypatch.setenv("CTSI_NO_FUSE_RES", "1")
    else:
        monkeypatch.delenv("CTSI_NO_FUSE_RES", raising=False)
    c = SMALL[case]
    torch.manual_seed(c["seed"])
    un = pkg.UNet3D(**c["kw"]).to(DEV).eval()
    mode = "exact" if case == "b1_6x6" else "fast"
    prog, _ = _unet_program(pkg, un, *c["shape"], mode=mode, kind="dpmpp", seed=c["seed"])
    rows, missing = A.audit_forward(prog)
    names = {r["name"] for r in rows}
    del prog
    _free()
    assert ("res1x1" in names) == (fuse == "CTSI_NO_FUSE_RES") and ("res1x1+gn" in names) == (fuse == "fused_tail")
    assert (mode == "exact") == ("attn.softmax_rowsum" in names)
    _report(f"U-Net {case} ({fuse}, attention {mode}) + dpmpp: forward ops against float64", rows, missing, t0)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("kind,eta,churn", [("ddim", 0.0, 0.0), ("ddim", 0.5, 0.0), ("ddpm", 0.0, 0.0), ("dpmpp", 0.0, 0.0),
                                            ("heun", 0.0, 0.0), ("heun", 0.0, 40.0)])
def test_sampler_step_audit(pkg, kind, eta, churn, precision):
    """Every update kind, with and without noise, bf16 and fp32 network input: the U-Net runs unaudited, then the launches
    behind it (update, step counter; guided: combine and mirror too) are audited, evaluation after evaluation of a real
    coefficient table.  The last evaluation meets NaN, +Inf and -Inf in eps (kinds that count them)."""
    t0 = time.time()
    c = SMALL["b1_6x6"]
    torch.manual_seed(c["seed"])
    un = pkg.UNet3D(**c["kw"]).to(DEV).eval()
    guided = kind == "ddpm"           # one kind also runs behind the guidance launches (not one that meets NaN: the statistics)
    cls = E32.UNetProgramF32 if precision == "fp32" else E.UNetProgram
    prog, evals = _unet_program(pkg, un, *c["shape"], kind=kind, eta=eta, churn=churn, cls=cls, guided=guided, rescale=guided,
                                seed=30)
    tail = range(prog.unet_op_count, len(prog.ops))
    rows, missing = [], []
    for ev in range(evals):
        with prog.ctx.scope():
            for op in prog.ops[:prog.unet_op_count]:
                op()
            if ev == evals - 1 and E.SAMPLER_STEPS[kind].nonfinite:
                flat = prog.eps.view(-1)
                flat[5], flat[77], flat[1001] = float("nan"), float("inf"), float("-inf")
        r, missing = A.audit_forward(prog, only=tail)
        assert int(prog.step_ptr[0]) == ev + 1
        rows += r
    if E.SAMPLER_STEPS[kind].nonfinite:
        assert int(prog.nonfinite[evals - 1].sum()) >= 3      # the three poked values were counted (and checked exactly)
    del prog
    _free()
    assert sum(r["name"] == "sampler.step" and r["what"] == "z" for r in rows) == evals
    _report(f"sampler update {kind} (eta {eta}, churn {churn}, {precision}{', guided' if guided else ''}): {evals} evaluations",
            rows, missing, t0)


def test_unet_f32_config1_forward_audit(pkg):
    """The fp32 engine's U-Net (f32 MFMA convs, fp32 activations) at the config-1 patch latent, DDIM update appended."""
    t0 = time.time()
    torch.manual_seed(0)
    un = pkg.UNet3D(latent_dim=8).to(DEV).eval()
    prog, _ = _unet_program(pkg, un, 1, 48, 48, 48, cls=E32.UNetProgramF32, seed=40)
    rows, missing = A.audit_forward(prog)
    del prog
    _free()
    _report("fp32 U-Net (1, 8, 48, 48, 48) + ddim: forward ops against float64", rows, missing, t0)


# ---- VAE programs ---------------------------------------------------------------------------------------------------------
def _vae(pkg, seed=0):
    torch.manual_seed(seed)
    return pkg.VideoVAE(in_channels=1, latent_dim=16, base_channels=128, scaling_factor=0.5).to(DEV).eval()


@pytest.mark.parametrize("d,hw", [(48, 192), (8, 512)])
@pytest.mark.parametrize("leg", ["encode", "decode"])
def test_vae_forward_audit(pkg, leg, d, hw):
    """Base-128 VAE legs at the patch size and at full slices (depth 8: the thin patch; 4096 tiles per sample, tensors beyond
    the 512 MB non-temporal threshold of ctsi_gn_apply): the stem, the strided and transposed convs with nclass = 4 column
    sums, the in-place normalise-then-conv, the fp32-strided quant conv and the tanh head."""
    t0 = time.time()
    vae = _vae(pkg)
    ctx = E.Ctx.get(DEV)
    with ctx.scope():
        if leg == "encode":
            prog = E.VAEEncodeProgram(ctx, vae, 1, d, hw, hw)
            prog((torch.rand((1, 1, d, hw, hw), generator=torch.Generator().manual_seed(d)) * 2 - 1).to(DEV))
        else:
            prog = E.VAEDecodeProgram(ctx, vae, 1, d, hw // 4, hw // 4)
            prog(_randn((1, 16, d, hw // 4, hw // 4), d + 1))
    rows, missing = A.audit_forward(prog)
    del prog
    _free()
    _report(f"VAE {leg} base 128, slices {d} x {hw} x {hw}: forward ops against float64", rows, missing, t0)


# ---- forward halves of the training programs ----------------------------------------------------------------------------------
def test_unet_train_config3_forward_audit(pkg):
    """ops[:n_fwd] of the config-3 training program (batch 4, latent 48^3): train.inputs, the unfused ResBlock tails, the
    two-conv attention middle, loss.fwd."""
    t0 = time.time()
    torch.manual_seed(0)
    un = pkg.UNet3D(latent_dim=8).to(DEV)
    diff = pkg.GaussianDiffusion("cosine", 1000).to(DEV)
    n, L, d, h, w = 4, 8, 48, 48, 48
    g = torch.Generator().manual_seed(1)
    z0, cond, noise = (torch.randn((n, L, d, h, w), generator=g).to(DEV) for _ in range(3))
    t = torch.randint(0, 1000, (n,), generator=g).to(DEV)
    acp = diff.alphas_cumprod[t]
    snr = acp / (1 - acp + 1e-8)
    norm = (snr.clamp(max=5.0) / (snr + 1e-8)) / float(n * L * d * h * w)
    mask = (torch.rand((n, L, d), generator=g) > 0.3).float().to(DEV)
    ctx = E.Ctx.get(DEV)
    with ctx.scope():
        prog = T.UNetTrainProgram(ctx, un, n, d, h, w)
        prog.set_diffusion(diff)
        prog.run_forward(z0, cond, t, noise, norm, mask)
    rows, missing = A.audit_forward(prog, stop=prog.n_fwd)
    names = {r["name"] for r in rows}
    del prog
    _free()
    assert {"train.inputs", "loss.fwd"} <= names
    _report("U-Net training program config 3 (4, 8, 48, 48, 48): forward half against float64", rows, missing, t0)


@pytest.mark.parametrize("depth", [48, 8])
def test_vae_train_forward_audit(pkg, depth):
    """ops[:n_fwd] of the VAE training program at the thick and thin patches (1, 1, depth, 192, 192): encoder, quant conv,
    the seam cast, decoder."""
    t0 = time.time()
    torch.manual_seed(0)
    vae = pkg.VideoVAE(in_channels=1, latent_dim=16, base_channels=128, scaling_factor=1.0 if depth == 48 else 0.5).train().to(DEV)
    x = (torch.rand((1, 1, depth, 192, 192), generator=torch.Generator().manual_seed(depth)) * 2 - 1).to(DEV)
    ctx = E.Ctx.get(DEV)
    with ctx.scope():
        prog = V.VAETrainProgram(ctx, vae, 1, depth, 192, 192)
        prog.run_forward(x)
    rows, missing = A.audit_forward(prog, stop=prog.n_fwd)
    names = {r["name"] for r in rows}
    del prog
    _free()
    assert "seam.z_to_bf16" in names
    _report(f"VAE training program (1, 1, {depth}, 192, 192): forward half against float64", rows, missing, t0)


# ---- the audit sees one wrong element and one lost tile, at the launch that made them ------------------------------------------------
def test_audit_flags_a_wrong_element_and_a_lost_colsum_tile(pkg):
    """A conv launch of a small program is wrapped so that, after the kernel, ONE output element sits 2^-6 of its value (2 - 4
    bf16 ulps) off and ONE tile's column sums are gone.  The audit must refuse exactly that launch's output and column sums --
    and nothing downstream: every later launch is judged on the operands it actually read."""
    c = SMALL["b1_6x6"]
    torch.manual_seed(c["seed"])
    un = pkg.UNet3D(**c["kw"]).to(DEV).eval()
    prog, _ = _unet_program(pkg, un, *c["shape"], seed=60)
    i = next(k for k, m in enumerate(prog.op_meta) if m[0] == "rb.conv2")
    rec, op = prog.op_audit[i], prog.ops[i]

    def slipped():
        op()
        y = A.act_ndhwc(rec["out"]).view(-1)
        j = int(y.float().abs().argmax())
        y[j] = (y[j].double() * (1.0 + 2.0 ** -6)).to(torch.bfloat16)
        cpad = rec["stats"]["cpad"]
        rec["colsum"]()[cpad:2 * cpad] = 0.0           # tile 1 of the sums; the slab of squares is left alone

    prog.ops[i] = slipped
    rows, missing = A.audit_forward(prog)
    failed = {(r["op"], r["what"]) for r in rows if not r["ok"]}
    del prog
    _free()
    assert not missing
    assert failed == {(i, "y"), (i, "colsum1")}, failed


# ---- records change nothing ---------------------------------------------------------------------------------------------------
def test_outputs_with_records_equal_outputs_without(pkg, monkeypatch):
    """Programs built with the records stripped at _emit (nothing keeps a record alive) give the same bits, the same op list
    and the same pool as programs built with them: U-Net + guided update, VAE decode, fp32 U-Net."""
    c = SMALL["latent4_three_levels"]
    torch.manual_seed(c["seed"])
    un = pkg.UNet3D(**c["kw"]).to(DEV).eval()
    vae = pkg.VideoVAE(in_channels=1, latent_dim=16, base_channels=32, scaling_factor=0.5).to(DEV).eval()
    zl = _randn((1, 16, 4, 12, 12), 7)

    def build_and_run():
        outs, shapes = [], []
        for cls in (E.UNetProgram, E32.UNetProgramF32):
            prog, evals = _unet_program(pkg, un, *c["shape"], kind="heun", churn=40.0, cls=cls, guided=True, rescale=True, seed=50)
            with prog.ctx.scope():
                for _ in range(evals):
                    prog.run()
                outs += [prog.z.clone(), prog.eps.clone(), prog.xin.t.clone(), prog.hist.clone(), prog._gn_sums.clone()]
            shapes.append((len(prog.ops), prog.pool.total_bytes, [m for m in prog.op_meta], sum(a is not None for a in prog.op_audit)))
            del prog
        ctx = E.Ctx.get(DEV)
        with ctx.scope():
            dec = E.VAEDecodeProgram(ctx, vae, 1, 4, 12, 12)
            outs.append(dec(zl))
        shapes.append((len(dec.ops), dec.pool.total_bytes, [m for m in dec.op_meta], sum(a is not None for a in dec.op_audit)))
        torch.cuda.synchronize()
        return outs, shapes

    with_rec, shp_rec = build_and_run()
    emit = E.Program._emit

    def emit_stripped(self, fn, name="op", flops=0.0, kernel="", nbytes=0.0, alg_bytes=0.0, audit=None):
        return emit(self, fn, name, flops, kernel, nbytes, alg_bytes, None)

    monkeypatch.setattr(E.Program, "_emit", emit_stripped)
    without, shp_none = build_and_run()
    monkeypatch.undo()
    _free()
    assert all(s[3] > 0 for s in shp_rec) and all(s[3] == 0 for s in shp_none)
    assert [s[:3] for s in shp_rec] == [s[:3] for s in shp_none]
    assert len(with_rec) == len(without)
    for a, b in zip(with_rec, without):
        assert A.cmp_same(a, b)["ok"]
