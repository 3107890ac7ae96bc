"""What the engine's program builders emit, as text two commits can be compared on.  For each of a fixed set of small
programs (formula weights from tests/helpers.py; every path a conv can take: single-GPU, guided, fp32 and bf16x3 on all
three column tiles, depth-sharded with and without the overlap split, the VAE legs, both training programs, the
differentiable decode, the VGG-19 and LPIPS losses) one line per op -- name, flops, kernel label, bytes, algorithmic bytes,
the audit record's kind and a digest of its key set -- then the program's totals, the packed-weight cache keys it added and a
SHA-256 of every output after an eager run (the U-Nets: again after capture() + two launch()es; the training programs: of
every weight image after repack() and after an in-place update + fast_repack(), and of every parameter gradient of a
backward).  The long uniform lists (op lines other than the launches of an overlapped conv, cache keys, weight images,
gradients) are folded into one digest line each; --full prints them line by line, to find what a digest that differs hides.

    python tools/program_fingerprint.py [--full] > out.txt           # on a ROCm device
    python tools/program_fingerprint.py --compare a1.txt a2.txt b.txt
        a1 / a2: two runs of the parent commit, b: the new commit.  Lines a1 and a2 disagree on are named and left out;
        the rest must be identical.  Exit status 1 on any difference."""
import gc
import hashlib
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.helpers import MID_UNET, TINY_UNET, formula_input, load_formula  # noqa: E402

DEV = "cuda:0"
T_DESC = [999, 500, 0]
FULL = "--full" in sys.argv
OVERLAPPED = ("interior", "lower", "upper")     # name suffixes of the three launches of an overlapped conv
_folded = {}                                    # label -> [lines, sha256 of them]


def fold(label, line):
    """One line of a long uniform list: printed under --full, else folded into the digest line of `label` (unfold)."""
    if FULL:
        print(line)
        return
    ent = _folded.setdefault(label, [0, hashlib.sha256()])
    ent[0] += 1
    ent[1].update((line + "\n").encode())


def unfold():
    for label, (n, h) in _folded.items():
        print(f"{label} {n} lines sha256 {h.hexdigest()[:32]}")
    _folded.clear()


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def describe(tag, prog):
    """The static half: what the builder emitted."""
    print(f"{tag} ops {len(prog.ops)}")
    for i, (meta, nb, alg, aud) in enumerate(zip(prog.op_meta, prog.op_bytes, prog.op_alg_bytes, prog.op_audit)):
        keys = "-" if aud is None else aud["kind"] + ":" + hashlib.sha256(",".join(sorted(aud)).encode()).hexdigest()[:8]
        line = f"{tag} op {i} {meta[0]} {meta[1]!r} {meta[2] or '-'} bytes {nb!r} alg {alg!r} audit {keys}"
        if meta[0].rsplit(".", 1)[-1] in OVERLAPPED:
            print(line)
        else:
            fold(f"{tag} op-lines", line)
    print(f"{tag} flops {prog.flops!r} pool {prog.pool.total_bytes} pack_stats {sorted(prog.pack_stats.items())}")
    print(f"{tag} conv_flops {hashlib.sha256(repr(prog.conv_flops).encode()).hexdigest()[:32]} n {len(prog.conv_flops)}")
    print(f"{tag} pack_meta {len(prog._pack_meta)}")


def packed_keys(E):
    return set(E._PACKED.get(torch.device(DEV).index, {}).keys())


def main():
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    EF = importlib.import_module("video-to-video-diffusion_amd.engine_f32")
    EX = importlib.import_module("video-to-video-diffusion_amd.engine_x3")
    P = importlib.import_module("video-to-video-diffusion_amd.parallel")
    S = importlib.import_module("video-to-video-diffusion_amd.sampler")
    T = importlib.import_module("video-to-video-diffusion_amd.train_engine")
    V = importlib.import_module("video-to-video-diffusion_amd.vae_train_engine")
    ctx = E.Ctx.get(torch.device(DEV))
    diff = pkg.GaussianDiffusion("cosine", 1000).to(DEV)
    coef = S.ddim_coef_rows(diff.alphas_cumprod, T_DESC, 0.0).to(DEV)

    def section(tag, build, run):
        """build() -> programs (alive together); run(progs) -> [(name, tensor)]."""
        gc.collect()
        before = packed_keys(E)
        with ctx.scope():
            progs = build()
            for r, pr in enumerate(progs):
                describe(f"{tag}[{r}]", pr)
            for k in sorted(repr(k) for k in packed_keys(E) - before):
                fold(f"{tag} packed", f"{tag} packed {k}")
            unfold()
            for name, t in run(progs):
                if ".image" in name:
                    fold(f"{tag} sha {name.split('.image')[0]}.images", f"{tag} sha {name} {sha(t)}")
                else:
                    unfold()
                    print(f"{tag} sha {name} {sha(t)}")
            unfold()
            for pr in progs:
                pr.check_errors()
        torch.cuda.synchronize()

    # ---- U-Net step programs -----------------------------------------------------------------------------------------
    def unet(cfg):
        un = pkg.UNet3D(**cfg)
        load_formula(un, 8)
        return un.to(DEV)

    def unet_section(tag, cfg, shape, cls=E.UNetProgram, guided=False, shard=None):
        un = unet(cfg)
        n, L, d, h, w = shape
        x, c = formula_input(shape, 10), formula_input(shape, 11)

        def build():
            kw = dict(guided=True, rescale=True) if guided else {}
            pr = cls(ctx, un, n, d, h, w, 8, shard=shard() if shard else None, **kw)
            pr.add_sampler_step("ddim", False)
            pr.load_latents(x, c)
            pr.set_schedule([t for t in T_DESC for _ in range(2 if guided else 1)], coef)
            if guided:
                pr.set_guidance(3.0, 0.7)
            return [pr]

        def run(progs):
            pr = progs[0]
            pr.run()
            yield "eager.eps", pr.eps_ncdhw()
            yield "eager.z", pr.z_ncdhw()
            pr.capture()
            pr.launch()
            pr.launch()
            yield "graph.eps", pr.eps_ncdhw()
            yield "graph.z", pr.z_ncdhw()

        section(tag, build, run)

    unet_section("unet.tiny", TINY_UNET, (1, 8, 4, 8, 8))
    unet_section("unet.mid", MID_UNET, (1, 4, 8, 12, 8))
    unet_section("unet.tiny.f32", TINY_UNET, (1, 8, 4, 8, 8), cls=EF.UNetProgramF32)
    unet_section("unet.tiny.x3", TINY_UNET, (1, 8, 4, 8, 8), cls=EX.UNetProgramX3)
    # MID_UNET's third level has 128 channels: the 128x128 tile, column sums included, which TINY_UNET never reaches
    unet_section("unet.mid.f32", MID_UNET, (1, 4, 8, 12, 8), cls=EF.UNetProgramF32)
    unet_section("unet.mid.x3", MID_UNET, (1, 4, 8, 12, 8), cls=EX.UNetProgramX3)
    unet_section("unet.tiny.guided", TINY_UNET, (1, 8, 4, 8, 8), guided=True)
    comm1 = P.RcclComm.single(with_rccl=True)      # one rank, overlap forced: fork / join inside the capture too
    unet_section("unet.tiny.force1", TINY_UNET, (1, 8, 4, 8, 8), shard=lambda: P.ShardSpec(0, 1, comm1, 4, overlap="force"))

    def sharded_unet():        # world 3 over depth 10: ragged slabs 4 + 3 + 3, overlap split on
        un = unet(TINY_UNET)
        shape, world = (1, 8, 10, 8, 8), 3
        x, c = formula_input(shape, 10), formula_input(shape, 11)

        def build():
            comm, progs = P.LocalComm(world), []
            for r in range(world):
                spec = P.ShardSpec(r, world, comm, shape[2])
                pr = E.UNetProgram(ctx, un, 1, spec.depth_local, 8, 8, 8, shard=spec)
                pr.add_sampler_step("ddim", False)
                pr.load_latents(x, c)
                pr.set_schedule(T_DESC, coef)
                progs.append(pr)
            return progs

        def run(progs):
            for it in range(2):
                P.run_lockstep(progs)
                yield f"step{it}.eps", torch.cat([p.eps_ncdhw() for p in progs], dim=2)
                yield f"step{it}.z", torch.cat([p.z_ncdhw() for p in progs], dim=2)

        section("unet.tiny.world3", build, run)

    sharded_unet()

    # ---- VAE -----------------------------------------------------------------------------------------------------------
    vae = pkg.VideoVAE(in_channels=1, latent_dim=8, base_channels=16, scaling_factor=0.5)
    load_formula(vae, 10)
    vae.to(DEV)
    vid, lat = formula_input((1, 1, 3, 16, 12), 16).clamp(-1, 1), formula_input((1, 8, 3, 4, 3), 17)
    for prec, enc, dec in (("bf16", E.VAEEncodeProgram, E.VAEDecodeProgram),
                           ("f32", EF.VAEEncodeProgramF32, EF.VAEDecodeProgramF32),
                           ("x3", EX.VAEEncodeProgramX3, EX.VAEDecodeProgramX3)):
        section(f"vae.enc.{prec}", lambda: [enc(ctx, vae, 1, 3, 16, 12)], lambda ps: [("out", ps[0](vid))])
        section(f"vae.dec.{prec}", lambda: [dec(ctx, vae, 1, 3, 4, 3)], lambda ps: [("out", ps[0](lat))])
    lat6 = torch.cat([lat, lat.flip(2)], dim=2)

    def build_dec2():
        comm, progs = P.LocalComm(2), []
        for r in range(2):
            pr = E.VAEDecodeProgram(ctx, vae, 1, 3, 4, 3, shard=P.ShardSpec(r, 2, comm, 6))
            pr.load(lat6)
            progs.append(pr)
        return progs

    def run_dec2(progs):
        P.run_lockstep(progs)
        return [("out", torch.cat([p.out for p in progs], dim=2))]

    section("vae.dec.world2", build_dec2, run_dec2)

    # ---- training programs: private weight images, the generic and the fast re-pack -----------------------------------------
    def train_run(pr, params, fwd, bwd):
        """`bwd()` -> the parameter gradients of the latest forward, in `params` order."""
        yield from fwd()
        pr.repack()
        for i, ent in enumerate(pr._pack_meta):
            yield f"repack.image{i}", ent["holder"][0]
        with torch.no_grad():
            for p in params:
                p.mul_(0.75)
        pr.fast_repack()
        print(f"fast tables: packs {len(pr._fast['packs'])} slow {len(pr._fast['slow'])} segments {pr._fast['nseg']}")
        for i, ent in enumerate(pr._pack_meta):
            yield f"fast_repack.image{i}", ent["holder"][0]
        yield from fwd()
        for i, g in enumerate(bwd()):
            yield f"grad.image{i}", g

    un = unet(TINY_UNET)
    shape = (1, 8, 4, 8, 8)
    z0, cond, noise = (formula_input(shape, s).to(DEV) for s in (20, 21, 22))
    t = torch.tensor([612], device=DEV)
    norm = torch.tensor([1.0 / z0.numel()], device=DEV)

    def build_ut():
        pr = T.UNetTrainProgram(ctx, un, 1, 4, 8, 8)
        pr.set_diffusion(diff)
        return [pr]

    section("train.unet", build_ut, lambda ps: train_run(
        ps[0], list(un.parameters()), lambda: [("loss", ps[0].run_forward(z0, cond, t, noise, norm))],
        lambda: ps[0].run_backward(torch.ones(1, device=DEV))))
    vae.train()
    xv = formula_input((1, 1, 3, 16, 12), 18).clamp(-1, 1).to(DEV)
    g_recon, g_lat = formula_input((1, 1, 3, 16, 12), 23).to(DEV), formula_input((1, 8, 3, 4, 3), 24).to(DEV)
    section("train.vae", lambda: [V.VAETrainProgram(ctx, vae, 1, 3, 16, 12)], lambda ps: train_run(
        ps[0], list(vae.parameters()), lambda: list(zip(("recon", "z"), ps[0].run_forward(xv))),
        lambda: ps[0].run_backward(g_recon, g_lat)))

    # ---- the differentiable decode: the decoder half of train.vae, data gradients only ----------------------------------
    def run_decgrad(ps):
        yield "recon", ps[0].run_forward(lat.to(DEV))
        yield "g_z", ps[0].run_backward(g_recon)

    section("train.decgrad", lambda: [V.VAEDecodeGradProgram(ctx, vae, 1, 3, 4, 3)], run_decgrad)

    # ---- the feature losses, through their modules (the program comes out of the module's pool after the call) ----------
    LS = importlib.import_module("video-to-video-diffusion_amd.losses")
    from tests.lpips_restatement import he_state_dict as he_vgg16  # noqa: E402
    from tests.vgg_restatement import he_state_dict as he_vgg19  # noqa: E402

    def loss_section(tag, module, shape, n_img, outputs):
        """outputs(module, out) -> [(name, tensor)] besides the input gradient."""
        module.to(DEV)
        a = formula_input(shape, 30).clamp(-1, 1).to(DEV).requires_grad_(True)
        b = formula_input(shape, 31).clamp(-1, 1).to(DEV)
        res = []

        def build():
            out = module(a, b)
            out.sum().backward()
            res.extend(outputs(module, out.detach()) + [("grad", a.grad)])
            return [module._take_program(ctx, n_img, *shape[-2:])]

        def run(ps):
            module._give_program(ps[0])
            return res

        section(tag, build, run)

    loss_section("loss.vgg19", LS.VGGPerceptualLoss(feature_layers=[2, 7], slice_sample_rate=1.0, weights=he_vgg19(40, upto=7)),
                 (1, 1, 2, 16, 16), 2, lambda m, out: [("loss", out), ("layer_means", m.last_layer_means)])
    loss_section("loss.lpips", LS.LPIPS(weights=he_vgg16(41), lpips=False), (2, 3, 16, 16), 2,
                 lambda m, out: [("values", out), ("layer_means", m.last_layer_means)])


def compare(a1, a2, b):
    """See the module docstring."""
    la1, la2, lb = ([ln.rstrip("\n") for ln in open(p)] for p in (a1, a2, b))
    if not len(la1) == len(la2) == len(lb):
        print(f"line counts differ: {len(la1)} / {len(la2)} / {len(lb)}")
        return 1
    bad = 0
    for x1, x2, y in zip(la1, la2, lb):
        if x1 != x2:
            print(f"not reproduced by the parent, left out:\n  {x1}\n  {x2}")
        elif x1 != y:
            bad += 1
            print(f"- {x1}\n+ {y}")
    print(f"{len(la1)} lines compared, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:]))
    main()
