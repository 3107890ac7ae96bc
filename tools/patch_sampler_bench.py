"""What the device patch sampler costs, variants ALTERNATED in one process.

  1. the host path it replaces, restated here: torch.load of one ~370 MB patient file (thin (1,300,512,512) + thick
     (1,50,512,512) fp32) plus the crop, in 4 and in 16 worker processes; patches per second.  The file is written by this tool
     to a temporary directory and read back from the page cache, which flatters the host path.  Runs FIRST: the workers are
     started before this process opens the GPU.
  2. ctsi_patch_sample alone at B = 4 and B = 8, 48 / 8 x 192 x 192 out of a 300 x 512 x 512 volume, from fp16 and from fp32
     storage, k = 0 / 1 / 2 with the flips off and on; us per launch and TB/s of the bytes the formula moves (every thin
     slice read once, two thick slices per thick output slice, every output written once), beside ctsi_nan_to_num_f32 on the
     two output tensors (one read + one write of the same outputs: the project's streaming yardstick).
  3. a config-3 micro-step (B = 4) on a fixed resident batch -- bench.py --mode train -- against the same step fed by
     DevicePatchLoader, in alternating blocks; the difference beside the block-to-block spread of the fixed-batch step.
  4. the store's footprint per patient at both storage types.

    python tools/patch_sampler_bench.py >> profiles/patch_sampler_bench.log"""
import argparse
import importlib
import multiprocessing
import os
import random
import sys
import tempfile
import time

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import torch  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DT, DK, PS = 48, 8, 192
VOL = (300, 50, 512, 512)       # D_thin, D_thick, H, W


def host_item(args):
    """The reference's __getitem__ without the augmentation: load the whole patient file, cut one patch, drop the rest."""
    path, seed = args
    import torch.nn.functional as F
    rng = random.Random(seed)
    d = torch.load(path, weights_only=False)
    thick, thin = d["input"], d["target"]
    y0, x0, z = rng.randint(0, VOL[2] - PS), rng.randint(0, VOL[3] - PS), rng.randint(0, VOL[0] - DT)
    k0 = int(z * VOL[1] / VOL[0])
    k1 = min(VOL[1], max(int((z + DT) * VOL[1] / VOL[0]), k0 + 1))
    sub = thick[:, k0:k1, y0:y0 + PS, x0:x0 + PS]
    tk = F.interpolate(sub.unsqueeze(0), size=(DK, PS, PS), mode="trilinear", align_corners=False).squeeze(0)
    return float(tk.sum() + thin[:, z:z + DT, y0:y0 + PS, x0:x0 + PS].sum())


def host_path(thick, thin, items):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "case_000.pt")
        torch.save({"input": thick, "target": thin, "category": "c", "patient_id": "0"}, path)
        print(f"host path: one patient file of {os.path.getsize(path) / 1e6:.0f} MB, torch.load + crop per item, "
              f"{os.cpu_count()} CPUs visible, torch threads per worker 1")
        ctx = multiprocessing.get_context("spawn")
        for workers in (4, 16):
            with ctx.Pool(workers, initializer=torch.set_num_threads, initargs=(1,)) as pool:
                pool.map(host_item, [(path, -i) for i in range(workers)])            # start the workers, warm the page cache
                t0 = time.perf_counter()
                pool.map(host_item, [(path, i) for i in range(items)], chunksize=1)
                dt = time.perf_counter() - t0
            print(f"  {workers:2d} workers: {items} items in {dt:6.2f} s = {items / dt:6.1f} patches/s "
                  f"({items / dt * os.path.getsize(path) / 1e9:5.1f} GB/s unpickled)")


def alternate(variants, rounds, warmup, reps, stream):
    times = {name: [] for name, _ in variants}
    for rnd in range(warmup + rounds):
        for name, fn in variants:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
            if rnd >= warmup:
                times[name].append(e0.elapsed_time(e1) / reps)
    return times


def kernel_alone(DD, E, stores, vols, args):
    ctx = E.Ctx.get(torch.device(DEV))
    lib = ctx.lib
    variants, nbytes = [], {}
    keep = []
    for B in (4, 8):
        thin = torch.empty((B, 1, DT, PS, PS), dtype=torch.float32, device=DEV)
        thick = torch.empty((B, 1, DK, PS, PS), dtype=torch.float32, device=DEV)
        keep += [thin, thick]
        out_bytes = (thin.numel() + thick.numel()) * 4

        def yard(thin=thin, thick=thick):
            lib.nan_to_num_f32(E._ptr(thin), thin.numel(), ctx.sptr)
            lib.nan_to_num_f32(E._ptr(thick), thick.numel(), ctx.sptr)

        variants.append((f"B={B} nan_to_num on both outputs", yard))
        nbytes[variants[-1][0]] = 2 * out_bytes
        for sname, store in stores.items():
            es = 2 if sname == "fp16" else 4
            sampler = DD.DevicePatchSampler(store, DT, DK, (PS, PS), seed=B)
            base = sampler.draw([0] * B)
            for k in (0, 1, 2):
                for flips in (0, 3):
                    rows = base.clone()
                    rows[:, DD.C_FLAGS] = k << 2 | flips
                    sampler.check_rows(rows)
                    table = torch.empty((B, DD.TABLE_COLS), dtype=torch.int64)
                    table[:, 2:] = rows[:, 1:]
                    table[:, 0], table[:, 1] = store.thin[0].data_ptr(), store.thick[0].data_ptr()
                    table = table.to(DEV)
                    keep.append(table)

                    def fn(table=table, thin=thin, thick=thick, st=DD.STORAGE[store.dtype], B=B):
                        lib.patch_sample(E._ptr(table), B, st, DT, DK, PS, PS, E._ptr(thin), E._ptr(thick), ctx.sptr)

                    name = f"B={B} {sname} k={k} flips={'on ' if flips else 'off'}"
                    variants.append((name, fn))
                    nbytes[name] = B * (DT + 2 * DK) * PS * PS * es + out_bytes
    with ctx.scope():
        times = alternate(variants, args.rounds, args.warmup, args.reps, ctx.stream)
    print(f"ctsi_patch_sample alone, {DT}/{DK} x {PS} x {PS} out of {VOL[0]} x {VOL[2]} x {VOL[3]} (x0 drawn: rows mostly off the "
          f"16-byte grid); {args.rounds} rounds of {args.reps} launches, all variants alternated")
    for name, _ in variants:
        s = sorted(times[name])
        med = s[len(s) // 2]
        print(f"  ({name:34s}) min {1e3 * s[0]:8.1f} us  median {1e3 * med:8.1f} us  max {1e3 * s[-1]:8.1f} us   "
              f"{nbytes[name] / 1e6:7.1f} MB   {nbytes[name] / (med * 1e-3) / 1e12:6.3f} TB/s")


def micro_steps(pkg, DD, store, args):
    from bench import EFFECTIVE_CFG
    torch.manual_seed(0)
    model = pkg.VideoToVideoDiffusion(EFFECTIVE_CFG).eval().to(DEV)
    params = list(model.unet.parameters())
    for p in model.vae.parameters():
        p.requires_grad_(False)
    B = 4
    gen = torch.Generator(device="cpu").manual_seed(1)
    v_in = (torch.rand(B, 1, DK, PS, PS, generator=gen) * 2 - 1).to(DEV)
    v_gt = (torch.rand(B, 1, DT, PS, PS, generator=gen) * 2 - 1).to(DEV)
    loader = DD.DevicePatchLoader(DD.DevicePatchSampler(store, DT, DK, (PS, PS)), batch_size=B, patches_per_volume=4096)
    it = iter(loader)

    def step(batch):
        for p in params:
            p.grad = None
        loss, _ = model(batch["input"].to(DEV), batch["target"].to(DEV))
        loss.backward()
        return loss

    fixed = {"input": v_in, "target": v_gt}
    for _ in range(3):
        step(fixed)
        step(next(it))
    blocks = {"fixed": [], "loader": []}
    for _ in range(args.blocks):
        for name in ("fixed", "loader"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = step(fixed if name == "fixed" else next(it))
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    assert bool(torch.isfinite(loss))
    f, ld = blocks["fixed"], blocks["loader"]
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"config-3 micro-step (B = 4, {DK}/{DT} x {PS} x {PS}), {args.blocks} alternating blocks of {args.steps} steps, ms per step")
    print(f"  fixed resident batch : {' '.join(f'{x:7.2f}' for x in f)}   median {med(f):7.2f}  spread {max(f) - min(f):5.2f}")
    print(f"  fed by the loader    : {' '.join(f'{x:7.2f}' for x in ld)}   median {med(ld):7.2f}  spread {max(ld) - min(ld):5.2f}")
    print(f"  loader - fixed (medians): {med(ld) - med(f):+6.2f} ms = {100 * (med(ld) - med(f)) / med(f):+5.2f} %; block-to-block spread "
          f"of the fixed-batch step {max(f) - min(f):5.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-items", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--skip", default="", help="comma list of: host, kernel, step")
    args = ap.parse_args()
    skip = set(args.skip.split(",")) if args.skip else set()
    g = torch.Generator().manual_seed(0)
    thin = torch.rand((1, VOL[0], VOL[2], VOL[3]), generator=g) * 2 - 1
    thick = torch.rand((1, VOL[1], VOL[2], VOL[3]), generator=g) * 2 - 1
    if "host" not in skip:
        host_path(thick, thin, args.host_items)          # before the GPU is opened: worker processes are started here
    pkg = importlib.import_module("video-to-video-diffusion_amd")
    DD = importlib.import_module("video-to-video-diffusion_amd.device_data")
    E = importlib.import_module("video-to-video-diffusion_amd.engine")
    stores = {}
    for name, dtype in (("fp16", torch.float16), ("fp32", torch.float32)):
        stores[name] = DD.DeviceVolumeStore(DEV, dtype)
        stores[name].add(thick, thin, patient_id="0")
        print(f"store footprint per patient ({VOL[0]} thin + {VOL[1]} thick slices of {VOL[2]} x {VOL[3]}), {name}: "
              f"{stores[name].nbytes / 1e6:.1f} MB; 356 patients: {356 * stores[name].nbytes / 1e9:.1f} GB")
    if "kernel" not in skip:
        kernel_alone(DD, E, stores, [(thick, thin)], args)
    if "step" not in skip:
        stores["fp16"].add(thick, thin, patient_id="1")
        micro_steps(pkg, DD, stores["fp16"], args)


if __name__ == "__main__":
    main()
