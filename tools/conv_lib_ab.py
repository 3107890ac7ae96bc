"""Two builds of libctsi.so on single layers of the fp32 and bf16x3 convolutions, in ONE process: every column tile (128x32,
128x64, 128x128), with and without the column-sum epilogue, and the VAE's two thin layers at their real size.  Per layer:
outputs and column-sum slabs of the two libraries compared bit for bit, then blocks of launches between two events,
library A / library B alternating, min and max of the per-launch time over the rounds.

    python tools/conv_lib_ab.py A=path/to/libctsi.so B=path/to/other/libctsi.so"""
import ctypes as C
import importlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
L = importlib.import_module("video-to-video-diffusion_amd.lib")
DEV = "cuda:0"

# name: (c1, cout, dims, k, p, act, ncdhw_out, colsum, launches per block)
CASES = {
    "post_quant 1x1x1 8->8 @48x128x128": (8, 8, (48, 128, 128), (1, 1, 1), (0, 0, 0), 0, False, False, 200),
    "k333 32->32 +colsum @48x64x64": (32, 32, (48, 64, 64), (3, 3, 3), (1, 1, 1), 0, False, True, 20),
    "head k333 128->1 tanh strided @48x512x512": (128, 1, (48, 512, 512), (3, 3, 3), (1, 1, 1), 1, True, False, 3),
    "k333 64->64 +colsum @48x64x64 (128x64 tile)": (64, 64, (48, 64, 64), (3, 3, 3), (1, 1, 1), 0, False, True, 10),
    "k333 128->128 +colsum @48x64x64 (128x128 tile)": (128, 128, (48, 64, 64), (3, 3, 3), (1, 1, 1), 0, False, True, 5),
    "k333 256->200 +colsum @24x32x32 (two N-tiles)": (256, 200, (24, 32, 32), (3, 3, 3), (1, 1, 1), 0, False, True, 5),
    "k111 128->128 @48x64x64 (128x128 tile)": (128, 128, (48, 64, 64), (1, 1, 1), (0, 0, 0), 0, False, False, 20),
}
ROUNDS = 5


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def main():
    libs = dict(a.split("=", 1) for a in sys.argv[1:])
    if len(libs) != 2:
        sys.exit(__doc__)
    LIBS = {tag: L._Lib(Path(p).resolve()) for tag, p in libs.items()}
    ta, tb = LIBS
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(3)
    torch.manual_seed(4)
    for fam in ("conv_f32", "conv_bf16x3"):
        for name, (c1, cout, dims, k, p, act, ncdhw, colsum, reps) in CASES.items():
            d, h, w = dims
            desc = L.ConvDesc(0, k[0], k[1], k[2], 1, 1, p[0], p[1], p[2], 1, c1, 0, cout, d, h, w, 0)
            x = torch.rand((d * h * w * c1,), device=DEV) * 2 - 1
            wt = (torch.randn((cout, c1) + k, generator=g) * (c1 * k[0] * k[1] * k[2]) ** -0.5).to(DEV)
            b = (torch.randn((cout,), generator=g) * 0.1).to(DEV)
            state = {}
            for tag, lib in LIBS.items():
                f = lambda s: getattr(lib, f"{fam}_{s}")
                assert f("supported")(C.byref(desc)) == 1
                gg = [C.c_int() for _ in range(6)]
                f("geometry")(C.byref(desc), *[C.byref(v) for v in gg])
                do, ho, wo, tps, ncls, cpad = [v.value for v in gg]
                packed = torch.empty(f("weight_bytes")(C.byref(desc)), dtype=torch.uint8, device=DEV)
                co = L.ConvOut()
                if ncdhw:
                    y = torch.empty((1, cout, do, ho, wo), device=DEV)
                    co.mode, (co.sn, co.sc, co.sd, co.sh, co.sw) = 1, y.stride()
                else:
                    y = torch.empty((1, do, ho, wo, cout), device=DEV)
                    co.mode, co.cout_stride, co.c_off = 0, cout, 0
                co.y, co.act = y.data_ptr(), act
                cs = torch.zeros(2 * ncls * tps * cpad, device=DEV) if colsum else None
                co.colsum = 0 if cs is None else cs.data_ptr()
                f("pack_weights")(C.byref(desc), ptr(wt), ptr(packed), sp)
                fwd = f("fwd")
                run = lambda fwd=fwd, packed=packed, co=co: fwd(C.byref(desc), ptr(x), ptr(None), ptr(packed), ptr(b), ptr(None),
                                                                 C.byref(co), sp)
                run()
                torch.cuda.synchronize()
                state[tag] = (run, y, cs, packed, co)
            same = torch.equal(state[ta][1], state[tb][1]) and (
                not colsum or torch.equal(state[ta][2], state[tb][2]))
            times = {ta: [], tb: []}
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(ROUNDS):
                for tag in (ta, tb):
                    run = state[tag][0]
                    torch.cuda.synchronize()
                    s.record()
                    for _ in range(reps):
                        run()
                    e.record()
                    torch.cuda.synchronize()
                    times[tag].append(s.elapsed_time(e) / reps * 1e3)
            pa, br = times[ta], times[tb]
            print(f"{fam:12s} {name:46s} {ta} min {min(pa):10.2f} us (max {max(pa):10.2f})   {tb} min {min(br):10.2f} us "
                  f"(max {max(br):10.2f})   {tb}/{ta} {min(br) / min(pa):.4f}   outputs identical: {same}", flush=True)
            del state, x


if __name__ == "__main__":
    main()
