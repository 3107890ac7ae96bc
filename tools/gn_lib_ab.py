"""Two builds of libctsi.so on every form of the GroupNorm passes, in ONE process: the bf16 forward (the 16 option combinations of
ctsi_gn_apply and film x drop of ctsi_gn_apply_mod), the fp32 forward, the default backward (the GN_CASES of
tests/test_gpu_train_ops.py, with and without g_buf where the entry point allows it) and the backward with options (the CASES of
tests/test_gpu_resblock_options.py x film x drop).  Every output buffer of the two libraries is compared bit for bit: y, dx, the g
buffer, dgamma, dbeta, the dtbias columns, dxsum and the workspace.  Per library it also reports whether
ctsi_gn_apply_mod(film=0, p_thr16=0) equals ctsi_gn_apply(silu_pre=1, tbias).  CTSI_GN_NT / CTSI_GN_CONTIG are read once per
process: a run of its own for each setting.

    python tools/gn_lib_ab.py A=path/to/libctsi.so B=path/to/other/libctsi.so [--time]

--time: the forward and backward at the real shapes (1, 128, 48, 128, 128) and (1, 256, 48, 64, 64): blocks of launches between two
events, library A / library B alternating, min, median and max of the per-launch time over the rounds."""
import ctypes as C
import importlib
import itertools
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
L = importlib.import_module("video-to-video-diffusion_amd.lib")
DEV = "cuda:0"
EPS = 1e-5
FWD_SHAPES = [(2, 32, 3, 5, 7), (2, 40, 3, 5, 7), (1, 192, 2, 3, 5), (1, 64, 6, 10, 10), (2, 256, 2, 6, 6)]
TB_OFF, TB_PAD = 8, 24
THR, LAYER = 16384, 5
INV = 65536.0 / (65536.0 - THR)
REAL_SHAPES = [(1, 128, 48, 128, 128), (1, 256, 48, 64, 64)]
ROUNDS = 7


def ptr(t, off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + off)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def group_sums(x, groups):
    n, c = x.shape[0], x.shape[-1]
    v = x.double().reshape(n, -1, groups, c // groups)
    return torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1).contiguous()


def operands(shape, dt, seed, film, groups=8, misalign=False):
    n, c, d, h, w = shape
    g = torch.Generator().manual_seed(seed)
    numel = n * d * h * w * c
    pad = 1 if misalign else 0          # a 4-byte offset: the fp32 pass then takes its scalar path
    xs = torch.randn(numel + pad, generator=g).to(DEV, dt)
    rs = torch.randn(numel + pad, generator=g).to(DEV, dt)
    x, res = xs[pad:].view(n, d, h, w, c), rs[pad:].view(n, d, h, w, c)
    width = 2 * c if film else c
    stride = TB_OFF + width + TB_PAD
    rows = torch.full((2 * n, stride), float("nan"))
    rows[:, TB_OFF:TB_OFF + width] = 0.5 * torch.randn((2 * n, width), generator=g)
    return dict(x=x, res=res, dy=torch.randn((n, d, h, w, c), generator=g).to(DEV, dt), gamma=(1 + 0.3 * torch.randn(c, generator=g)).to(DEV),
                beta=(0.3 * torch.randn(c, generator=g)).to(DEV), rows=rows.to(DEV), stride=stride, width=width,
                sums=group_sums(x, groups).to(DEV), groups=groups, keep=(xs, rs))


class Run:
    def __init__(self, libs):
        self.libs = libs
        self.sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.step1 = torch.tensor([1], dtype=torch.int32, device=DEV)          # row block 1 of the time rows
        self.seed = torch.tensor([0x1E3779B97F4A7C15], dtype=torch.int64, device=DEV)
        self.bad = []
        self.count = 0

    def check(self, what, outs):
        """outs: tag -> dict of output tensors"""
        (ta, a), (tb, b) = outs.items()
        diff = [k for k in a if not same(a[k], b[k])]
        self.count += 1
        if diff:
            self.bad.append(what)
            for k in diff:
                ne = bits(a[k]) != bits(b[k])
                rel = ((a[k].double() - b[k].double()).abs() / a[k].double().abs().clamp_min(1e-30))[ne.view(a[k].shape)].max()
                print(f"  DIFFERENT {what}: {k}: {int(ne.sum())} of {ne.numel()} elements, largest relative difference {float(rel):.3e}")
        return not diff

    def fwd_bf16(self, lib, shape, o, silu_pre, tb, res, post, mod=None, pre=None):
        n, c, d, h, w = shape
        y = torch.full_like(o["x"], float("nan")) if pre is None else pre
        tbp = ptr(o["rows"], 4 * TB_OFF) if tb else ptr(None)
        common = (ptr(o["x"]), ptr(y), ptr(o["sums"]), ptr(o["gamma"]), ptr(o["beta"]), n, c, d, h, w, d, o["groups"], EPS,
                  int(silu_pre), tbp, o["stride"], ptr(self.step1), ptr(o["res"] if res else None), int(post))
        if mod is None:
            lib.gn_apply(*common, self.sp)
        else:
            film, drop = mod
            lib.gn_apply_mod(*common, int(film), THR if drop else 0, INV if drop else 1.0, ptr(self.seed if drop else None), LAYER,
                             self.sp)
        return y

    def fwd_f32(self, lib, shape, o, silu_pre, tb, res, post, film=None):
        n, c, d, h, w = shape
        ys = torch.full_like(o["keep"][0], float("nan"))
        y = ys[ys.numel() - o["x"].numel():].view(o["x"].shape)
        tbp = ptr(o["rows"], 4 * TB_OFF) if tb else ptr(None)
        common = (ptr(o["x"]), ptr(y), ptr(o["sums"]), ptr(o["gamma"]), ptr(o["beta"]), n, c, d, h, w, d, o["groups"], EPS,
                  int(silu_pre), tbp, o["stride"], ptr(self.step1), ptr(o["res"] if res else None), int(post))
        if film is None:
            lib.gn_apply_f32(*common, self.sp)
        else:
            lib.gn_apply_mod_f32(*common, int(film), self.sp)
        return y

    def forward(self):
        print("== bf16 forward: 16 option combinations of ctsi_gn_apply, film x drop of ctsi_gn_apply_mod", flush=True)
        for shape in FWD_SHAPES:
            ok = True
            for film in (False, True):
                o = operands(shape, torch.bfloat16, 11 + shape[1], film)
                if not film:
                    for opt in itertools.product((0, 1), repeat=4):
                        outs = {t: dict(y=self.fwd_bf16(lib, shape, o, *opt)) for t, lib in self.libs.items()}
                        torch.cuda.synchronize()
                        ok &= self.check(f"gn_apply {shape} silu_pre,tb,res,post={opt}", outs)
                for drop in (False, True):
                    outs = {t: dict(y=self.fwd_bf16(lib, shape, o, 1, 1, 0, 0, (film, drop))) for t, lib in self.libs.items()}
                    torch.cuda.synchronize()
                    ok &= self.check(f"gn_apply_mod {shape} film={film} drop={drop}", outs)
                if not film:
                    for t, lib in self.libs.items():
                        eq = same(self.fwd_bf16(lib, shape, o, 1, 1, 0, 0, (False, False)), self.fwd_bf16(lib, shape, o, 1, 1, 0, 0))
                        print(f"  {shape} library {t}: gn_apply_mod(film=0, p_thr16=0) == gn_apply(silu_pre=1, tbias): {eq}")
            print(f"  {shape}: identical: {ok}", flush=True)
        print("== fp32 forward: 16 option combinations of ctsi_gn_apply_f32, film of ctsi_gn_apply_mod_f32", flush=True)
        cases = [(s, False) for s in FWD_SHAPES] + [((1, 6, 2, 3, 5), False), ((2, 32, 3, 5, 7), True)]
        for shape, mis in cases:
            ok = True
            groups = 3 if shape[1] == 6 else 8
            for film in (False, True):
                o = operands(shape, torch.float32, 12 + shape[1], film, groups, mis)
                if not film:
                    for opt in itertools.product((0, 1), repeat=4):
                        outs = {t: dict(y=self.fwd_f32(lib, shape, o, *opt)) for t, lib in self.libs.items()}
                        torch.cuda.synchronize()
                        ok &= self.check(f"gn_apply_f32 {shape} 4-byte offset={mis} silu_pre,tb,res,post={opt}", outs)
                outs = {t: dict(y=self.fwd_f32(lib, shape, o, 1, 1, 0, 0, film)) for t, lib in self.libs.items()}
                torch.cuda.synchronize()
                ok &= self.check(f"gn_apply_mod_f32 {shape} 4-byte offset={mis} film={film}", outs)
            print(f"  {shape} 4-byte offset={mis}: identical: {ok}", flush=True)

    def bwd(self, lib, shape, o, silu_pre, res, post, bcast, add, gbuf, pre=None):
        n, c, d, h, w = shape
        if pre is not None:
            return self._bwd(lib, shape, o, silu_pre, res, post, bcast, add, pre)
        ws = torch.full((lib.gn_bwd_workspace_floats(n, c, d, h, w, o["groups"]),), float("nan"), device=DEV)
        nanf = lambda *s: torch.full(s, float("nan"), device=DEV)
        out = dict(dx=torch.full_like(o["x"], float("nan")), dgamma=nanf(c), dbeta=nanf(c), dxsum=nanf(c), dtb=nanf(n, c + 3), ws=ws)
        if gbuf:
            out["g"] = torch.full_like(o["x"], float("nan"))
        return self._bwd(lib, shape, o, silu_pre, res, post, bcast, add, out)

    def _bwd(self, lib, shape, o, silu_pre, res, post, bcast, add, out):
        n, c, d, h, w = shape
        ws = out["ws"]
        dy = o["dy"][:, :1].contiguous() if bcast else o["dy"]
        lib.gn_bwd(ptr(o["x"]), ptr(dy), int(bcast), ptr(o["sums"]), ptr(o["gamma"]), ptr(o["beta"]), n, c, d, h, w, o["groups"], EPS,
                   int(silu_pre), ptr(o["res"] if res else None), int(post), ptr(o["keep"][1][:o["x"].numel()] if add else None),
                   ptr(out.get("g")), ptr(out["dx"]), ptr(ws), ptr(out["dgamma"]), ptr(out["dbeta"]), ptr(out["dtb"]), c + 3,
                   ptr(out["dxsum"]), self.sp)
        return out

    def bwd_mod(self, lib, shape, o, film, drop, pre=None):
        n, c, d, h, w = shape
        if pre is not None:
            return self._bwd_mod(lib, shape, o, film, drop, pre)
        ws = torch.full((lib.gn_bwd_mod_workspace_floats(n, c, d, h, w, o["groups"]),), float("nan"), device=DEV)
        nanf = lambda *s: torch.full(s, float("nan"), device=DEV)
        out = dict(dx=torch.full_like(o["x"], float("nan")), dgamma=nanf(c), dbeta=nanf(c), dxsum=nanf(c), dtb=nanf(n, o["stride"]), ws=ws)
        return self._bwd_mod(lib, shape, o, film, drop, out)

    def _bwd_mod(self, lib, shape, o, film, drop, out):
        n, c, d, h, w = shape
        ws = out["ws"]
        lib.gn_bwd_mod(ptr(o["x"]), ptr(o["dy"]), ptr(o["sums"]), ptr(o["gamma"]), ptr(o["beta"]), n, c, d, h, w, o["groups"], EPS,
                       ptr(o["rows"], 4 * TB_OFF), o["stride"], int(film), THR if drop else 0, INV if drop else 1.0,
                       ptr(self.seed if drop else None), LAYER, ptr(out["dx"]), ptr(ws), ptr(out["dgamma"]), ptr(out["dbeta"]),
                       ptr(out["dtb"], 4 * TB_OFF), o["stride"], ptr(out["dxsum"]), self.sp)
        return out

    def backward(self):
        from tests.test_gpu_resblock_options import CASES
        from tests.test_gpu_train_ops import GN_CASES
        print("== default backward: GN_CASES, with and without g_buf", flush=True)
        for name, c, groups, (n, d, h, w), silu_pre, res, post, bcast, add in GN_CASES:
            shape = (n, c, d, h, w)
            o = operands(shape, torch.bfloat16, 13 + c, False, groups)
            ok = True
            for gbuf in (True, False):
                if not gbuf and (res or post):
                    continue
                outs = {t: self.bwd(lib, shape, o, silu_pre, res, post, bcast, add, gbuf) for t, lib in self.libs.items()}
                torch.cuda.synchronize()
                ok &= self.check(f"gn_bwd {name} g_buf={gbuf}", outs)
            print(f"  {name}: identical: {ok}", flush=True)
        print("== backward with options: CASES x film x drop", flush=True)
        for shape in CASES:
            ok = True
            for film, drop in itertools.product((False, True), repeat=2):
                o = operands(shape, torch.bfloat16, 14 + shape[1], film)
                outs = {t: self.bwd_mod(lib, shape, o, film, drop) for t, lib in self.libs.items()}
                torch.cuda.synchronize()
                ok &= self.check(f"gn_bwd_mod {shape} film={film} drop={drop}", outs)
            print(f"  {shape}: identical: {ok}", flush=True)

    def time(self):
        print("== timing at the real shapes, us per launch: min / median / max over %d alternating rounds" % ROUNDS, flush=True)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for shape in REAL_SHAPES:
            o = {film: operands(shape, torch.bfloat16, 15, film, 32) for film in (False, True)}
            forms = [("fwd default silu_pre+tbias", lambda lib, p: self.fwd_bf16(lib, shape, o[False], 1, 1, 0, 0, pre=p)),
                     ("fwd default residual+post", lambda lib, p: self.fwd_bf16(lib, shape, o[False], 0, 0, 1, 1, pre=p)),
                     ("fwd film", lambda lib, p: self.fwd_bf16(lib, shape, o[True], 1, 1, 0, 0, (True, False), pre=p)),
                     ("fwd film+drop", lambda lib, p: self.fwd_bf16(lib, shape, o[True], 1, 1, 0, 0, (True, True), pre=p)),
                     ("bwd default silu_pre no g_buf", lambda lib, p: self.bwd(lib, shape, o[False], 1, 0, 0, 0, 0, False, pre=p)),
                     ("bwd default residual+post g_buf", lambda lib, p: self.bwd(lib, shape, o[False], 0, 1, 1, 0, 0, True, pre=p)),
                     ("bwd film", lambda lib, p: self.bwd_mod(lib, shape, o[True], True, False, pre=p)),
                     ("bwd film+drop", lambda lib, p: self.bwd_mod(lib, shape, o[True], True, True, pre=p))]
            for name, fn0 in forms:
                times = {t: [] for t in self.libs}
                pre = {t: fn0(lib, None) for t, lib in self.libs.items()}          # outputs allocated once, outside the timing
                for _ in range(ROUNDS):
                    for t, lib in self.libs.items():
                        torch.cuda.synchronize()
                        s.record()
                        for _ in range(5):
                            fn0(lib, pre[t])
                        e.record()
                        torch.cuda.synchronize()
                        times[t].append(s.elapsed_time(e) / 5 * 1e3)
                (ta, a), (tb, b) = times.items()
                inside = statistics.median(b) <= max(a)
                print(f"  {shape} {name:34s} {ta} {min(a):9.1f} / {statistics.median(a):9.1f} / {max(a):9.1f}   {tb} {min(b):9.1f} / "
                      f"{statistics.median(b):9.1f} / {max(b):9.1f}   {tb} median within or below {ta}'s range: {inside}", flush=True)


def main():
    args = [a for a in sys.argv[1:] if "=" in a]
    libs = dict(a.split("=", 1) for a in args)
    if len(libs) != 2:
        sys.exit(__doc__)
    run = Run({tag: L._Lib(Path(p).resolve()) for tag, p in libs.items()})
    if "--time" in sys.argv:
        run.time()
        return
    run.forward()
    run.backward()
    print(f"{run.count} comparisons, {len(run.bad)} with a difference")
    for b in run.bad:
        print("  differs:", b)


if __name__ == "__main__":
    main()
