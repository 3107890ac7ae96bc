"""Poison-and-guard harness: run a scenario with every `torch.empty / empty_like / zeros / zeros_like` allocation
placed inside a larger byte block -- `guard_bytes` below, the payload, `guard_bytes` above -- that is filled with one
byte value first.  Two kernel defects that parity tests on fresh (mostly zero) memory cannot see become visible:

  * a read of an element nobody wrote: the public result then depends on the fill byte (check 2 of `run_scenario`);
  * a store next to the buffer it was meant for: a guard byte changes (`Poison.check_guards`).

The three fills decode as (checked in tests/test_host_poison_harness.py)

    byte   bf16      fp32      fp64       int32        hides
    0x00   0         0         0          0            the lucky case ordinary tests see
    0xFF   NaN       NaN       NaN        -1           survives x * 0; a max / select can swallow it
    0x7F   3.39e38   3.40e38   1.38e306   2139062143   survives max and selects; x * 0 swallows it

Limits: a store further than `guard_bytes` from its buffer, device globals of the library and LDS are out of reach;
allocations that do not go through the four patched entry points (`.to()`, `clone`, `new_empty`, ...) are not guarded.
"""
from __future__ import annotations

import contextlib
import importlib
import struct
import sys
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import torch

FILLS = (0x00, 0xFF, 0x7F)
GUARD_BYTES = 1 << 20

_ITEMSIZE = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4, torch.float64: 8, torch.int8: 1, torch.uint8: 1,
             torch.int16: 2, torch.int32: 4, torch.int64: 8}
_NEW_KW = {"dtype", "device", "requires_grad", "layout", "pin_memory", "memory_format", "size"}
_LIKE_KW = {"dtype", "device", "requires_grad", "layout", "pin_memory", "memory_format", "input"}
_ENTRY_POINTS = ("empty", "empty_like", "zeros", "zeros_like")
_ACTIVE: List["Poison"] = []

# kernel name (Program.op_meta) -> names of the scenarios that ran it poisoned; printed once by tests/test_gpu_poison.py
COVERAGE: Dict[str, set] = {}


def _engine():
    return importlib.import_module("video-to-video-diffusion_amd.engine")


def _default_device() -> torch.device:
    get = getattr(torch, "get_default_device", None)
    return torch.device(get()) if get is not None else torch.device("cpu")


def _call_site() -> str:
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == __file__ and f.f_code.co_name in ("_alloc", "patched"):
        f = f.f_back
    if f is None:
        return "?"
    return "%s:%d %s" % (f.f_code.co_filename, f.f_lineno, f.f_code.co_name)


class Block:
    """One guarded allocation: `block` is the whole uint8 tensor, the payload is block[guard : guard + nbytes]."""
    __slots__ = ("site", "block", "nbytes", "guard", "zeroed")

    def __init__(self, site, block, nbytes, guard, zeroed):
        self.site, self.block, self.nbytes, self.guard, self.zeroed = site, block, nbytes, guard, zeroed

    @property
    def payload(self) -> torch.Tensor:
        return self.block[self.guard:self.guard + self.nbytes]


class Poison:
    """The state of one `poisoned` scope: the registry of guarded blocks and the programs built inside it."""

    def __init__(self, fill: int, guard_bytes: int, device_types: Sequence[str]):
        if not 0 <= fill <= 255:
            raise ValueError("fill is one byte")
        if guard_bytes <= 0 or guard_bytes % 512:
            raise ValueError("guard_bytes must be a positive multiple of 512 (the payload keeps the allocator's alignment)")
        self.fill, self.guard_bytes, self.device_types = fill, guard_bytes, tuple(device_types)
        self.blocks: List[Block] = []
        self._by_storage: Dict[int, Block] = {}
        self.programs: list = []
        self.max_row_pitch = 0       # over every engine.Act made in the scope: w * c * 2 bytes
        self.max_slice_bytes = 0     # ... and slice_elems * 2 bytes
        self.acts = 0
        self._real: Dict[str, Callable] = {}

    # ---- allocation -----------------------------------------------------------------------------------------
    def _wants(self, device: torch.device) -> bool:
        return device.type in self.device_types

    def _alloc(self, size: Tuple[int, ...], dtype, device: torch.device, zero: bool, requires_grad: bool) -> torch.Tensor:
        numel = 1
        for s in size:
            numel *= s
        nbytes = numel * _ITEMSIZE[dtype]
        g = self.guard_bytes
        block = self._real["empty"](g + nbytes + g, dtype=torch.uint8, device=device)
        block.fill_(self.fill)
        blk = Block(_call_site(), block, nbytes, g, zero)
        if zero:
            blk.payload.zero_()
        if device.type == "cuda":
            # the fill was queued on the caller's current stream; the buffer may be written next from any other stream (a
            # plain torch.empty carries no work to wait for), so it has to be complete before this call returns
            torch.cuda.current_stream(device).synchronize()
        self.blocks.append(blk)
        self._by_storage[block.untyped_storage().data_ptr()] = blk
        t = blk.payload.view(dtype).view(size)
        if requires_grad:
            t.requires_grad_(True)
        return t

    def _parse_new(self, args, kw):
        if not set(kw) <= _NEW_KW or kw.get("pin_memory") or kw.get("layout", torch.strided) is not torch.strided:
            return None
        if kw.get("memory_format", torch.contiguous_format) is not torch.contiguous_format:
            return None
        size = kw.get("size")
        if size is None:
            size = args[0] if (len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size))) else args
        elif args:
            return None
        size = tuple(size)
        if not all(type(s) is int and s >= 0 for s in size):
            return None
        dtype = kw.get("dtype") or torch.get_default_dtype()
        device = torch.device(kw["device"]) if kw.get("device") is not None else _default_device()
        return size, dtype, device

    def _parse_like(self, args, kw):
        if not set(kw) <= _LIKE_KW or kw.get("pin_memory") or kw.get("layout", torch.strided) is not torch.strided:
            return None
        if len(args) + ("input" in kw) != 1:
            return None
        src = args[0] if args else kw["input"]
        if not (torch.is_tensor(src) and src.layout is torch.strided and not src.is_quantized and src.is_contiguous()):
            return None
        if kw.get("memory_format", torch.preserve_format) not in (torch.preserve_format, torch.contiguous_format):
            return None
        dtype = kw.get("dtype") or src.dtype
        device = torch.device(kw["device"]) if kw.get("device") is not None else src.device
        return tuple(src.shape), dtype, device

    def _wrap(self, name: str):
        real, parse, zero = self._real[name], (self._parse_like if name.endswith("_like") else self._parse_new), \
            name.startswith("zeros")

        def patched(*args, **kw):
            spec = parse(args, kw)
            if spec is None:
                return real(*args, **kw)
            size, dtype, device = spec
            if dtype not in _ITEMSIZE or not self._wants(device) or 0 in size or len(size) == 0:
                return real(*args, **kw)
            return self._alloc(size, dtype, device, zero, bool(kw.get("requires_grad", False)))

        patched.__name__ = name
        patched.__wrapped__ = real
        return patched

    def install(self):
        for name in _ENTRY_POINTS:
            self._real[name] = getattr(torch, name)
        for name in _ENTRY_POINTS:
            setattr(torch, name, self._wrap(name))

    def uninstall(self):
        for name, fn in self._real.items():
            setattr(torch, name, fn)

    # ---- queries ---------------------------------------------------------------------------------------------
    def block_of(self, t: torch.Tensor) -> Optional[Block]:
        """The guarded block `t` lies in (its storage IS the block's), or None."""
        if not torch.is_tensor(t):
            return None
        return self._by_storage.get(t.untyped_storage().data_ptr())

    def check_guards(self) -> List[Tuple[str, int, int]]:
        """[(allocation site, offset of the first changed guard byte, how many changed)], one entry per block whose
        guard bands no longer hold the fill byte.  Offsets are in bytes relative to the payload's first byte: negative in
        the band below it, >= the payload's size in the band above."""
        if not self.blocks:
            return []
        counts = []
        for b in self.blocks:
            g = b.guard
            counts.append(((b.block[:g] != self.fill).sum() + (b.block[g + b.nbytes:] != self.fill).sum()).cpu())
        found = []
        for b, cnt in zip(self.blocks, counts):
            if int(cnt) == 0:
                continue
            g = b.guard
            bad = torch.cat([b.block[:g] != self.fill, b.block[g + b.nbytes:] != self.fill]).nonzero().flatten()
            first = int(bad[0])
            off = first - g if first < g else b.nbytes + (first - g)
            found.append((b.site, off, int(cnt)))
        return found

    def repoison(self, tensors: Iterable[torch.Tensor]):
        """Refill the bytes of `tensors` (contiguous tensors inside registered blocks) with the fill byte."""
        tensors = [t for t in tensors if t is not None]
        for t in tensors:
            if self.block_of(t) is None:
                raise AssertionError("repoison: a tensor that was not allocated inside this scope")
            t.view(torch.uint8).fill_(self.fill)
        if any(t.is_cuda for t in tensors):
            torch.cuda.synchronize()

    def repoison_scratch(self, prog):
        """Scratch by contract of an engine.Program: the activation pool and the column-sum slab.  NOT `keep`, which holds
        state (sampler z, history, schedules) and zero-initialised workspaces (split-K tickets)."""
        self.repoison(list(prog.pool.all) + [prog._colsum])

    # ---- wiring ----------------------------------------------------------------------------------------------
    def assert_wired(self, expect_programs: bool = True):
        """Every buffer a program of this scope works in was allocated through the patched entry points."""
        assert self.blocks, "the scenario ran with zero guarded allocations: the harness is not wired in"
        if expect_programs:
            assert self.programs, "no engine.Program was built inside the poisoned scope (a cached program was reused?)"
        for prog in self.programs:
            named = [("pool.all", t) for t in prog.pool.all] + [("keep", t) for t in prog.keep if torch.is_tensor(t)]
            named += [("_colsum", prog._colsum), ("_gn_sums", prog._gn_sums)]
            for what, t in named:
                if t is None:        # (a program that was abandoned before finalize_layout)
                    continue
                assert self.block_of(t) is not None, \
                    f"{type(prog).__name__}.{what}: a {tuple(t.shape)} {t.dtype} buffer was not allocated under the harness"

    def assert_guard_covers(self, ragged: bool):
        """Conditions of the method: one h-row pitch of every activation fits in a guard band (so an off-by-one row lands
        in it), and at the ragged small shapes a whole depth slice does."""
        assert self.max_row_pitch <= self.guard_bytes, (self.max_row_pitch, self.guard_bytes)
        if ragged:
            assert self.max_slice_bytes <= self.guard_bytes, (self.max_slice_bytes, self.guard_bytes)

    def kernels(self) -> set:
        names = set()
        for prog in self.programs:
            names.update(m[2] or m[0] for m in prog.op_meta)
        return names


@contextlib.contextmanager
def poisoned(fill: int, guard_bytes: int = GUARD_BYTES, *, device_types: Sequence[str] = ("cuda",),
             modules: Sequence[torch.nn.Module] = (), engine: bool = True):
    """See the module docstring.  `modules`: their cached engine programs are dropped on entry and on exit, together with
    the packed-weight cache, so every program, packed image and workspace of the scenario is allocated inside the scope
    and nothing poisoned outlives it.  `engine` False: torch entry points only (the harness's own CPU tests)."""
    if _ACTIVE:
        raise RuntimeError("poisoned() scopes do not nest")
    P = Poison(fill, guard_bytes, device_types)
    E = _engine() if engine else None

    def drop_caches():
        if E is not None:
            for m in modules:
                E.invalidate_engine_cache(m)
            E._PACKED.clear()

    real_prog_init = real_act_init = None
    if E is not None:
        real_prog_init, real_act_init = E.Program.__init__, E.Act.__init__

        def prog_init(self, *a, **k):
            P.programs.append(self)
            real_prog_init(self, *a, **k)

        def act_init(self, *a, **k):
            real_act_init(self, *a, **k)
            P.acts += 1
            P.max_row_pitch = max(P.max_row_pitch, self.w * self.c * 2)
            P.max_slice_bytes = max(P.max_slice_bytes, self.slice_elems * 2)

    drop_caches()
    _ACTIVE.append(P)
    P.install()
    try:
        if E is not None:
            E.Program.__init__, E.Act.__init__ = prog_init, act_init
        yield P
    finally:
        P.uninstall()
        if E is not None:
            E.Program.__init__, E.Act.__init__ = real_prog_init, real_act_init
        _ACTIVE.pop()
        if any(b.block.is_cuda for b in P.blocks):
            torch.cuda.synchronize()
        P.programs.clear()
        P.blocks.clear()
        P._by_storage.clear()
        drop_caches()


@contextlib.contextmanager
def no_reuse():
    """engine._Pool.put as a no-op: every activation of a program built inside gets a buffer of its own (check 5)."""
    E = _engine()
    real = E._Pool.put
    E._Pool.put = lambda self, t: None
    try:
        yield
    finally:
        E._Pool.put = real


# ---- comparing public results bit by bit -----------------------------------------------------------------------
def flatten(res, prefix: str = "") -> List[Tuple[str, object]]:
    """A scenario's result (tensor / number / None, or dicts, lists and tuples of them) as [(name, leaf)]."""
    if isinstance(res, dict):
        return [kv for k, v in res.items() for kv in flatten(v, f"{prefix}{k}.")]
    if isinstance(res, (list, tuple)):
        return [kv for i, v in enumerate(res) for kv in flatten(v, f"{prefix}{i}.")]
    return [(prefix[:-1] or "result", res)]


def snapshot(res):
    """Detach a result from the memory it was computed in: tensors -> CPU copies (the guarded blocks die with the scope)."""
    if isinstance(res, dict):
        return {k: snapshot(v) for k, v in res.items()}
    if isinstance(res, (list, tuple)):
        return [snapshot(v) for v in res]
    if torch.is_tensor(res):
        return res.detach().cpu().clone()
    return res


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


def diff_bits(a, b) -> List[str]:
    """Differences between two results, compared on integer views (NaN == NaN of the same bits, -0 != +0)."""
    fa, fb = flatten(a), flatten(b)
    if [n for n, _ in fa] != [n for n, _ in fb]:
        return [f"result structure differs: {[n for n, _ in fa]} vs {[n for n, _ in fb]}"]
    out = []
    for (name, x), (_, y) in zip(fa, fb):
        if torch.is_tensor(x) and torch.is_tensor(y):
            if x.shape != y.shape or x.dtype != y.dtype:
                out.append(f"{name}: {tuple(x.shape)} {x.dtype} vs {tuple(y.shape)} {y.dtype}")
                continue
            bx, by = _bits(x).cpu(), _bits(y).cpu()
            if not torch.equal(bx, by):
                item = x.element_size()
                bad = (bx != by).reshape(-1, item).any(1).nonzero().flatten()
                out.append(f"{name}: {bad.numel()} of {x.numel()} elements differ (first at flat index {int(bad[0])}: "
                           f"{x.reshape(-1)[int(bad[0])].item()!r} vs {y.reshape(-1)[int(bad[0])].item()!r})")
        elif isinstance(x, float) and isinstance(y, float):
            if struct.pack("<d", x) != struct.pack("<d", y):
                out.append(f"{name}: {x!r} vs {y!r}")
        elif type(x) is not type(y) or x != y:
            out.append(f"{name}: {x!r} vs {y!r}")
    return out


def evaluate_scenario(f: Callable[[], object], *, name: str = "scenario", modules: Sequence[torch.nn.Module] = (),
                      fills: Sequence[int] = FILLS, guard_bytes: int = GUARD_BYTES, device_types: Sequence[str] = ("cuda",),
                      engine: bool = True, ragged: bool = False, expect_programs: bool = True,
                      inside: Optional[Callable[[Poison, object, object], List[str]]] = None,
                      reference_fill: Optional[int] = None, no_reuse_fills: Sequence[int] = ()):
    """Checks 1-3 of a scenario `f() -> public results`.  Returns (reference result, [finding, ...]); an empty list is a
    pass.  `inside(P, result, reference) -> [difference, ...]` runs in each poisoned scope after f: check 4, see `reevaluate`.
    `no_reuse_fills`: check 5 under these fills (engine scenarios at small shapes).
    `reference_fill`: take the two reference runs under that fill instead of unpatched (the planted defects, whose
    unpatched result is whatever the allocator left behind)."""
    E = _engine() if engine else None

    def plain():
        if E is not None:
            for m in modules:
                E.invalidate_engine_cache(m)
        if reference_fill is None:
            return snapshot(f())
        with poisoned(reference_fill, guard_bytes, device_types=device_types, modules=modules, engine=engine):
            return snapshot(f())

    ref = plain()
    again = plain()
    d = diff_bits(again, ref)
    if d:      # nondeterminism: the finding; checks 2-5 would say nothing
        return ref, [f"{name}: two plain runs differ: {x}" for x in d]
    findings = []
    for fill in fills:
        with poisoned(fill, guard_bytes, device_types=device_types, modules=modules, engine=engine) as P:
            res = f()
            got = snapshot(res)
            findings += [f"{name}: fill 0x{fill:02X}: result depends on uninitialised memory: {x}" for x in diff_bits(got, ref)]
            findings += [f"{name}: fill 0x{fill:02X}: write outside its buffer, allocated at {site}: first changed guard "
                         f"byte at offset {off}, {cnt} changed" for site, off, cnt in P.check_guards()]
            if inside is not None:
                findings += [f"{name}: fill 0x{fill:02X}: second evaluation depends on what the first left in scratch: {x}"
                             for x in inside(P, res, ref)]
                findings += [f"{name}: fill 0x{fill:02X}: write outside its buffer (second evaluation), allocated at {site}: "
                             f"offset {off}, {cnt} changed" for site, off, cnt in P.check_guards()]
            if engine:
                P.assert_wired(expect_programs)
                P.assert_guard_covers(ragged)
            else:
                assert P.blocks, "the scenario ran with zero guarded allocations: the harness is not wired in"
            for k in P.kernels():
                COVERAGE.setdefault(k, set()).add(name)
            del res
    for fill in no_reuse_fills:      # check 5: every activation in a buffer of its own
        with no_reuse(), poisoned(fill, guard_bytes, device_types=device_types, modules=modules, engine=engine) as P:
            got = snapshot(f())
            findings += [f"{name}: fill 0x{fill:02X}, no buffer reuse: result depends on what an earlier layer left in a "
                         f"recycled buffer (or a buffer was released before its last reader): {x}" for x in diff_bits(got, ref)]
            findings += [f"{name}: fill 0x{fill:02X}, no buffer reuse: write outside its buffer, allocated at {site}: offset "
                         f"{off}, {cnt} changed" for site, off, cnt in P.check_guards()]
            P.assert_wired(expect_programs)
    return ref, findings


def reevaluate(f: Callable[[], object]):
    """Check 4 as an `inside` hook: refill the scratch of every program the scope built (activation pool, column-sum slab)
    and evaluate again -- the cached programs and their captured graphs are reused -- against the reference."""
    def inside(P: Poison, res, ref):
        for prog in P.programs:
            if prog._colsum is not None:
                P.repoison_scratch(prog)
        built = len(P.programs)
        got = snapshot(f())
        assert len(P.programs) == built, "the second evaluation built new programs instead of launching the cached ones again"
        return diff_bits(got, ref)
    return inside


def run_scenario(f, **kw):
    """evaluate_scenario, asserted: returns the reference result."""
    ref, findings = evaluate_scenario(f, **kw)
    assert not findings, "\n".join(findings)
    return ref


# ---- planted defects: torch ops only, every access inside one guarded block -----------------------------------------
# (tests/test_host_poison_harness.py on the CPU, once on the GPU in tests/test_gpu_poison.py: they show that the harness
# bites, and why there are three fills.  The overrun toys are only safe INSIDE a poisoned scope.)
def toy_overrun(device, below: bool) -> torch.Tensor:
    """A 'kernel' that stores one int32 element next to its 64-element buffer."""
    buf = torch.empty(64, dtype=torch.int32, device=device)
    buf.fill_(3)
    off = buf.storage_offset() + (-1 if below else 64)
    torch.as_strided(buf, (1,), (1,), off).fill_(0x55555555)      # every byte differs from each of the three fills
    return buf


def toy_read_unwritten(device) -> torch.Tensor:
    """Writes 7 of 8 elements, sums all 8."""
    buf = torch.empty(8, dtype=torch.float32, device=device)
    buf[:7] = torch.arange(1, 8, dtype=torch.float32, device=device)
    return buf.sum()


def toy_times_zero(device) -> torch.Tensor:
    """The unwritten element is 'cancelled' by a zero weight: NaN * 0 is NaN, 3.4e38 * 0 is 0."""
    buf = torch.empty(8, dtype=torch.float32, device=device)
    buf[:7] = torch.arange(1, 8, dtype=torch.float32, device=device)
    wgt = torch.ones(8, dtype=torch.float32, device=device)
    wgt[7] = 0.0
    return (buf * wgt).sum()


def toy_max(device) -> torch.Tensor:
    """The unwritten element goes through fmax(x, 1), as the device's max does: a NaN is dropped, 3.4e38 is not."""
    buf = torch.empty(8, dtype=torch.float32, device=device)
    buf[:7] = torch.arange(1, 8, dtype=torch.float32, device=device)
    return torch.fmax(buf, torch.ones(8, dtype=torch.float32, device=device)).clamp(max=1e30).sum()
