"""Host-side execution engine: turns the reference's module trees (UNet3D, the VAE encoder and
decoder) into flat programs of libctsi launches on one HIP stream, optionally captured into a
hipGraph (one graph per denoising step).

PyTorch is used here for device memory, the stream object and parameter storage only; every
arithmetic op of the hot path is a libctsi kernel.  There is no CPU path: constructing a context
without a HIP device (or without libctsi.so) raises ``CtsiError``.

Data layout in HBM
  activations   bf16, channels-last (n, d, h, w, c), c contiguous; 16-byte (8-channel) accesses
  weights       bf16, re-laid out once per layer into the gather-GEMM image [class][cout_pad][K]
  GN statistics fp32 per-tile column sums -> fp64 (sum, sumsq) per (sample, group)
  sampler state fp32 NDHWC (z) + its bf16 copy inside the U-Net input tensor [z | cond]
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import weakref
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from .attention import ATTENTION_MODES, check_attention_mode, emit_softmax_attention
from .spatial_attention import check_spatial_attention_supported, emit_spatial_attention
from .learned_sigma import add_sigma_split, check_learn_sigma_unsharded
from .lib import ConvDesc, ConvOut, CtsiError, get_lib
from .prediction import add_pred_to_eps, check_prediction_type
from .x0_form import add_x0_step, check_update_form

_CTX: Dict[int, "Ctx"] = {}

# Packed-weight cache ("weight pre-packing cache keyed by checkpoint hash").  The bf16 kernel-layout
# image of a layer's weights is content-addressed: key = (layout signature of the plan, _pack_sig; 2 x 64-bit checksum of
# the fp32 weight tensor the layer's weight_fn returns).  Every program built from the same weights -- the sampler program, the
# plain forward, other latent shapes, window batches, the depth-sharded variants: 265 M parameters = 0.53 GB of packed
# bf16 per program otherwise -- shares ONE image and packs it once.  Entries are immutable and die with their last user
# (weak values); a program whose weights changed looks up / packs new images and drops its captured graph.  Both precisions
# read and fill it in one place, Program._weight_image.
_PACKED: Dict[int, "weakref.WeakValueDictionary"] = {}
# every live program (weak): check_device_errors re-zeroes their split-K hand-off workspaces after a reported device error
_LIVE_PROGRAMS: "weakref.WeakSet" = weakref.WeakSet()


def _pack_sig(lib, plan, transposed, k, s, c1: int, c2: int, cout: int, cin_w: Optional[int]) -> tuple:
    """The layout half of a packed-image cache key: everything ctsi_conv_plan_pack_weights reads besides the weight values.
    ctsi_conv_plan_pack_layout names the image layout the plan's kernel consumes (family; for the k32 kernel also its form
    and the cout-permuted image of the direct-store epilogue, which the tile and split-K choice -- hence the batch size and
    the depth-sharded view -- decide); the rest are the descriptor's channel / kernel fields and the plan's sizes."""
    bm, bn, mode = C.c_int(), C.c_int(), C.c_int()
    lib.conv_plan_config(plan, C.byref(bm), C.byref(bn), C.byref(mode))
    return (lib.conv_plan_pack_layout(plan), int(transposed), tuple(k), tuple(s), c1, c2, cout, cin_w,
            lib.conv_plan_cout_pad(plan), lib.conv_plan_weight_bytes(plan), bn.value, bm.value,
            bool(lib.conv_plan_workspace_bytes(plan)))


_KEY_CHUNK = 1 << 22


def _content_key(wt: torch.Tensor) -> Tuple[int, int, int]:
    """Two independent 63-bit position-dependent checksums of the fp32 bit patterns + the element count.  Each element is
    mixed with its index through an odd-constant multiply and an xor-shift (wrapping int64 arithmetic), so neither sum is
    linear in the data nor periodic in the position; computed in 4 M-element chunks (16 MB of temporaries, not 3 x numel
    int64) and read back with ONE host sync per tensor."""
    xi = wt.reshape(-1).view(torch.int32)
    acc = torch.zeros(2, dtype=torch.int64, device=wt.device)
    for off in range(0, xi.numel(), _KEY_CHUNK):
        v = xi[off:off + _KEY_CHUNK].to(torch.int64) & 0xFFFFFFFF
        idx = torch.arange(off, off + v.numel(), device=wt.device, dtype=torch.int64)
        h = v + 0x632BE59BD9B4E019 + idx * -0x61C8864680B583EB      # odd (golden-ratio) constant; int64 wraps
        h = h ^ (h >> 29)
        h = h * -0x4B47D0C5B1A3F1B5
        h = h ^ (h >> 32)
        g = (v ^ (idx * 0x2545F4914F6CDD1D)) * -0x395B586CA42E166B
        g = g ^ (g >> 31)
        acc[0] += h.sum()
        acc[1] += g.sum()
    a = acc.tolist()
    return int(a[0]), int(a[1]), int(xi.numel())


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


class Ctx:
    """Per-device engine context: the library handle and the engine's own HIP stream."""

    def __init__(self, device: torch.device):
        self.lib = get_lib()
        if not torch.cuda.is_available() or not self.lib.device_available():
            raise CtsiError("the HIP engine needs a ROCm device; none is visible to this process")
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self.sptr = C.c_void_p(self.stream.cuda_stream)

    @staticmethod
    def get(device) -> "Ctx":
        device = torch.device(device)
        if device.type != "cuda":
            raise CtsiError(
                f"the HIP engine runs on ROCm devices only (got device '{device}'); there is no CPU path")
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in _CTX:
            _CTX[idx] = Ctx(torch.device("cuda", idx))
        return _CTX[idx]

    def comm_stream_ptr(self) -> C.c_void_p:
        """The context's second HIP stream (created on first use): halo transfers that overlap interior compute."""
        if getattr(self, "_comm_stream", None) is None:
            self._comm_stream = torch.cuda.Stream(device=self.device)
        return C.c_void_p(self._comm_stream.cuda_stream)

    # make the engine stream wait for work queued on torch's current stream, and vice versa
    def enter(self):
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def leave(self):
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    @contextlib.contextmanager
    def scope(self):
        """Run a block on the engine stream, ordered after/before the caller's current stream."""
        self.enter()
        try:
            with torch.cuda.stream(self.stream):
                yield self
        finally:   # also on an exception: the caller's stream must still wait for what was queued
            self.leave()


class _Pool:
    """Tiny size-keyed buffer pool used while a program is being laid out (ops run in stream
    order, so a buffer may be handed out again as soon as its last reader has been emitted)."""

    def __init__(self, device):
        self.device = device
        self.free: Dict[Tuple[int, torch.dtype], List[torch.Tensor]] = {}
        self.all: List[torch.Tensor] = []   # ops hold raw pointers: every buffer lives as long as the program
        self.total_bytes = 0

    def get(self, numel: int, dtype: torch.dtype) -> torch.Tensor:
        lst = self.free.get((numel, dtype))
        if lst:
            return lst.pop()
        self.total_bytes += numel * torch.empty(0, dtype=dtype).element_size()
        t = torch.empty(numel, dtype=dtype, device=self.device)
        self.all.append(t)
        return t

    def put(self, t: torch.Tensor):
        self.free.setdefault((t.numel(), t.dtype), []).append(t)


class Act:
    """A bf16 NDHWC activation buffer with its logical shape.  In depth-sharded programs (`halo` = 1)
    the buffer holds d + 2 slices: one halo slice below and above the rank's own d slices."""
    __slots__ = ("t", "n", "c", "d", "h", "w", "halo", "dirty", "grad")

    def __init__(self, t, n, c, d, h, w, halo=0):
        self.t, self.n, self.c, self.d, self.h, self.w = t, n, c, d, h, w
        self.halo = halo
        self.dirty = True  # halo slices stale (they are refreshed lazily, right before a depth-3 conv)
        self.grad = None   # gradient Act (training programs only)

    @property
    def vox(self):
        return self.d * self.h * self.w

    @property
    def slice_elems(self):
        return self.h * self.w * self.c

    @property
    def ip(self) -> C.c_void_p:
        """pointer to the first own (interior) slice"""
        return C.c_void_p(self.t.data_ptr() + self.halo * self.slice_elems * 2)

    @property
    def fp(self) -> C.c_void_p:
        """pointer to the whole buffer (lower halo slice first)"""
        return C.c_void_p(self.t.data_ptr())


class _ConvPlan(NamedTuple):
    """One bf16 conv layer as Program._conv_setup leaves it: the plan and everything the emitters read of it."""
    plan: C.c_void_p
    desc: ConvDesc
    out_dims: Tuple[int, int, int]      # (d, h, w) of the output
    wbytes: int                         # size of the packed weight image
    mode: int                           # the plan's kernel family (ctsi_conv_plan_config)
    kernel: str                         # the launch's label (_conv_label)
    flops: float
    tiles: int
    tps: int                            # tiles per sample
    cpad: int                           # cout padded to the kernel's tile
    workspace: int                      # split-K hand-off workspace (device address), 0: the plan has none
    holder: List[Optional[torch.Tensor]]    # [the packed weight image] (Program._weight_image)


def _conv_label(bm: int, bn: int, mode: int, desc: ConvDesc, split_k: bool) -> str:
    """conv_mfma_<bm>x<bn>_m<mode>[t|d|p][s] -- t: ConvTranspose form, d: Downsample form, p: planar (1,3,3) form (all of the
    k32 family, mode 9), s: split-K form."""
    form = "t" if desc.transposed else ("d" if (desc.sh, desc.sw) == (2, 2) else ("p" if desc.kd == 1 and desc.kh == 3 else ""))
    return "conv_mfma_%dx%d_m%d%s%s" % (bm, bn, mode, form if mode == 9 else "", "s" if split_k else "")


class Program:
    """A flat list of libctsi launches plus the buffers they touch."""

    def __init__(self, ctx: Ctx):
        self.ctx = ctx
        self.lib = ctx.lib
        self.ops: List[Callable[[], None]] = []
        self.op_meta: List[Tuple[str, float, str]] = []
        self.op_bytes: List[float] = []
        self.op_alg_bytes: List[float] = []   # convs: algorithmic HBM bytes (inputs + outputs + weights, each once)
        self.op_audit: List[Optional[dict]] = []   # per op: what it computes from which buffers (see _emit), or None
        self.pool = _Pool(ctx.device)
        self.keep: List[object] = []       # tensors / ctypes structs that must outlive the ops
        self.plans: List[C.c_void_p] = []  # conv plan handles (destroyed with the program)
        self.pack_fns: List[Callable[[], None]] = []
        self.flops = 0.0
        self.conv_flops: List[Tuple[str, float]] = []
        self.gn_slots = 0
        self._gn_sums: Optional[torch.Tensor] = None
        self._colsum: Optional[torch.Tensor] = None
        self._colsum_need = 0
        self._gn_need: List[Tuple[int, int]] = []
        self.graph = None
        self._params: List[torch.Tensor] = []
        self._param_storages: set = set()    # storage addresses of the tracked parameters (_build_fast)
        self._track_module: Optional[nn.Module] = None
        self._events: List[C.c_void_p] = []  # fork / join events of overlapped convs (destroyed with the program)
        self._versions: Tuple[int, ...] = ()
        self.shard = None  # parallel.ShardSpec for depth-sharded programs
        self.weight_cache = True    # share packed weight images between programs (training programs repack in place)
        self._weights_moved = False
        self.pack_stats = dict(packed=0, shared=0)
        # fast re-pack (see fast_repack): what every pack function reads and writes, so that the launches can be replayed from
        # prebuilt pointer tables without touching torch
        self._f32_meta: List[dict] = []     # dev_f32 buffers: dict(buf, make, parts, scale, fn)
        self._pack_meta: List[dict] = []    # conv weight images: dict(plan (None: an fp32 image), weight_fn, holder, fn)
        self._fast = None
        self._sk_workspaces: List[torch.Tensor] = []   # split-K hand-off workspaces (tickets / flags + parked partial sums)
        _LIVE_PROGRAMS.add(self)

    def _emit(self, fn: Callable[[], None], name: str = "op", flops: float = 0.0, kernel: str = "", nbytes: float = 0.0,
              alg_bytes: float = 0.0, audit: Optional[dict] = None):
        """`nbytes`: algorithmic HBM bytes of an HBM-bound op (what bench.py divides by the launch time for GB/s).
        `audit`: a description of what the op computes -- its kind, the Acts / tensors it reads and writes and the scalars of
        the formula (references only; it changes nothing about the launch).  Every op that computes something carries one,
        so that a test can re-derive each launch's result from its own operands (tests/fwd_audit.py for the forward ops,
        tests/train_audit.py for the training backward).  Buffers that exist only after finalize_layout (`_colsum`,
        `_gn_sums`) are named through a callable."""
        self.ops.append(fn)
        self.op_meta.append((name, flops, kernel))
        self.op_bytes.append(float(nbytes))
        self.op_alg_bytes.append(float(alg_bytes))
        self.op_audit.append(audit)

    # ---- buffers -------------------------------------------------------------------------------------
    def act(self, n, c, d, h, w, halo: Optional[int] = None) -> Act:
        if halo is None:
            halo = 1 if self.shard is not None else 0
        return Act(self.pool.get(n * c * (d + 2 * halo) * h * w, torch.bfloat16), n, c, d, h, w, halo)

    # ---- depth-sharding collectives (no-ops in single-GPU programs) -----------------------------------
    # A sharded program is ~64 sync points per U-Net evaluation (was 119): the GroupNorm statistics of a tensor travel in
    # the SAME sync point as the raw boundary slices of that tensor (`sync_stats_and_halos`); the normalisation is then
    # applied to the own slices AND the received halo slices (`ext` ranges below), so the tensor a depth-3 conv consumes
    # never needs a second exchange.  Only tensors no GroupNorm follows (conv_in / Downsample / Upsample outputs, the
    # sampler's updated input) use the plain `halo_exchange`.
    def _slices(self, a: Act):
        se, d = a.slice_elems, a.d
        buf = a.t
        return buf[se:2 * se], buf[d * se:(d + 1) * se], buf[0:se], buf[(d + 1) * se:(d + 2) * se]

    def halo_exchange(self, a: Act):
        """Refresh a's two halo slices from the depth neighbours (zeros at the volume's ends)."""
        if self.shard is None or not a.halo or not a.dirty:
            return
        a.dirty = False
        lo_own, hi_own, lo_halo, hi_halo = self._slices(a)
        spec, sptr = self.shard, self.ctx.sptr

        def run():
            spec.comm.exchange(spec.rank, lo_own, hi_own, lo_halo, hi_halo, sptr=sptr)

        self._emit(run, "halo.exchange", 0.0, "comm")

    def sync_stats_and_halos(self, a: Optional[Act], slot: Optional[int], nvals: int = 0,
                             f32: Optional[torch.Tensor] = None, name: str = "gn.sync"):
        """ONE sync point: all-reduce of the fp64 statistics slot (and of `f32`, the attention depth sum) together with
        the neighbour exchange of a's raw boundary slices (a = None: statistics only)."""
        if self.shard is None:
            return
        spec, sptr, prog = self.shard, self.ctx.sptr, self
        sl = self._slices(a) if (a is not None and a.halo) else (None, None, None, None)
        if a is not None and a.halo:
            a.dirty = False
        holder = {}

        def run():
            sums = None
            if slot is not None:
                if "v" not in holder:
                    holder["v"] = prog._gn_sums[slot:slot + nvals]
                sums = holder["v"]
            spec.comm.exchange(spec.rank, sl[0], sl[1], sl[2], sl[3], sums=sums, f32=f32, sptr=sptr)

        self._emit(run, name, 0.0, "comm")

    def ext(self, a: Act) -> Tuple[int, int]:
        """(slices below the own ones, total depth) of the range an elementwise op covers on `a`: the own slices plus
        the halo slices that exist -- none on a single GPU, none towards a volume end (those stay zero: the conv's
        zero padding)."""
        if self.shard is None or not a.halo:
            return 0, a.d
        lo = 1 if self.shard.rank > 0 else 0
        hi = 1 if self.shard.rank < self.shard.world - 1 else 0
        return lo, a.d + lo + hi

    def ext_ptr(self, a: Act, lo: int) -> C.c_void_p:
        return C.c_void_p(a.ip.value - lo * a.slice_elems * 2)

    def zero_end_halos(self, a: Act):
        """A NEW buffer written over its `ext` range: the halo slice towards a volume end is not covered and must read
        as zeros (emitted on every rank -- the lock-step test driver needs equal op lists; a no-op on inner ranks)."""
        if self.shard is None or not a.halo:
            return
        spec, lib, sptr = self.shard, self.lib, self.ctx.sptr
        _, _, lo_halo, hi_halo = self._slices(a)
        nbytes = a.slice_elems * 2

        def run():
            if spec.rank == 0:
                lib.memset_async(_ptr(lo_halo), 0, nbytes, sptr)
            if spec.rank == spec.world - 1:
                lib.memset_async(_ptr(hi_halo), 0, nbytes, sptr)

        self._emit(run, "halo.zero_ends")

    def release(self, a: Act):
        self.pool.put(a.t)

    def _conv_workspace(self, plan) -> int:
        """Device scratch of a split-K conv plan (ctsi_conv_plan_workspace_bytes): one zero-initialised buffer per layer, kept
        for the program's lifetime (the kernel leaves its hand-off tickets reset after every launch)."""
        nbytes = self.lib.conv_plan_workspace_bytes(plan)
        if not nbytes:
            return 0
        ws = self.persistent((nbytes,), torch.uint8, zero=True)
        self._sk_workspaces.append(ws)
        return ws.data_ptr()

    def check_errors(self):
        """Programs with split-K layers: raise if one of their hand-offs failed (see check_device_errors).  The samplers
        check once per sample() whatever the program holds; the VAE legs and the training step call this, which costs a
        stream synchronisation only when the program has such a layer at all."""
        if self._sk_workspaces:
            check_device_errors(self.ctx)

    def persistent(self, shape, dtype, zero=False) -> torch.Tensor:
        t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.ctx.device)
        self.keep.append(t)
        return t

    # ---- parameters ------------------------------------------------------------------------------------
    def track(self, *params: torch.Tensor):
        self._params.extend(params)

    def dev_f32(self, make: Callable[[], torch.Tensor], parts: Optional[Sequence[Callable[[], torch.Tensor]]] = None,
                scale: float = 1.0) -> torch.Tensor:
        """A persistent fp32 device copy of a (derived) parameter, refreshed by repack().  `parts` (optional) says how the
        value is made of parameter storage -- buf = scale * concat(part() for part in parts), every part a contiguous view
        of a parameter -- so that fast_repack() can refresh it from a pointer table; a `make()` that itself returns such a
        view needs no `parts`."""
        src = make().detach()
        buf = torch.empty(src.shape, dtype=torch.float32, device=self.ctx.device)
        self.keep.append(buf)

        def refresh():
            buf.copy_(make().detach().to(device=self.ctx.device, dtype=torch.float32))

        self.pack_fns.append(refresh)
        self._f32_meta.append(dict(buf=buf, make=make, parts=parts, scale=float(scale), fn=refresh))
        return buf

    # ---- fast re-pack after an optimizer step (optim.FusedAdamW) -------------------------------------------------------
    # The generic repack() goes through torch for every operand (600 small copies and pack launches for the training
    # program: ~6 ms, all of it host time).  After an optimizer step nothing but the VALUES changed, so the same device
    # work can be issued from tables built once: ONE ctsi_copy_scale_multi launch for all small fp32 operands and one
    # ctypes call per conv image (+ its dgrad re-layout), with every pointer precomputed.  Only programs that own their
    # weight images (weight_cache False: the training program) take this path; operands it cannot express (values that are
    # not contiguous views of parameter storage) keep their generic refresh function.
    def _param_view(self, t: torch.Tensor) -> bool:
        """A contiguous fp32 view INTO THE STORAGE OF A TRACKED PARAMETER: only such an address is still the value's home
        after the next optimizer step (a temporary -- cat, scaled copy, matmul result -- passes every other test, and its
        freed address would be baked into the pointer table and the recorded graph)."""
        if not (torch.is_tensor(t) and t.is_cuda and t.device == self.ctx.device and t.dtype == torch.float32
                and t.is_contiguous() and t.numel() > 0):
            return False
        return t.untyped_storage().data_ptr() in self._param_storages

    def _build_fast(self):
        import struct
        if self._fast and self._fast.get("graph") is not None:      # (a parameter moved: the recorded pointers are stale)
            self.lib.graph_destroy(self._fast["graph"])
            self._fast["graph"] = None
        # where the parameters live NOW (this runs again exactly when one of them moved: the old addresses may be reused)
        self._param_storages = {p.untyped_storage().data_ptr() for p in self._params if torch.is_tensor(p)}
        segs, slow, packs = [], [], []
        for ent in self._f32_meta:
            parts = ent["parts"] if ent["parts"] is not None else [ent["make"]]
            vals = [pt() for pt in parts]
            if all(self._param_view(v.detach()) for v in vals) and sum(v.numel() for v in vals) == ent["buf"].numel():
                off = 0
                for v in vals:
                    segs.append((v.data_ptr(), ent["buf"].data_ptr() + 4 * off, v.numel(), ent["scale"]))
                    off += v.numel()
            else:
                slow.append(ent["fn"])
        lib, sptr, dev = self.lib, self.ctx.sptr, self.ctx.device
        for ent in self._pack_meta:
            holder, plan, wfn = ent["holder"], ent["plan"], ent["weight_fn"]
            fast = getattr(wfn, "fast_layout", None)
            if holder[0] is None or plan is None:     # (an fp32 image is packed from its descriptor: no plan to replay)
                slow.append(ent["fn"])
                continue
            dst = C.c_void_p(holder[0].data_ptr())
            if fast is not None:      # data-gradient image: flipped / transposed re-layout of a parameter view, then the pack
                src_fn, co_w, ci_w, T, coff, cnt = fast
                src = src_fn().detach()
                if not self._param_view(src):
                    slow.append(ent["fn"])
                    continue
                tmp = torch.empty((cnt * co_w * T,), dtype=torch.float32, device=dev)
                self.keep.append(tmp)
                sp, tp = C.c_void_p(src.data_ptr()), C.c_void_p(tmp.data_ptr())
                packs.append((lib.weight_dgrad_layout, (sp, tp, co_w, ci_w, T, coff, cnt, sptr)))
                packs.append((lib.conv_plan_pack_weights, (plan, tp, dst, sptr)))
                continue
            wt = wfn().detach()
            if self._param_view(wt):
                packs.append((lib.conv_plan_pack_weights, (plan, C.c_void_p(wt.data_ptr()), dst, sptr)))
            else:
                slow.append(ent["fn"])
        # refresh functions registered outside the two tables (an attention block's folded matrix) have no fast form: they
        # run as they are, and keep the step out of the recorded graph
        known = {id(ent["fn"]) for ent in self._f32_meta} | {id(ent["fn"]) for ent in self._pack_meta}
        slow.extend(fn for fn in self.pack_fns if id(fn) not in known and fn not in slow)
        seg_bytes = b"".join(struct.pack("<QQqfi", s_, d_, n_, sc, 0) for (s_, d_, n_, sc) in segs)
        pieces = [(i, q) for i, (_, _, n_, _) in enumerate(segs) for q in range((n_ + 4095) // 4096)]
        pc_bytes = b"".join(struct.pack("<ii", i, q) for (i, q) in pieces)
        seg_t = torch.frombuffer(bytearray(seg_bytes or b"\0" * 32), dtype=torch.uint8).to(dev)
        pc_t = torch.frombuffer(bytearray(pc_bytes or b"\0" * 8), dtype=torch.uint8).to(dev)
        self._fast = dict(segs=seg_t, pieces=pc_t, npieces=len(pieces), packs=packs, slow=slow,
                          ptrs=tuple(p.data_ptr() for p in self._params), nseg=len(segs))

    def fast_repack(self):
        """Re-pack after the parameter VALUES changed in place (same storage): see the comment above.  Falls back to the
        generic repack() for programs that share weight images, and rebuilds its tables when a parameter moved."""
        if self.weight_cache:
            return self.repack()
        if self._fast is None or self._fast["ptrs"] != tuple(p.data_ptr() for p in self._params):
            with torch.cuda.stream(self.ctx.stream):
                self._build_fast()
        f = self._fast
        with torch.cuda.stream(self.ctx.stream):
            if f.get("graph") is None and not f["slow"] and not os.environ.get("CTSI_NO_REPACK_GRAPH"):
                # every launch of the list has constant arguments: record it once, replay it as ONE hipGraph afterwards
                # (240 launches for the training program: ~1 ms of ctypes calls otherwise)
                self.lib.graph_begin_capture(self.ctx.sptr)
                ok = False
                try:
                    self.lib.copy_scale_multi(_ptr(f["segs"]), _ptr(f["pieces"]), f["npieces"], self.ctx.sptr)
                    for fn, args in f["packs"]:
                        fn(*args)
                    ok = True
                finally:
                    g = C.c_void_p()
                    self.lib.graph_end_capture(self.ctx.sptr, C.byref(g))
                    if not ok and g:          # a launch failed under capture: the partial graph must not be replayed
                        self.lib.graph_destroy(g)
                f["graph"] = g
            if f.get("graph") is not None:
                self.lib.graph_launch(f["graph"], self.ctx.sptr)
            else:
                self.lib.copy_scale_multi(_ptr(f["segs"]), _ptr(f["pieces"]), f["npieces"], self.ctx.sptr)
                for fn, args in f["packs"]:
                    fn(*args)
                for fn in f["slow"]:
                    fn()
        self._versions = self._fingerprint()

    def _fingerprint(self):
        """What the packed weights were made from: the tracked Parameter objects' in-place version counters and
        storage addresses, plus (when the program knows its module) the objects and addresses the module's
        parameter names resolve to NOW -- so optimizer steps, `load_state_dict` (in place or assign=True) and a
        replaced `module.weight` are all seen.  Writes through `p.data` / raw pointers bump nothing torch can
        observe: call `model.invalidate_engine_cache()` after those."""
        fp = [(p._version, p.data_ptr()) for p in self._params]
        if self._track_module is not None:
            fp.extend((id(p), p._version, p.data_ptr()) for p in self._track_module.parameters())
        return tuple(fp)

    def track_module(self, module: nn.Module):
        self._track_module = module
        self.track(*list(module.parameters()))

    def repack(self):
        with torch.cuda.stream(self.ctx.stream):
            for fn in self.pack_fns:
                fn()
        self._versions = self._fingerprint()
        if self._weights_moved:
            # content-addressed weight images: changed weights live in NEW buffers, so a captured graph (which holds the
            # old pointers) is dropped; the samplers re-capture on their next call, launch() runs eagerly until then
            self._weights_moved = False
            if self.graph is not None:
                self.lib.graph_destroy(self.graph)
                self.graph = None

    def ensure_fresh(self):
        if self._fingerprint() != self._versions:
            self.repack()

    def needs_rebuild(self) -> bool:
        return False

    # ---- conv ----------------------------------------------------------------------------------------------
    # One emitter for every conv of every program.  What both precisions need -- the weight image, the `norm_in` pre-pass,
    # the bias buffer, the column-sum slab, the ConvOut target, the flops count -- is a method of its own below:
    # conv() / _conv_overlapped put them around a conv plan, engine_f32._F32Ops.conv around ctsi_conv_f32_fwd.
    def _weight_image(self, weight_fn, sig: tuple, wbytes: int, pack_call, plan=None) -> List[Optional[torch.Tensor]]:
        """Register the packed kernel-layout image of a conv's weights and return its holder, a one-element list that
        repack() fills and the launch reads.  `sig` is the layout half of the cache key (_pack_sig / _f32_pack_sig);
        `pack_call(src, dst)` lays the fp32 weights out: ctsi_conv_plan_pack_weights on `plan`, or
        ctsi_conv_f32_pack_weights on a descriptor (`plan` None).  A program that shares images (`weight_cache`) looks the
        image up in _PACKED by (sig, content) and packs on a miss only; the others own a private image, repacked in place."""
        prog, dev = self, self.ctx.device
        holder: List[Optional[torch.Tensor]] = [None]

        def pack():
            wt = weight_fn().detach().to(device=dev, dtype=torch.float32).contiguous()
            if prog.weight_cache:
                cache = _PACKED.setdefault(dev.index, weakref.WeakValueDictionary())
                key = (sig, _content_key(wt))
                t = cache.get(key)
                if t is None:
                    t = torch.empty(wbytes, dtype=torch.uint8, device=dev)
                    pack_call(_ptr(wt), _ptr(t))
                    cache[key] = t
                    prog.pack_stats["packed"] += 1
                else:
                    prog.pack_stats["shared"] += 1
            else:
                t = holder[0] if holder[0] is not None else torch.empty(wbytes, dtype=torch.uint8, device=dev)
                pack_call(_ptr(wt), _ptr(t))
            wt.record_stream(prog.ctx.stream)
            if holder[0] is not t:
                prog._weights_moved = prog._weights_moved or holder[0] is not None
                holder[0] = t

        self.pack_fns.append(pack)
        self._pack_meta.append(dict(plan=plan, weight_fn=weight_fn, holder=holder, fn=pack))
        return holder

    def _norm_in_pass(self, x1: Act, norm_in, synced: bool = False):
        """The `norm_in` of conv(): x1 <- silu?(gn(x1)) + tbias in place, as a pass of its own ahead of the conv.  A fifth
        entry of `norm_in` (film, True) makes it the scale-shift form silu(gn(x1) * (1 + s) + b) of the same pass."""
        slot, gn, silu, tb, *mode = norm_in
        kw_tb = {} if tb is None else dict(tbias=tb[0], tbias_off=tb[1], tbias_stride=tb[2], step_ptr=tb[3])
        if mode and mode[0]:
            kw_tb["film"] = True
        self.gn_apply(x1, slot, gn, silu_pre=silu, out=x1, synced=synced, **kw_tb)

    def _conv_bias(self, bias_fn) -> Optional[torch.Tensor]:
        if bias_fn is None:
            return None
        return self.dev_f32(bias_fn, parts=getattr(bias_fn, "parts", None), scale=getattr(bias_fn, "scale", 1.0))

    def _count_conv(self, name: str, fl: float):
        self.flops += fl
        self.conv_flops.append((name, fl))

    def _conv_stats(self, tiles: int, tps: int, cpad: int, nclass: int, off: int = 0) -> dict:
        """The handle gn_finalize takes for the column sums a `want_stats` conv of `tiles` tiles writes, `off` floats into
        the program's column-sum buffer."""
        self._colsum_need = max(self._colsum_need, off + 2 * tiles * cpad)
        return dict(tps=tps, cpad=cpad, nclass=nclass)

    def _conv_target(self, co: ConvOut, x1: Act, cout: int, dims, out: Optional[Act], f32_out, f32_strides,
                     ext_lo: int = 0) -> Optional[Act]:
        """Point `co` at the conv's output: the fp32 tensor `f32_out` with element strides (n, c, d, h, w), or an Act --
        `out`, or a new one of `dims` = (d, h, w) -- written from `ext_lo` slices below its own ones.  Returns the Act."""
        if f32_out is not None:
            co.y = f32_out.data_ptr()
            co.mode = 1
            co.sn, co.sc, co.sd, co.sh, co.sw = [int(v) for v in f32_strides]
            return None
        if out is None:
            out = self.act(x1.n, cout, *dims, halo=x1.halo)
        co.y = self.ext_ptr(out, ext_lo).value
        co.mode = 0
        co.cout_stride = out.c
        co.c_off = 0
        return out

    def _conv_setup(self, name: str, desc: ConvDesc, weight_fn, cin_w: Optional[int],
                    stream_tail: bool = False) -> _ConvPlan:
        """Everything one launch of ctsi_conv_fwd needs besides its operands: the plan of `desc`, what the emitters read
        of it, its split-K workspace and its weight image; counts the layer's flops under `name`."""
        lib, sptr = self.lib, self.ctx.sptr
        plan = C.c_void_p()
        lib.conv_plan_create(C.byref(plan), C.byref(desc))
        self.plans.append(plan)
        if cin_w is not None:
            lib.conv_plan_set_weight_cin(plan, cin_w)
        if stream_tail:
            lib.conv_plan_set_stream_tail(plan, 1)
        do, ho, wo, bm, bn, mode = (C.c_int() for _ in range(6))
        lib.conv_plan_out_dims(plan, C.byref(do), C.byref(ho), C.byref(wo))
        lib.conv_plan_config(plan, C.byref(bm), C.byref(bn), C.byref(mode))
        wbytes = lib.conv_plan_weight_bytes(plan)
        sig = _pack_sig(lib, plan, desc.transposed, (desc.kd, desc.kh, desc.kw), (desc.sh, desc.sw), desc.c1, desc.c2,
                        desc.cout, cin_w)
        holder = self._weight_image(weight_fn, sig, wbytes, lambda w, t: lib.conv_plan_pack_weights(plan, w, t, sptr), plan)
        fl = lib.conv_plan_flops(plan)
        self._count_conv(name, fl)
        workspace = self._conv_workspace(plan)
        return _ConvPlan(plan, desc, (do.value, ho.value, wo.value), wbytes, mode.value,
                         _conv_label(bm.value, bn.value, mode.value, desc, bool(workspace)), fl, lib.conv_plan_tiles(plan),
                         lib.conv_plan_tiles_per_sample(plan), lib.conv_plan_cout_pad(plan), workspace, holder)

    def _conv_launch(self, name: str, cp: _ConvPlan, x1p, x2p, bias, co: ConvOut, *, colsum_off: Optional[int] = None,
                     gn_slot: Optional[int] = None, audit: Optional[dict] = None):
        """Emit ctsi_conv_fwd of the layer set up as `cp` on the input views `x1p` / `x2p`, into the target `co` describes.
        `colsum_off`: where its column sums go (floats into the column-sum buffer; None: it writes none); `gn_slot`: the
        statistics the fused GroupNorm tail of `co` reads."""
        lib, sptr, prog, plan, holder, desc = self.lib, self.ctx.sptr, self, cp.plan, cp.holder, cp.desc
        co.workspace = cp.workspace
        self.keep.append(co)
        bp = _ptr(bias)

        def run():
            co.colsum = 0 if colsum_off is None else prog._colsum.data_ptr() + colsum_off * 4
            if gn_slot is not None:
                co.gn_sums = prog._gn_sums.data_ptr() + gn_slot * 8
            lib.conv_fwd(plan, x1p, x2p, _ptr(holder[0]), bp, C.byref(co), sptr)

        # algorithmic HBM bytes: inputs + weights + output (+ the tensor a fused GroupNorm tail reads), each once
        do, ho, wo = cp.out_dims
        out_elems = float(desc.n * do * ho * wo * desc.cout)
        alg = (2.0 * desc.n * desc.di * desc.hi * desc.wi * (desc.c1 + desc.c2) + float(cp.wbytes)
               + (4.0 if co.mode == 1 else 2.0) * out_elems + (2.0 * out_elems if co.gn_x else 0.0))
        self._emit(run, name, cp.flops, cp.kernel, alg_bytes=alg, audit=audit)

    def conv(self, name: str, weight_fn, bias_fn, x1: Act, x2: Optional[Act], *, transposed=False,
             k=(3, 3, 3), s=(1, 1), p=(1, 1, 1), cout: int, cin_w: Optional[int] = None,
             out: Optional[Act] = None, want_stats=False, f32_out: Optional[torch.Tensor] = None,
             f32_strides: Optional[Sequence[int]] = None, act: int = 0, fuse_gn=None, ext_out: bool = False,
             norm_in=None, audit: Optional[dict] = None):
        """Emit one convolution of [x1 | x2] (x2: the second half of a channel concatenation, never materialised).
        Returns (out_act, stats_handle).  The parameters both precisions take (engine_f32._F32Ops.conv is the fp32 form):
        `weight_fn` / `bias_fn` return the *current* fp32 parameter tensors (possibly derived, e.g. scaled or
            pre-multiplied; bias_fn may be None); `cin_w`: input channels the weights carry when the activation is padded.
        `transposed`, `k`, `s` (h, w), `p`, `cout`: the layer's geometry.
        `out`: write into this Act instead of a new one.  `f32_out` + `f32_strides` (element strides n, c, d, h, w): store
            fp32 into that tensor instead (out_act is None).  `act`: the epilogue's activation (1 = tanh).
        `want_stats`: also write per-tile column sums; the stats handle is what gn_finalize takes.
        `norm_in` = (slot, gn: nn.GroupNorm, silu: bool, tb) with tb = None or (tbias, tbias_off, tbias_stride, step_ptr):
            x1 is the RAW output of the previous conv and this conv's input is silu?(gn(x1)) + tbias: the normalisation is
            emitted as its own in-place pass first (depth-sharded: its statistics travel with the raw boundary slices in
            one sync point), so x1 must not be used raw afterwards.  (A normalise-on-load variant of the 512-voxel kernel
            that applied it to the staged tile in LDS was bit-identical but slower: csrc/experiments/conv3_halo_m512.hip.)
        bf16 only (the fp32 form rejects them):
        `fuse_gn` = (h: Act, slot, gn: nn.GroupNorm, silu: bool): the epilogue stores silu?(gn(h) + conv result) instead of
            the conv result (ctsi_conv_out.gn_x; h may be the output buffer itself).
        `ext_out`: a pointwise conv over inputs with valid halo slices covers them too.
        `audit`: replaces the op's audit record (the training programs' data-gradient convs).
        fp32 only: `residual` (an fp32 Act of the output's shape), added in the epilogue."""
        nin_synced = False
        if norm_in is not None and self.shard is not None and x1.halo:
            # depth-sharded: statistics + RAW boundary slices in one sync point, whichever way the normalisation happens
            self.sync_stats_and_halos(x1, norm_in[0], x1.n * norm_in[1].num_groups * 2)
            nin_synced = True
        deep = k[0] > 1 and x1.halo == 1   # depth taps read the halo slices: "valid" conv along depth
        if x1.halo and x1.n != 1:
            raise CtsiError("a depth-sharded program holds one volume (batches run volume by volume, see "
                            "sampler.run_sampler_sharded)")
        if (deep and self.shard is not None and getattr(self.shard, "overlap", True)
                and (self.shard.world > 1 or self.shard.overlap == "force")
                and (x1.dirty or (x2 is not None and x2.dirty)) and min(self.shard.depth_counts) >= 3 and not transposed and tuple(s) == (1, 1)
                and f32_out is None and fuse_gn is None and norm_in is None and not ext_out and out is None and act == 0):
            return self._conv_overlapped(name, weight_fn, bias_fn, x1, x2, k, p, cout, cin_w, want_stats)
        if deep:
            self.halo_exchange(x1)
            if x2 is not None:
                self.halo_exchange(x2)
        # a pointwise conv whose inputs carry valid halo slices may cover them too (`ext_out`): its output then has valid
        # halos without an exchange of its own (the fused residual tail of a sharded ResBlock)
        ext_lo, ext_d = (0, x1.d)
        if ext_out:
            if deep or x1.dirty or (x2 is not None and x2.dirty):
                raise CtsiError("internal: ext_out needs a pointwise conv over inputs with valid halo slices")
            ext_lo, ext_d = self.ext(x1)
        if norm_in is not None:
            self._norm_in_pass(x1, norm_in, nin_synced)
        bias = self._conv_bias(bias_fn)
        desc = ConvDesc(int(transposed), k[0], k[1], k[2], s[0], s[1], p[0], p[1], p[2], x1.n, x1.c,
                        0 if x2 is None else x2.c, cout, x1.d + 2 if deep else ext_d, x1.h, x1.w, 1 if deep else 0)
        # the ResBlock tails are HBM-bound passes: the streaming kernel where the layer qualifies (csrc/conv1_stream.hip)
        tail = fuse_gn is not None and tuple(k) == (1, 1, 1) and f32_out is None and not want_stats and act == 0
        cp = self._conv_setup(name, desc, weight_fn, cin_w, stream_tail=tail)
        do, ho, wo = cp.out_dims
        stats = self._conv_stats(cp.tiles, cp.tps, cp.cpad, 4 if transposed else 1) if want_stats else None
        co = ConvOut()
        out_act = self._conv_target(co, x1, cout, (do - (ext_d - x1.d), ho, wo), out, f32_out, f32_strides, ext_lo)
        if out_act is not None:
            out_act.dirty = not ext_out
        co.act = act
        prog = self
        if fuse_gn is not None:
            gh, gslot, gmod, gsilu = fuse_gn
            if f32_out is not None or want_stats or (gh.n, gh.c, gh.d, gh.h, gh.w) != (x1.n, cout, out_act.d, ho, wo):
                raise CtsiError("internal: fused GroupNorm tail needs a bf16 output of the normalised tensor's shape")
            ggamma = self.dev_f32(lambda: gmod.weight)
            gbeta = self.dev_f32(lambda: gmod.bias)
            d_stat = self.shard.depth_total if (self.shard is not None and gh.halo) else gh.d
            co.gn_x = self.ext_ptr(gh, ext_lo).value
            co.gn_gamma, co.gn_beta = ggamma.data_ptr(), gbeta.data_ptr()
            co.gn_groups, co.gn_eps = gmod.num_groups, float(gmod.eps)
            co.gn_count = (cout // gmod.num_groups) * d_stat * gh.h * gh.w
            co.gn_silu = int(gsilu)
        if audit is not None:
            audit = dict(audit, out=out_act)
        else:
            audit = dict(kind="conv_fwd", x1=x1, x2=x2, weight=weight_fn, bias=bias, transposed=bool(transposed), k=tuple(k),
                         s=tuple(s), p=tuple(p), cout=cout, cin_w=cin_w, act=act, out=out_act, f32_out=f32_out,
                         f32_strides=None if f32_out is None else tuple(int(v) for v in f32_strides), stats=stats,
                         colsum=(lambda: prog._colsum) if want_stats else None, stream_tail=cp.mode == 10, fuse_gn=None)
            if fuse_gn is not None:
                audit["fuse_gn"] = dict(x=gh, slot=gslot, sums=lambda: prog._gn_sums, gamma=ggamma, beta=gbeta,
                                        groups=gmod.num_groups, eps=float(gmod.eps), count=int(co.gn_count), silu=bool(gsilu))
        x1p = x1.fp if deep else self.ext_ptr(x1, ext_lo)
        x2p = C.c_void_p(0) if x2 is None else (x2.fp if deep else self.ext_ptr(x2, ext_lo))
        self._conv_launch(name, cp, x1p, x2p, bias, co, colsum_off=0 if want_stats else None,
                          gn_slot=fuse_gn[1] if fuse_gn is not None else None, audit=audit)
        return out_act, stats

    def _conv_overlapped(self, name, weight_fn, bias_fn, x1: Act, x2: Optional[Act], k, p, cout, cin_w, want_stats):
        """A depth-3 stride-1 conv whose input still needs its plain halo exchange (tensors no GroupNorm follows: conv_in /
        Downsample / Upsample outputs, the sampler's updated input): the transfer runs on the context's second stream while
        the INTERIOR output slices -- which read own slices only -- are computed; the two BOUNDARY slices follow the join
        (SURVEY section 7-10).  Three launches of the same layer on three views of the same buffers:
            interior  input = the d own slices taken as a halo'd tensor   -> output slices 1 .. d-2
            lower     input = [lo halo, own 0, own 1]                     -> output slice 0
            upper     input = [own d-2, own d-1, hi halo]                 -> output slice d-1"""
        lib, sptr = self.lib, self.ctx.sptr
        spec = self.shard
        cs = self.ctx.comm_stream_ptr()
        ev_fork, ev_join = C.c_void_p(), C.c_void_p()
        lib.event_create(C.byref(ev_fork))
        lib.event_create(C.byref(ev_join))
        self._events += [ev_fork, ev_join]
        todo = [a for a in (x1, x2) if a is not None and a.halo and a.dirty]
        sl = [self._slices(a) for a in todo]
        for a in todo:
            a.dirty = False

        def run_fork():
            lib.event_record(ev_fork, sptr)                 # the producer of the boundary slices is done ...
            lib.stream_wait_event(cs, ev_fork)              # ... before the transfer starts, on the second stream
            for (lo_own, hi_own, lo_halo, hi_halo) in sl:
                spec.comm.exchange(spec.rank, lo_own, hi_own, lo_halo, hi_halo, sptr=cs)
            lib.event_record(ev_join, cs)

        def run_join():
            lib.stream_wait_event(sptr, ev_join)            # halos have landed: the boundary slices may be computed

        self._emit(run_fork, "halo.exchange.async", 0.0, "comm")
        d, se_in1 = x1.d, x1.slice_elems * 2
        c2, se_in2 = (0, 0) if x2 is None else (x2.c, x2.slice_elems * 2)
        out = self.act(x1.n, cout, d, x1.h, x1.w, halo=x1.halo)
        out.dirty = True
        se_out = out.slice_elems * 2
        bias = self._conv_bias(bias_fn)
        parts, col_off = [], 0
        views = [("interior", d, x1.ip.value, 0 if x2 is None else x2.ip.value, out.ip.value + se_out),
                 ("lower", 3, x1.fp.value, 0 if x2 is None else x2.fp.value, out.ip.value),
                 ("upper", 3, x1.ip.value + (d - 2) * se_in1, 0 if x2 is None else x2.ip.value + (d - 2) * se_in2,
                  out.ip.value + (d - 1) * se_out)]
        for tag, di, p1, p2, py in views:
            if tag == "lower":
                self._emit(run_join, "halo.join", 0.0, "comm.join")
            desc = ConvDesc(0, k[0], k[1], k[2], 1, 1, p[0], p[1], p[2], x1.n, x1.c, c2, cout, di, x1.h, x1.w, 1)
            cp = self._conv_setup(name + "." + tag, desc, weight_fn, cin_w)
            if want_stats:
                parts.append(dict(self._conv_stats(cp.tiles, cp.tps, cp.cpad, 1, col_off), off=col_off))
            co = ConvOut()
            co.y, co.mode, co.cout_stride, co.c_off = py, 0, cout, 0
            self._conv_launch(name + "." + tag, cp, C.c_void_p(p1), C.c_void_p(p2), bias, co,
                              colsum_off=col_off if want_stats else None)
            col_off += 2 * cp.tiles * cp.cpad
        return out, (dict(parts=parts) if want_stats else None)

    # ---- GroupNorm ----------------------------------------------------------------------------------------
    def _gn_slot(self, n, groups) -> int:
        off = self.gn_slots
        self.gn_slots += n * groups * 2
        return off

    def gn_finalize(self, x: Act, groups: int, stats: dict) -> int:
        """colsum slab(s) (already written by the producer) -> fp64 sums slot; returns the slot offset.  A tensor produced
        by several launches (`stats["parts"]`: the interior / boundary split of a depth-sharded conv) is finalised slab by
        slab, the later ones accumulating (ordered on the stream: still deterministic)."""
        slot = self._gn_slot(x.n, groups)
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        n, c = x.n, x.c
        parts = stats.get("parts") or [dict(tps=stats["tps"], cpad=stats["cpad"], nclass=stats["nclass"], off=0)]

        def run():
            for i, pt in enumerate(parts):
                lib.gn_finalize(C.c_void_p(prog._colsum.data_ptr() + pt["off"] * 4),
                                C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), n, c, pt["cpad"], groups, pt["tps"],
                                pt["nclass"], int(i > 0), sptr)

        self._emit(run, "gn.finalize", audit=dict(kind="gn_finalize", colsum=lambda: prog._colsum, sums=lambda: prog._gn_sums,
                                                  slot=slot, n=n, c=c, groups=groups, parts=parts))
        # depth-sharded programs: the slot holds this slab's sums until `sync_stats_and_halos` (emitted by the consumer:
        # gn_apply / attention / the fused residual tail) all-reduces it together with the tensor's boundary slices
        return slot

    def gn_colsum(self, x: Act) -> dict:
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        tps = lib.gn_colsum_tiles(x.d, x.h, x.w)
        self._colsum_need = max(self._colsum_need, 2 * x.n * tps * x.c)
        xp = x.ip
        n, c, d, h, w = x.n, x.c, x.d, x.h, x.w

        def run():
            lib.gn_colsum(xp, _ptr(prog._colsum), n, c, d, h, w, None, sptr)

        self._emit(run, "gn.colsum", nbytes=2.0 * n * c * d * h * w,
                   audit=dict(kind="gn_colsum", x=x, colsum=lambda: prog._colsum, tps=tps, tile_rows=512))
        return dict(tps=tps, cpad=x.c, nclass=1)

    def gn_apply(self, x: Act, slot: int, gn: nn.GroupNorm, *, silu_pre: bool, tbias=None,
                 tbias_off: int = 0, tbias_stride: int = 0, step_ptr: Optional[torch.Tensor] = None,
                 residual: Optional[Act] = None, silu_post: bool = False, out: Optional[Act] = None,
                 synced: bool = False, film: bool = False, drop=None) -> Act:
        """y = [silu](gn(x)) [+ tbias] [+ residual] [silu].  Depth-sharded: first the sync point that all-reduces the
        statistics and exchanges x's RAW boundary slices (unless `synced`: the caller already did), then the
        normalisation over own + received halo slices -- y's halos are valid without an exchange of its own.
        `film` / `drop` (the ResBlock's middle pass only) emit ctsi_gn_apply_mod instead: film: the time row
        holds (s | b) and y = silu(gn(x) * (1 + s) + b); drop = (state, layer_id): dropout with the threshold, scale and seed
        buffer of `state` (norm_mod.DropoutState, read at launch time).  Neither given: the default launch, as ever."""
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        if film or drop is not None:
            if self.shard is not None:
                raise CtsiError("use_scale_shift_norm / dropout do not support depth sharding")
            if tbias is None or residual is not None or silu_post or not silu_pre:
                raise CtsiError("internal: the scale-shift / dropout pass is the ResBlock's middle pass only")
        if self.shard is not None and not synced:
            self.sync_stats_and_halos(x if x.halo else None, slot, x.n * gn.num_groups * 2)
        if residual is not None and self.shard is not None and residual.halo:
            self.halo_exchange(residual)     # (already valid in the networks of this repo: a no-op)
        lo, d_ext = self.ext(x)
        gamma = self.dev_f32(lambda: gn.weight)
        beta = self.dev_f32(lambda: gn.bias)
        self.track(gn.weight, gn.bias)
        fresh = out is None
        if out is None:
            out = self.act(x.n, x.c, x.d, x.h, x.w, halo=x.halo)
        out.dirty = bool(self.shard is not None and x.halo and x.dirty)
        xp, yp, gp, bp = self.ext_ptr(x, lo), self.ext_ptr(out, lo), _ptr(gamma), _ptr(beta)
        tbp = C.c_void_p(0 if tbias is None else tbias.data_ptr() + tbias_off * 4)
        stp = _ptr(step_ptr)
        rp = C.c_void_p(0) if residual is None else self.ext_ptr(residual, lo)
        n, c, h, w, groups, eps = x.n, x.c, x.h, x.w, gn.num_groups, float(gn.eps)
        d_stat = self.shard.depth_total if (self.shard is not None and x.halo) else x.d   # statistics span all ranks
        d = d_ext

        def run():
            lib.gn_apply(xp, yp, C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), gp, bp, n, c, d, h, w, d_stat,
                         groups, eps, int(silu_pre), tbp, tbias_stride, stp, rp, int(silu_post), sptr)

        if film or drop is not None:
            from .norm_mod import emit_gn_apply_mod
            emit_gn_apply_mod(self, xp=xp, yp=yp, slot=slot, gp=gp, bp=bp, n=n, c=c, d=d, h=h, w=w, d_stat=d_stat, groups=groups,
                              eps=eps, tbp=tbp, tbias_stride=tbias_stride, stp=stp, film=film, drop=drop,
                              record=dict(x=x, out=out, sums=lambda: prog._gn_sums, slot=slot, gamma=gamma, beta=beta,
                                          groups=groups, eps=eps, d_stat=d_stat, silu_pre=True, tbias=tbias,
                                          tbias_off=tbias_off, tbias_stride=tbias_stride, step_ptr=step_ptr))
            if fresh:
                self.zero_end_halos(out)
            return out
        self._emit(run, "gn.apply", nbytes=(2 + (residual is not None)) * 2.0 * n * c * d * h * w,
                   audit=dict(kind="gn_apply", x=x, out=out, sums=lambda: prog._gn_sums, slot=slot, gamma=gamma, beta=beta,
                              groups=groups, eps=eps, d_stat=d_stat, silu_pre=bool(silu_pre), tbias=tbias, tbias_off=tbias_off,
                              tbias_stride=tbias_stride, step_ptr=step_ptr, residual=residual, silu_post=bool(silu_post)))
        if fresh:
            self.zero_end_halos(out)
        return out

    # ---- U-Net blocks ------------------------------------------------------------------------------------
    def unet_resblock(self, m, x: Act, skip: Optional[Act], tbias: torch.Tensor, tbias_off: int,
                      tbias_stride: int, step_ptr: Optional[torch.Tensor]) -> Act:
        """ResBlock3D of the U-Net (models/unet3d.py:116-133); `skip` is the second half of a
        channel concatenation feeding the block (never materialised)."""
        cout = m.conv1.conv.out_channels
        has_res_conv = not isinstance(m.residual_conv, nn.Identity)
        if not has_res_conv and skip is not None:
            raise CtsiError("identity residual with a concatenated input")
        c1, st = self.conv("rb.conv1", lambda: m.conv1.conv.weight, lambda: m.conv1.conv.bias, x, skip,
                           cout=cout, want_stats=True)
        slot = self.gn_finalize(c1, m.conv1.norm.num_groups, st)
        # conv2 consumes silu(gn(c1)) + time bias: normalised on load where the plan supports it (c1 is never rewritten)
        c2, st = self.conv("rb.conv2", lambda: m.conv2[0].weight, lambda: m.conv2[0].bias, c1, None, cout=cout,
                           want_stats=True,
                           norm_in=(slot, m.conv1.norm, True, (tbias, tbias_off, tbias_stride, step_ptr))
                           + ((True,) if getattr(m, "scale_shift", False) else ()))
        self.release(c1)
        slot = self.gn_finalize(c2, m.conv2[1].num_groups, st)
        if not has_res_conv:
            return self.gn_apply(c2, slot, m.conv2[1], silu_pre=False, residual=x, silu_post=True, out=c2)
        if os.environ.get("CTSI_NO_FUSE_RES"):   # tuning / test aid: residual conv and GroupNorm tail as two launches
            if self.shard is not None:
                for a in (x, skip):
                    if a is not None:
                        self.halo_exchange(a)
            r, _ = self.conv("res1x1", lambda: m.residual_conv.weight, lambda: m.residual_conv.bias, x, skip,
                             k=(1, 1, 1), p=(0, 0, 0), cout=cout, ext_out=self.shard is not None)
            out = self.gn_apply(c2, slot, m.conv2[1], silu_pre=False, residual=r, silu_post=True, out=c2)
            self.release(r)
            return out
        # block tail with a 1x1x1 residual conv: out = silu(gn(c2) + W_r [x | skip] + b_r) in ONE launch -- the conv's
        # epilogue applies the GroupNorm of c2 and the activation, so the residual tensor never goes to HBM
        if self.shard is not None:
            self.sync_stats_and_halos(c2, slot, c2.n * m.conv2[1].num_groups * 2)
            for a in (x, skip):
                if a is not None:
                    self.halo_exchange(a)    # valid already (a no-op) for every block of the U-Net
        out, _ = self.conv("res1x1+gn", lambda: m.residual_conv.weight, lambda: m.residual_conv.bias, x, skip,
                           k=(1, 1, 1), p=(0, 0, 0), cout=cout, out=c2, fuse_gn=(c2, slot, m.conv2[1], True),
                           ext_out=self.shard is not None)
        return out

    def attention_softmax(self, m, x: Act, save: bool = False):
        """TemporalAttention as true attention over depth (attention.py); returns (y, saved)."""
        return emit_softmax_attention(self, m, x, save)

    def attention(self, m, x: Act, mode: str = "fast") -> Act:
        """TemporalAttention (models/unet3d.py:163-194), see csrc/attention.hip; mode 'softmax': attention_softmax."""
        check_attention_mode(mode)
        if mode == "softmax":
            return self.attention_softmax(m, x)[0]
        lib, sptr, prog = self.lib, self.ctx.sptr, self
        n, c, d, h, w = x.n, x.c, x.d, x.h, x.w
        dev = self.ctx.device
        heads = m.num_heads
        tps = lib.attn_depthsum_tiles(c, h, w)
        self._colsum_need = max(self._colsum_need, 2 * n * tps * c)
        depthsum = self.pool.get(n * h * w * c, torch.float32)
        xp, dsp = x.ip, _ptr(depthsum)
        world = self.shard.world if (self.shard is not None and x.halo) else 1
        d_all = self.shard.depth_total if (self.shard is not None and x.halo) else d

        def run_ds():
            lib.attn_depthsum(xp, dsp, _ptr(prog._colsum), n, c, d, h, w, sptr)

        self._emit(run_ds, "attn.depthsum", nbytes=2.0 * n * c * d * h * w,
                   audit=dict(kind="attn_depthsum", x=x, depthsum=depthsum, colsum=lambda: prog._colsum, tps=tps,
                              tile_pos=256 // (c // 8)))
        slot = self.gn_finalize(x, m.norm.num_groups, dict(tps=tps, cpad=c, nclass=1))
        if self.shard is not None and x.halo:
            # one sync point: GroupNorm statistics (fp64) + the depth sum (fp32) over all ranks
            self.sync_stats_and_halos(None, slot, n * m.norm.num_groups * 2, f32=depthsum, name="attn.sync")
            self.halo_exchange(x)        # the block's input (valid already in this repo's networks: a no-op)
        gamma = self.dev_f32(lambda: m.norm.weight)
        beta = self.dev_f32(lambda: m.norm.bias)
        groups, eps = m.norm.num_groups, float(m.norm.eps)
        gp, bp = _ptr(gamma), _ptr(beta)

        # fold proj_out . V-projection:  P = (Wp Wv) xs + (D Wp bv + bp)
        def wv():
            return m.qkv.weight[2 * c:3 * c, :, 0, 0, 0].double()

        def wpv():
            wp = m.proj_out.weight[:, :, 0, 0, 0].double()
            return (wp @ wv()).float().reshape(c, c, 1, 1, 1)

        def bpv():
            wp = m.proj_out.weight[:, :, 0, 0, 0].double()
            return (float(d_all) * (wp @ m.qkv.bias[2 * c:3 * c].double()) + m.proj_out.bias.double()).float()

        if lib.attn_pv_supported(c, groups) and not os.environ.get("CTSI_NO_ATTN_PV"):
            # one launch: normalise the depth sum in registers and multiply by the folded matrix (csrc/attention.hip)
            wbuf = self.persistent((c, c), torch.bfloat16)
            self.pack_fns.append(lambda: wbuf.copy_(wpv().reshape(c, c).to(device=dev, dtype=torch.bfloat16)))
            bias_pv = self.dev_f32(bpv)
            pterm = self.act(n, c, 1, h, w, halo=0)
            wp_, bpp, ptp = _ptr(wbuf), _ptr(bias_pv), _ptr(pterm.t)

            def run_pv():
                lib.attn_pv(dsp, C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), gp, bp, wp_, bpp, ptp, n, c, d_all, h, w,
                            groups, eps, sptr)

            fl_pv = 2.0 * n * h * w * c * c
            self.flops += fl_pv
            self._emit(run_pv, "attn.pv", fl_pv, "attn_pv_mfma",
                       audit=dict(kind="attn_pv", depthsum=depthsum, sums=lambda: prog._gn_sums, slot=slot, gamma=gamma,
                                  beta=beta, w=wbuf, bias=bias_pv, out=pterm, groups=groups, eps=eps, d=d_all))
            self.pool.put(depthsum)
        else:
            xs = self.act(n, c, 1, h, w, halo=0)
            xsp = _ptr(xs.t)

            def run_ns():
                lib.attn_normsum(dsp, C.c_void_p(prog._gn_sums.data_ptr() + slot * 8), gp, bp, xsp, n, c, d_all, h, w,
                                 groups, eps, sptr)

            self._emit(run_ns, "attn.normsum",
                       audit=dict(kind="attn_normsum", depthsum=depthsum, sums=lambda: prog._gn_sums, slot=slot, gamma=gamma,
                                  beta=beta, out=xs, groups=groups, eps=eps, d=d_all))
            pterm, _ = self.conv("attn.pv", wpv, bpv, xs, None, k=(1, 1, 1), p=(0, 0, 0), cout=c)
            self.pool.put(depthsum)
            self.release(xs)
        rowsum = None
        if mode == "exact":
            # evaluate the softmax row sums the reference multiplies in (they equal 1 up to rounding)
            xn = self.gn_apply(x, slot, m.norm, silu_pre=False)
            qk, _ = self.conv("attn.qk", lambda: m.qkv.weight[:2 * c], lambda: m.qkv.bias[:2 * c], xn, None,
                              k=(1, 1, 1), p=(0, 0, 0), cout=2 * c)
            self.release(xn)
            if world > 1:
                raise CtsiError("exact-mode attention needs every key on one rank; use the fast mode when sharding")
            rowsum = self.pool.get(n * d * h * w * heads, torch.float32)
            qkp, rsp = qk.ip, _ptr(rowsum)

            def run_rs():
                lib.attn_softmax_rowsum(qkp, rsp, n, c, d, h, w, heads, sptr)

            self._emit(run_rs, "attn.softmax_rowsum",
                       audit=dict(kind="attn_softmax_rowsum", qk=qk, out=rowsum, heads=heads))
            self.release(qk)
        out = self.act(n, c, d, h, w, halo=x.halo)
        lo, d_ext = self.ext(x)          # x + P over own AND halo slices: P does not depend on depth
        out.dirty = False
        pp, op_, rsp2 = pterm.ip, self.ext_ptr(out, lo), _ptr(rowsum)
        xep = self.ext_ptr(x, lo)

        def run_ba():
            lib.attn_broadcast_add(xep, pp, rsp2, heads, op_, n, c, d_ext, h, w, sptr)

        self._emit(run_ba, "attn.broadcast_add", nbytes=4.0 * n * c * d_ext * h * w,
                   audit=dict(kind="attn_broadcast_add", x=x, p=pterm, rowsum=rowsum, heads=heads, out=out))
        self.zero_end_halos(out)
        self.release(pterm)
        if rowsum is not None:
            self.pool.put(rowsum)
        return out

    # ---- finish layout / execution ----------------------------------------------------------------------------
    def finalize_layout(self):
        dev = self.ctx.device
        self._colsum = torch.empty(max(self._colsum_need, 1), dtype=torch.float32, device=dev)
        self._gn_sums = torch.zeros(max(self.gn_slots, 1), dtype=torch.float64, device=dev)
        self.repack()

    def zero_gn_op(self):
        """Kept for the program builders' call sites: ctsi_gn_finalize WRITES its (sum, sumsq) slots (one block per
        (sample, group), fixed-order reduce), so the statistics buffer needs no per-evaluation zeroing any more."""

    def run(self):
        for op in self.ops:
            op()

    def profile_ops(self, repeats: int = 1):
        """Eager run with a HIP event pair around every op (on the engine stream).  Returns a list of
        (name, kernel, flops, milliseconds) — used by bench.py for the live roofline figure."""
        lib, sptr = self.lib, self.ctx.sptr
        nops = len(self.ops)
        evs = []
        for _ in range(nops + 1):
            e = C.c_void_p()
            lib.event_create(C.byref(e))
            evs.append(e)
        acc = [0.0] * nops
        for _ in range(repeats):
            lib.event_record(evs[0], sptr)
            for i, op in enumerate(self.ops):
                op()
                lib.event_record(evs[i + 1], sptr)
            for i in range(nops):
                ms = C.c_float()
                lib.event_elapsed_ms(evs[i], evs[i + 1], C.byref(ms))
                acc[i] += ms.value
        for e in evs:
            lib.event_destroy(e)
        return [(m[0], m[2], m[1], acc[i] / repeats) for i, m in enumerate(self.op_meta)]

    def capture(self):
        lib = self.lib
        lib.graph_begin_capture(self.ctx.sptr)
        try:
            self.run()
        finally:
            g = C.c_void_p()
            lib.graph_end_capture(self.ctx.sptr, C.byref(g))
        self.graph = g

    def launch(self):
        if self.graph is None:
            self.run()
        else:
            self.lib.graph_launch(self.graph, self.ctx.sptr)

    def __del__(self):
        try:
            if self.graph is not None:
                self.lib.graph_destroy(self.graph)
            for p in self.plans:
                self.lib.conv_plan_destroy(p)
            for ev in self._events:
                self.lib.event_destroy(ev)
            if self._fast and self._fast.get("graph") is not None:
                self.lib.graph_destroy(self._fast["graph"])
        except Exception:
            pass


class PhasedProgram(Program):
    """A program built as a forward followed by a backward and replayed one half at a time (the training programs, the
    differentiable decode, the VGG / LPIPS loss).  `ops[:n_fwd]` is the forward.  It overwrites the activations the backward
    reads, so every forward bumps `generation` and a backward names the generation it belongs to: one that belongs to an
    EARLIER forward fails loudly instead of differentiating through the wrong activations
    (l1 = model(a); l2 = model(b); (l1 + l2).backward())."""
    stale_msg = ""     # the CtsiError text of such a backward; may name {then} and {now}

    def __init__(self, ctx: Ctx):
        super().__init__(ctx)
        self.n_fwd = 0
        self.generation = 0

    def end_forward(self):
        """Build time: every op emitted so far is the forward, whatever follows the backward."""
        self.n_fwd = len(self.ops)

    def forward_ops(self, load: Optional[Callable[[], None]] = None):
        """Refresh the weight images, start a new generation, `load()` the inputs and run the forward."""
        self.ensure_fresh()
        self.generation += 1
        if load is not None:
            load()
        for op in self.ops[:self.n_fwd]:
            op()

    def backward_ops(self, generation: Optional[int], load: Optional[Callable[[], None]] = None):
        """Run the backward of the forward that started `generation` (None: unchecked), after `load()` took the incoming
        gradients; nothing is touched when that forward's activations are gone."""
        if generation is not None and generation != self.generation:
            raise CtsiError(self.stale_msg.format(then=generation, now=self.generation))
        if load is not None:
            load()
        for op in self.ops[self.n_fwd:]:
            op()


# ==========================================================================================================
# U-Net
# ==========================================================================================================
class SamplerStep(NamedTuple):
    """How a sampler kind's update is called: the ctsi_<entry> / ctsi_<entry>_f32 pair and its optional operands."""
    entry: str
    noise: bool         # takes the fp32 NCDHW noise (may still be NULL at run time)
    hist: bool          # takes a persistent fp32 NDHWC history buffer of z's shape
    nonfinite: bool     # takes the nonfinite table
    vraw: bool = False  # takes the variance channels of a learn_sigma model (fp32 NDHWC of z's shape; NULL: fixed-small)


# Every sampler update.  A new sampler adds one row here and one branch in sampler._step_plan.
SAMPLER_STEPS = {
    "ddim": SamplerStep("ddim_step", noise=True, hist=False, nonfinite=True),
    "ddpm": SamplerStep("ddpm_step", noise=True, hist=False, nonfinite=False),
    "dpmpp": SamplerStep("dpm_step", noise=False, hist=True, nonfinite=True),      # history: x0_{i-1}
    "heun": SamplerStep("heun_step", noise=True, hist=True, nonfinite=True),       # history: the predictor's D1
}
# Additive kinds (not in the reference's loops).  'ddpm_lv': the ancestral step on respaced rows, with the learned or the
# fixed-small variance.
EXTRA_SAMPLER_STEPS = {
    "ddpm_lv": SamplerStep("ddpm_lv_step", noise=True, hist=False, nonfinite=False, vraw=True),
}


def sampler_step_row(kind: str) -> SamplerStep:
    return SAMPLER_STEPS[kind] if kind in SAMPLER_STEPS else EXTRA_SAMPLER_STEPS[kind]


def sampler_step_launcher(lib, kind: str, f32: bool) -> Callable:
    """The update of `kind` behind one argument list, (z, eps, hist, noise, zin, c_total, coef, step_ptr, n, L, d, h,
    w, nonfinite, stream, vraw=None); operands the entry does not take are dropped.  `f32`: the entry that writes an fp32 zin."""
    s = sampler_step_row(kind)
    fn = getattr(lib, s.entry + ("_f32" if f32 else ""))

    def launch(z, eps, hist, noise, zin, c_total, coef, step_ptr, n, L, d, h, w, nonfinite, stream, vraw=None):
        ops = [z, eps] + ([vraw] if s.vraw else []) + ([hist] if s.hist else []) + ([noise] if s.noise else [])
        tail = [nonfinite] if s.nonfinite else []
        fn(*ops, zin, c_total, 0, coef, step_ptr, n, L, d, h, w, *tail, stream)
    return launch


class UNetProgram(Program):
    """One U-Net evaluation (models/unet3d.py:357-413) at a fixed latent shape, followed optionally by
    a sampler update; `step_ptr` selects the timestep row, so one captured graph serves all steps.

    `guided` (classifier-free guidance): the network runs at batch 2n -- rows [0, n) on the
    conditioning, rows [n, 2n) on the null conditioning, the all-zero latent -- and add_sampler_step puts ctsi_cfg_combine
    between the network and the update and ctsi_cfg_mirror behind it.  z, hist, noise, the nonfinite table and
    z_ncdhw() / eps_ncdhw() stay n-sized; timestep rows are per (evaluation, network row): 2n per evaluation.
    `rescale` adds the statistics pass of the guidance rescale (phi > 0).

    `prediction`: 'epsilon' (default: the program is what it always was) or 'v_prediction' -- the network
    output is v, and add_sampler_step puts one ctsi_pred_to_eps launch over all network rows between the network and
    everything that reads eps (guidance, update, counters, eps_ncdhw()); its rows sit in `pred_rows`, one per evaluation."""

    def __init__(self, ctx: Ctx, unet, n: int, d: int, h: int, w: int, max_rows: int, attention_mode="fast",
                 shard=None, guided: bool = False, rescale: bool = False, prediction: str = "epsilon"):
        """`d` is the depth this program owns: the whole volume on one GPU, or the rank's slab of
        `shard.depth_total // shard.world` slices when `shard` (parallel.ShardSpec) is given."""
        super().__init__(ctx)
        self.shard = shard
        if shard is not None and n != 1:
            raise CtsiError("depth-sharded programs support one volume per rank")
        if shard is not None and guided:
            raise CtsiError("classifier-free guidance does not support depth sharding: the sharded program holds one "
                            "volume per rank and the rescale statistics would need a collective")
        check_resblock_options_unsharded(unet, shard is not None)
        check_learn_sigma_unsharded(unet, shard is not None)
        check_spatial_attention_supported(unet, getattr(self, "precision", "bf16"), shard is not None)
        self.unet = unet
        self.learn_sigma = bool(getattr(unet, "learn_sigma", False))      # a 2L-channel head
        self.guided, self.rescale = bool(guided), bool(guided and rescale)
        self.prediction = check_prediction_type(prediction)
        self.n, self.d, self.h, self.w = n, d, h, w
        n = self.nb = 2 * n if guided else n        # the network's batch; self.n stays the number of samples
        L = unet.latent_dim
        self.L = L
        dev = ctx.device
        self.attention_mode = check_attention_mode(attention_mode)
        self.max_rows = max_rows
        halo = 0 if shard is None else 1
        self.xin, self.xin2 = self._input_acts(n, d, h, w, halo)
        self.eps = self.persistent((n, d, h, w, L), torch.float32)
        # learn_sigma: the head writes `out2`, ctsi_sigma_split packs its first half into `eps`; `vraw` (the variance channels
        # of rows [0, self.n)) exists once a step that reads it is added
        self.out2 = self.persistent((n, d, h, w, 2 * L), torch.float32) if self.learn_sigma else None
        self.vraw = None
        self.z = self.persistent((self.n, d, h, w, L), torch.float32, zero=True)
        self.step_ptr = self.persistent((1,), torch.int32, zero=True)
        self.t_rows = self.persistent((max_rows,), torch.int32, zero=True)
        self.t_rows_f = self.persistent((max_rows,), torch.float32, zero=True)   # fractional timesteps (EDM sampler)
        self.coef = self.persistent((max_rows, 8), torch.float32, zero=True)
        self.noise = None  # fp32 NCDHW, allocated on demand
        self.guide_z = None  # fp32 NDHWC like z: the state a guided evaluation saves before the replay (guide_scratch)
        self.track_module(unet)

        # ---- time embedding: stack every ResBlock's Linear(time_dim -> cout) -------------------------
        te = unet.time_embed.time_mlp
        self.dim = unet.model_channels
        self.time_dim = te[1].out_features
        blocks = [m for m in unet.modules() if type(m).__name__ == "ResBlock3D"]
        self.tb_off = {}
        off = 0
        for m in blocks:
            self.tb_off[id(m)] = off
            off += m.time_mlp[1].out_features
        self.total_out = off
        self.w1 = self.dev_f32(lambda: te[1].weight)
        self.b1 = self.dev_f32(lambda: te[1].bias)
        self.w2 = self.dev_f32(lambda: te[3].weight)
        self.b2 = self.dev_f32(lambda: te[3].bias)
        self.w_all = self.dev_f32(lambda: torch.cat([m.time_mlp[1].weight for m in blocks], 0))
        self.b_all = self.dev_f32(lambda: torch.cat([m.time_mlp[1].bias for m in blocks], 0))
        self.tbias = self.persistent((max_rows, self.total_out), torch.float32, zero=True)
        self.te_scratch = self.persistent((max_rows * (self.dim + 2 * self.time_dim),), torch.float32)

        # ---- network ------------------------------------------------------------------------------------
        self.zero_gn_op()
        x, _ = self.conv("conv_in", lambda: unet.conv_in.weight, lambda: unet.conv_in.bias, self.xin, self.xin2,
                         cout=unet.conv_in.out_channels)
        skips: List[Act] = []

        def step(layer, xcur: Act, skip: Optional[Act] = None) -> Act:
            ynew = self._layer(layer, xcur, skip)
            if not any(xcur is sk for sk in skips):
                self.release(xcur)
            if skip is not None:
                self.release(skip)
            return ynew

        for level_blocks, down in zip(unet.down_blocks, unet.down_samples):
            for block_list in level_blocks:
                for layer in block_list:
                    x = step(layer, x)
            skips.append(x)  # stays allocated until the decoder has consumed it
            if not isinstance(down, nn.Identity):
                x, _ = self.conv("down", (lambda m=down: m.conv.weight), (lambda m=down: m.conv.bias), x, None,
                                 k=(3, 4, 4), s=(2, 2), p=(1, 1, 1), cout=down.conv.out_channels)
        x = step(unet.mid_block1, x)
        x = step(unet.mid_attn, x)
        if hasattr(unet, "mid_attn_spatial"):
            x = step(unet.mid_attn_spatial, x)
        x = step(unet.mid_block2, x)
        for level_blocks, up in zip(unet.up_blocks, unet.up_samples):
            for j, block_list in enumerate(level_blocks):
                skip = skips.pop() if j == 0 else None
                for layer in block_list:
                    x = step(layer, x, skip)
                    skip = None
            if not isinstance(up, nn.Identity):
                xo, _ = self.conv("up", (lambda m=up: m.conv.weight), (lambda m=up: m.conv.bias), x, None,
                                  transposed=True, k=(3, 4, 4), s=(2, 2), p=(1, 1, 1),
                                  cout=up.conv.out_channels)
                self.release(x)
                x = xo
        gn, conv = unet.conv_out[0], unet.conv_out[2]
        st = self.gn_colsum(x)
        slot = self.gn_finalize(x, gn.num_groups, st)
        y = self.gn_apply(x, slot, gn, silu_pre=True)
        self.release(x)
        vox = d * h * w
        Lo = 2 * L if self.learn_sigma else L          # ONE head conv: the variance channels ride along
        self.conv("conv_out", lambda: conv.weight, lambda: conv.bias, y, None, cout=Lo,
                  f32_out=self.out2 if self.learn_sigma else self.eps, f32_strides=(vox * Lo, 1, h * w * Lo, w * Lo, Lo))
        self.release(y)
        if self.learn_sigma:
            add_sigma_split(self)
        self.unet_op_count = len(self.ops)
        self.finalize_layout()

    def _input_acts(self, n, d, h, w, halo) -> Tuple[Act, Optional[Act]]:
        """The network input: ONE bf16 tensor [z | cond] (2 L channels; the sampler writes the z half in place)."""
        L = self.L
        return Act(self.persistent((n * (d + 2 * halo) * h * w * 2 * L,), torch.bfloat16, zero=True), n, 2 * L, d, h, w,
                   halo), None

    def _layer(self, layer, x: Act, skip: Optional[Act]) -> Act:
        kind = type(layer).__name__
        if kind == "ResBlock3D":
            return self.unet_resblock(layer, x, skip, self.tbias, self.tb_off[id(layer)], self.total_out,
                                      self.step_ptr)
        if kind == "TemporalAttention":
            return self.attention(layer, x, self.attention_mode)
        if kind == "SpatialAttention":
            return emit_spatial_attention(self, layer, x)[0]
        raise CtsiError(f"unsupported U-Net layer {kind}")

    # -- inputs / schedule --
    def load_latents(self, z_ncdhw: Optional[torch.Tensor], cond_ncdhw: Optional[torch.Tensor]):
        """Take (this rank's depth slab of) the fp32 NCDHW latent / conditioning into the engine layout."""
        lib, sptr = self.lib, self.ctx.sptr
        n, L, d, h, w = self.n, self.L, self.d, self.h, self.w
        lo = 0 if self.shard is None else self.shard.depth_start
        if z_ncdhw is not None:
            z = z_ncdhw.detach()[:, :, lo:lo + d].to(device=self.ctx.device, dtype=torch.float32).contiguous()
            lib.ncdhw_f32_to_ndhwc_f32(_ptr(z), _ptr(self.z), n, L, d, h, w, sptr)
            lib.ncdhw_f32_to_ndhwc_bf16(_ptr(z), self.xin.ip, n, L, d, h, w, 2 * L, 0, sptr)
            if self.guided:     # both halves of z; rows [n, 2n) of the conditioning stay zero (the null conditioning)
                lib.ncdhw_f32_to_ndhwc_bf16(_ptr(z), self._uncond_zin(), n, L, d, h, w, 2 * L, 0, sptr)
            z.record_stream(self.ctx.stream)
            self.xin.dirty = True
        if cond_ncdhw is not None:
            cnd = cond_ncdhw.detach()[:, :, lo:lo + d].to(device=self.ctx.device, dtype=torch.float32).contiguous()
            lib.ncdhw_f32_to_ndhwc_bf16(_ptr(cnd), self.xin.ip, n, L, d, h, w, 2 * L, L, sptr)
            cnd.record_stream(self.ctx.stream)

    def set_guidance(self, scale: float, rescale: float = 0.0):
        """Write {s, phi} into every row of the guided program's scale table (read at *step_ptr by ctsi_cfg_combine /
        ctsi_cfg_stats): a plain device write, the captured graph is untouched."""
        if not self.guided:
            raise CtsiError("internal: set_guidance on a program built without guidance")
        if rescale > 0.0 and not self.rescale:
            raise CtsiError("internal: guidance_rescale > 0 needs a program built with the statistics pass")
        row = torch.tensor([float(scale), float(rescale)], dtype=torch.float32)
        self.cfg_scale.copy_(row.expand(self.cfg_scale.shape[0], 2))

    def set_schedule(self, t_rows: Sequence[float], coef_rows: Optional[torch.Tensor] = None,
                     pred_rows: Optional[torch.Tensor] = None):
        """Upload the timestep of every (step, network row) row -- n per evaluation, 2n in a guided program -- embed all
        of them in one go and rewind the device-side step counter.  Integer-valued rows take the int32 entry
        (ctsi_time_embed_fwd); a schedule with any fractional timestep is embedded from fp32 rows
        (ctsi_time_embed_fwd_tf).  `pred_rows`: the (E, 4) conversion rows of a v-prediction program (StepPlan.pred)."""
        rows = len(t_rows)
        if rows > self.max_rows:
            raise CtsiError(f"schedule needs {rows} rows but the program was built for {self.max_rows}")
        lib, sptr = self.lib, self.ctx.sptr
        self.ensure_fresh()
        vals = list(t_rows)
        fractional = any(float(v) != int(v) for v in vals)
        if fractional:
            self.t_rows_f[:rows].copy_(torch.tensor([float(v) for v in vals], dtype=torch.float32), non_blocking=False)
        else:
            self.t_rows[:rows].copy_(torch.tensor([int(v) for v in vals], dtype=torch.int32), non_blocking=False)
        if coef_rows is not None:
            self.coef[:coef_rows.shape[0]].copy_(coef_rows.to(torch.float32))
        if self.prediction != "epsilon" and getattr(self, "pred_rows", None) is not None:
            if pred_rows is None:
                raise CtsiError("internal: a v-prediction step program needs the schedule's conversion rows")
            if pred_rows.shape[0] > self.pred_rows.shape[0]:
                raise CtsiError(f"schedule needs {pred_rows.shape[0]} conversion rows but the program holds "
                                f"{self.pred_rows.shape[0]}")
            if self.hist is None and bool((pred_rows[:, 2] != 0).any()):
                raise CtsiError("internal: a conversion row reads the history buffer but the sampler kind has none")
            self.pred_rows[:pred_rows.shape[0]].copy_(pred_rows.to(torch.float32))
        self.step_ptr.zero_()
        embed, tp = (lib.time_embed_fwd_tf, self.t_rows_f) if fractional else (lib.time_embed_fwd, self.t_rows)
        embed(_ptr(tp), rows, self.dim, self.time_dim, _ptr(self.w1), _ptr(self.b1), _ptr(self.w2), _ptr(self.b2),
              _ptr(self.w_all), _ptr(self.b_all), self.total_out, _ptr(self.te_scratch), _ptr(self.tbias), sptr)

    def eps_ncdhw(self) -> torch.Tensor:
        """The noise prediction the update reads, fp32 NCDHW: rows [0, n) of `eps` (the guided eps in a guided program).
        In an x0-form program (add_sampler_step(update_form='x0')) the update reads the network's raw v: that is returned."""
        out = torch.empty((self.n, self.L, self.d, self.h, self.w), dtype=torch.float32, device=self.ctx.device)
        self.lib.ndhwc_f32_to_ncdhw_f32(_ptr(self.eps), _ptr(out), self.n, self.L, self.d, self.h, self.w,
                                        self.ctx.sptr)
        return out

    def out_ncdhw(self) -> torch.Tensor:
        """What UNet3D.forward returns, fp32 NCDHW: eps_ncdhw(), or all 2L channels of a learn_sigma model's head."""
        if not self.learn_sigma:
            return self.eps_ncdhw()
        out = torch.empty((self.nb, 2 * self.L, self.d, self.h, self.w), dtype=torch.float32, device=self.ctx.device)
        self.lib.ndhwc_f32_to_ncdhw_f32(_ptr(self.out2), _ptr(out), self.nb, 2 * self.L, self.d, self.h, self.w,
                                        self.ctx.sptr)
        return out

    def z_ncdhw(self) -> torch.Tensor:
        """The sampler state as fp32 NCDHW (the rank's slab only when depth-sharded; gather with
        shard.comm.gather_depth)."""
        out = torch.empty((self.n, self.L, self.d, self.h, self.w), dtype=torch.float32, device=self.ctx.device)
        self.lib.ndhwc_f32_to_ncdhw_f32(_ptr(self.z), _ptr(out), self.n, self.L, self.d, self.h, self.w,
                                        self.ctx.sptr)
        return out

    def guide_scratch(self) -> torch.Tensor:
        """The program's scratch for measurement guidance: a buffer of z's shape that receives the state
        before the replay of a guided evaluation.  Allocated on first use -- an unguided program never holds it -- and kept
        with the program; no captured launch reads or writes it."""
        if self.guide_z is None:
            self.guide_z = torch.empty_like(self.z)
        return self.guide_z

    def _sampler_zin(self):
        """The U-Net input slice the sampler update writes the new z into: (pointer, channels per voxel, bytes per
        element, fp32 entry).  Here the z half of the bf16 [z | cond] tensor."""
        return self.xin.ip, 2 * self.L, 2, False

    def _zin_act(self) -> Act:
        """The tensor of _sampler_zin() as an Act (what the update's audit record names)."""
        return self.xin

    def _add_input_fanout(self):
        """What carries the input the update wrote to every network row that reads it: ctsi_cfg_mirror in a guided program,
        nothing otherwise (window_fuse._WindowFused: the cut into the windows)."""
        if self.guided:
            self._add_guidance_mirror()

    def _uncond_zin(self) -> C.c_void_p:
        """Guided programs: where rows [n, 2n) of the slice of _sampler_zin start."""
        _, c_total, nbytes, _ = self._sampler_zin()
        return C.c_void_p(self._sampler_zin()[0].value + self.n * self.d * self.h * self.w * c_total * nbytes)

    def _add_guidance_combine(self):
        """ctsi_cfg_combine (behind the statistics pass when the program rescales) over the batch-2n eps."""
        lib, sptr = self.lib, self.ctx.sptr
        n, L, d, h, w = self.n, self.L, self.d, self.h, self.w
        numel = float(n * L * d * h * w)
        rows = max(self.max_rows // (2 * n), 1)                    # one {s, phi} row per evaluation
        self.cfg_scale = self.persistent((rows, 2), torch.float32, zero=True)
        self.cfg_scale[:, 0] = 1.0
        ep, cs, sp = _ptr(self.eps), _ptr(self.cfg_scale), _ptr(self.step_ptr)
        self.cfg_stats = None
        if self.rescale:
            bps = lib.cfg_stats_blocks(L * d * h * w)
            self.cfg_partials = self.persistent((n * bps * 4,), torch.float64, zero=True)
            self.cfg_stats = self.persistent((n, 4), torch.float64, zero=True)
            pp, stp = _ptr(self.cfg_partials), _ptr(self.cfg_stats)
            self._emit(lambda: lib.cfg_stats(ep, cs, sp, pp, n, L, d, h, w, sptr), "cfg.stats", nbytes=8.0 * numel,
                       audit=dict(kind="cfg_stats", eps=self.eps, scale=self.cfg_scale, step_ptr=self.step_ptr,
                                  partials=self.cfg_partials, n=n, bps=bps))
            self._emit(lambda: lib.cfg_stats_finalize(pp, stp, n, L, d, h, w, sptr), "cfg.stats_finalize",
                       audit=dict(kind="cfg_stats_finalize", partials=self.cfg_partials, stats=self.cfg_stats, n=n, bps=bps,
                                  count=L * d * h * w))
        stp = _ptr(self.cfg_stats)
        self._emit(lambda: lib.cfg_combine(ep, cs, sp, stp, n, L, d, h, w, sptr), "cfg.combine", nbytes=12.0 * numel,
                   audit=dict(kind="cfg_combine", eps=self.eps, scale=self.cfg_scale, step_ptr=self.step_ptr,
                              stats=self.cfg_stats, n=n))

    def _add_guidance_mirror(self):
        """ctsi_cfg_mirror: the z the update wrote into rows [0, n) of the network input, copied to rows [n, 2n)."""
        lib, sptr = self.lib, self.ctx.sptr
        src, c_total, nbytes, _ = self._sampler_zin()
        dst = self._uncond_zin()
        rows, L = self.n * self.d * self.h * self.w, self.L
        self._emit(lambda: lib.cfg_mirror(src, dst, rows, L * nbytes, c_total * nbytes, sptr), "cfg.mirror",
                   nbytes=2.0 * rows * L * nbytes, audit=dict(kind="cfg_mirror", zin=self.xin, n=self.n, L=L))

    def add_sampler_step(self, kind: str, with_noise: bool, update_form: str = "eps", learned_variance: bool = False):
        """Append the update of sampler `kind` (a SAMPLER_STEPS key) and the step-counter increment (done once, before
        capture).  'heun': one update per U-Net evaluation (predictor, corrector or final row); `with_noise` = churn on.
        A v-prediction program converts the network output first (prediction.add_pred_to_eps), ahead of the guidance.
        `update_form` 'x0' ('ddim', 'ddpm', 'dpmpp' of a v-prediction program): no conversion launch --
        the guidance and ctsi_x0_step (x0_form.add_x0_step) read the raw v, and eps_ncdhw() returns it.
        `learned_variance` (kind 'ddpm_lv' of a learn_sigma program): the update reads `vraw`, which the
        split launch then fills; otherwise the kind's variance operand is NULL (fixed-small)."""
        lib, sptr = self.lib, self.ctx.sptr
        n, L, d, h, w = self.n, self.L, self.d, self.h, self.w
        entry = sampler_step_row(kind)
        x0_form = check_update_form(update_form, self.prediction) == "x0"
        if x0_form and kind == "heun":
            raise CtsiError("internal: the EDM sampler has no x0-form update")
        if x0_form and entry.vraw:
            raise CtsiError("internal: the respaced / learned-variance ancestral step has no x0-form update")
        if entry.vraw and learned_variance and not self.learn_sigma:
            raise CtsiError("internal: a learned-variance step on a program without variance channels")
        if entry.vraw and learned_variance:
            self.vraw = self.persistent((n, d, h, w, L), torch.float32, zero=True)
        self.hist = None
        if self.prediction != "epsilon" and not x0_form:
            if entry.hist:      # (the conversion of a Heun corrector row reads the history)
                self.hist = self.persistent((n, d, h, w, L), torch.float32, zero=True)
            add_pred_to_eps(self)
        if self.guided:
            self._add_guidance_combine()
        if with_noise and self.noise is None:
            self.noise = self.persistent((n, L, d, h, w), torch.float32, zero=True)
        xp, c_total, zin_bytes, f32 = self._sampler_zin()
        step = sampler_step_launcher(lib, kind, f32)
        zp, ep, cp, sp = _ptr(self.z), _ptr(self.eps), _ptr(self.coef), _ptr(self.step_ptr)
        npz = _ptr(self.noise if with_noise else None)
        # what the reference's NaN/Inf checkpoints would report: rows 0..max_rows-1 = per step {noise_pred, z_0_pred, z}
        # x {NaN, Inf}; the two extra rows = initial noise and conditioning (sampler.py:268-275).  Read once per sample().
        self.nonfinite = self.persistent((self.max_rows + 2, 6), torch.int32, zero=True)
        nfp = _ptr(self.nonfinite)
        # the kind's history (fp32 NDHWC, zeroed: the update only ever stores finite values in it)
        if self.hist is None and entry.hist:
            self.hist = self.persistent((n, d, h, w, L), torch.float32, zero=True)
        hp = _ptr(self.hist)
        vp = _ptr(self.vraw)
        xin = self.xin

        def run_step():
            step(zp, ep, hp, npz, xp, c_total, cp, sp, n, L, d, h, w, nfp, sptr, vp)
            if not f32:
                xin.dirty = True

        def run_adv():
            lib.step_advance(sp, sptr)

        step_bytes = (4 + 4 + 4 + zin_bytes + (4 if with_noise else 0) + (8 if entry.hist else 0)
                      + (4 if self.vraw is not None else 0)) * float(
            n * L * d * h * w)
        if x0_form:
            add_x0_step(self, kind, with_noise)
        else:
            self._emit(run_step, "sampler.step", nbytes=step_bytes,
                       audit=dict(kind="sampler_step", sampler=kind, z=self.z, eps=self.eps, hist=self.hist,
                                  noise=self.noise if with_noise else None, zin=self._zin_act(), coef=self.coef,
                                  step_ptr=self.step_ptr, nonfinite=self.nonfinite if entry.nonfinite else None, n=n, L=L,
                                  **(dict(vraw=self.vraw) if entry.vraw else {})))
        self._add_input_fanout()
        self._emit(run_adv, "sampler.advance", audit=dict(kind="sampler_advance", step_ptr=self.step_ptr))
        self.sampler_kind = (kind, with_noise)
        self.update_form = update_form


# ==========================================================================================================
# VAE
# ==========================================================================================================
def _pad8(c: int) -> int:
    return (c + 7) // 8 * 8


class VAEEncodeProgram(Program):
    """VideoEncoder.forward + scaling (models/vae.py:139-147, 235-247) at a fixed input shape."""

    def __init__(self, ctx: Ctx, vae, n, d, h, w):
        super().__init__(ctx)
        enc = vae.encoder
        self.n, self.d, self.h, self.w = n, d, h, w
        cin = vae.in_channels
        self.cin, self.cin_pad = cin, _pad8(cin)
        self.track_module(enc)
        self.xin, cin_w = self._input_act(n, cin, d, h, w, 0)
        self.zero_gn_op()
        x = self._conv_gn_act(enc.conv_in, self.xin, cin_w=cin_w, free=False)
        for stage in (enc.down1, enc.down2):
            for m in stage:
                x = self._block(m, x)
        for m in enc.mid:
            x = self._block(m, x)
        y, _ = self.conv("enc.conv_out", lambda: enc.conv_out.weight, lambda: enc.conv_out.bias, x, None,
                         cout=enc.conv_out.out_channels)
        self.release(x)
        L = vae.latent_dim
        self.L = L
        hl, wl = y.h, y.w
        self.hl, self.wl = hl, wl
        self.out = self.persistent((n, L, d, hl, wl), torch.float32)
        vox = d * hl * wl
        sf = lambda: float(vae.scaling_factor)
        self.conv("enc.quant", lambda: enc.quant_conv.weight * sf(), lambda: enc.quant_conv.bias * sf(), y, None,
                  k=(1, 1, 1), p=(0, 0, 0), cout=L, f32_out=self.out,
                  f32_strides=(L * vox, vox, hl * wl, wl, 1))
        self.release(y)
        self.finalize_layout()

    def _input_act(self, n, c, d, h, w, halo) -> Tuple[Act, Optional[int]]:
        """The network input and the `cin_w` of its first conv: bf16 NDHWC padded to 8 channels (the weights carry c)."""
        return Act(self.persistent((n * (d + 2 * halo) * h * w * _pad8(c),), torch.bfloat16, zero=True), n, _pad8(c), d, h,
                   w, halo), c

    def _upload(self, src: torch.Tensor, a: Act, c: int):
        """fp32 NCDHW `src` (c channels) -> the own slices of the input tensor `a`."""
        self.lib.ncdhw_f32_to_ndhwc_bf16(_ptr(src), a.ip, a.n, c, a.d, a.h, a.w, a.c, 0, self.ctx.sptr)

    def _conv_gn_act(self, m, x: Act, *, cin_w=None, free=True, k=(3, 3, 3), s=(1, 1), transposed=False) -> Act:
        c, st = self.conv("conv+gn", lambda: m.conv.weight, lambda: m.conv.bias, x, None, k=k, s=s,
                          transposed=transposed, cout=m.conv.out_channels, cin_w=cin_w, want_stats=True)
        if free:
            self.release(x)
        slot = self.gn_finalize(c, m.norm.num_groups, st)
        return self.gn_apply(c, slot, m.norm, silu_pre=True, out=c)

    def _resblock(self, m, x: Act) -> Act:
        c1, st = self.conv("rb.conv1", lambda: m.conv1.conv.weight, lambda: m.conv1.conv.bias, x, None,
                           cout=x.c, want_stats=True)
        slot = self.gn_finalize(c1, m.conv1.norm.num_groups, st)
        c2, st = self.conv("rb.conv2", lambda: m.conv2[0].weight, lambda: m.conv2[0].bias, c1, None, cout=x.c,
                           want_stats=True, norm_in=(slot, m.conv1.norm, True, None))
        self.release(c1)
        slot = self.gn_finalize(c2, m.conv2[1].num_groups, st)
        out = self.gn_apply(c2, slot, m.conv2[1], silu_pre=False, residual=x, silu_post=True, out=c2)
        self.release(x)
        return out

    def _block(self, m, x: Act) -> Act:
        kind = type(m).__name__
        if kind == "ResBlock3D":
            return self._resblock(m, x)
        if kind == "DownsampleBlock":
            return self._conv_gn_act(m, x, k=(3, 4, 4), s=(2, 2))
        if kind == "UpsampleBlock":
            return self._conv_gn_act(m, x, k=(3, 4, 4), s=(2, 2), transposed=True)
        raise CtsiError(f"unsupported VAE block {kind}")

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        self.ensure_fresh()
        xx = x.detach().to(device=self.ctx.device, dtype=torch.float32).contiguous()
        self._upload(xx, self.xin, self.cin)
        xx.record_stream(self.ctx.stream)
        self.launch()
        out = self.out.clone()
        self.check_errors()
        return out


class VAEDecodeProgram(VAEEncodeProgram):
    """VideoDecoder.forward + unscaling (models/vae.py:190-204, 249-260) at a fixed latent shape.
    With `shard` the program decodes this rank's depth slab (d = local depth); halos are exchanged before
    every depth-3 conv and the GroupNorm statistics are all-reduced, as in the U-Net."""

    def __init__(self, ctx: Ctx, vae, n, d, h, w, shard=None):
        Program.__init__(self, ctx)
        self.shard = shard
        dec = vae.decoder
        self.n, self.d, self.h, self.w = n, d, h, w
        L = vae.latent_dim
        self.L, self.L_pad = L, _pad8(L)
        self.track_module(dec)
        halo = 0 if shard is None else 1
        self.zin, cin_w = self._input_act(n, L, d, h, w, halo)
        self.zero_gn_op()
        inv = lambda: 1.0 / float(vae.scaling_factor)
        x, _ = self.conv("dec.post_quant", lambda: dec.post_quant_conv.weight * inv(),
                         lambda: dec.post_quant_conv.bias, self.zin, None, k=(1, 1, 1), p=(0, 0, 0),
                         cout=dec.post_quant_conv.out_channels, cin_w=cin_w)
        x = self._conv_gn_act(dec.conv_in, x)
        for m in dec.mid:
            x = self._block(m, x)
        x = self._block(dec.up2_upsample, x)
        for m in dec.up2_res:
            x = self._block(m, x)
        x = self._block(dec.up3_upsample, x)
        for m in dec.up3_res:
            x = self._block(m, x)
        co = dec.conv_out.out_channels
        self.co = co
        self.ho, self.wo = x.h, x.w
        self.out = self.persistent((n, co, d, x.h, x.w), torch.float32)
        vox = d * x.h * x.w
        self.conv("dec.conv_out", lambda: dec.conv_out.weight, lambda: dec.conv_out.bias, x, None, cout=co,
                  f32_out=self.out, f32_strides=(co * vox, vox, x.h * x.w, x.w, 1), act=1)
        self.release(x)
        self.finalize_layout()

    def load(self, z: torch.Tensor):
        self.ensure_fresh()
        lo = 0 if self.shard is None else self.shard.depth_start
        zz = z.detach()[:, :, lo:lo + self.d].to(device=self.ctx.device, dtype=torch.float32).contiguous()
        self._upload(zz, self.zin, self.L)
        zz.record_stream(self.ctx.stream)

    def __call__(self, z: torch.Tensor) -> torch.Tensor:
        self.load(z)
        if self.shard is None:
            self.launch()
            out = self.out.clone()
            self.check_errors()
            return out
        self.run()
        out = self.shard.comm.gather_depth(self.shard.rank, self.out, counts=self.shard.depth_counts)
        self.check_errors()
        return out


# ==========================================================================================================
# program caches hung off the modules
# ==========================================================================================================
PROGRAM_CACHE_SIZE = int(os.environ.get("CTSI_PROGRAM_CACHE", "4"))   # programs kept per module (they own their
                                                                        # activation buffers: ~5 GB for the 512^2 U-Net)


def invalidate_engine_cache(module: nn.Module):
    """Drop every cached program (packed weights, captured graphs, activation buffers) of `module` and its
    sub-modules; the next call rebuilds from the current parameters."""
    for m in module.modules():
        m.__dict__.pop("_ctsi_programs", None)


def check_resblock_options_unsharded(unet, sharded: bool):
    """CtsiError when a U-Net built with use_scale_shift_norm=True meets depth sharding (out of scope, as
    softmax attention is -- the scale-shift pass has no halo-extended form)."""
    if sharded and getattr(unet, "use_scale_shift_norm", False):
        raise CtsiError("use_scale_shift_norm=True does not support depth sharding (unet.depth_shard_comm): the scale-shift "
                        "pass has no halo-extended form; drop the communicator or build the model with "
                        "use_scale_shift_norm=False")


def cached_program(module: nn.Module, key, build: Callable[[], Program]) -> Program:
    cache = module.__dict__.setdefault("_ctsi_programs", {})
    prog = cache.get(key)
    if prog is not None and prog.needs_rebuild():
        cache.pop(key)
        prog = None
    if prog is not None:
        cache[key] = cache.pop(key)   # LRU: most recently used last
    if prog is None:
        if len(cache) >= max(1, PROGRAM_CACHE_SIZE):
            cache.pop(next(iter(cache)))
        prog = build()
        cache[key] = prog
    return prog


def check_device_errors(ctx: Ctx):
    """Raise CtsiError if a kernel recorded a device-side error since the last check (ctsi_device_error_status: a split-K
    conv block whose wait for its partner expired raises a sticky count instead of passing a wrong result on
    silently).  One 8-byte synchronous read: called where the host reads results anyway (once per sample())."""
    cnt, det = C.c_uint(0), C.c_uint(0)
    ctx.stream.synchronize()       # the read below is a blocking copy on the null stream, which does not order with ours
    ctx.lib.device_error_status(C.byref(cnt), C.byref(det), 1)
    if cnt.value:
        # the failed hand-off left its ticket / flag words set (on purpose: a late partner must not meet reset words): start
        # every split-K layer of every live program on this device from a clean workspace again
        with torch.cuda.stream(ctx.stream):
            for prog in list(_LIVE_PROGRAMS):
                if prog.ctx is ctx:
                    for ws in prog._sk_workspaces:
                        ws.zero_()
        ctx.stream.synchronize()
        raise CtsiError(f"{cnt.value} device-side error(s) recorded by the HIP engine (last: split-K hand-off of conv tile "
                        f"{det.value} timed out); outputs computed since the last check are invalid")


def trilinear_depth(ctx: Ctx, z: torch.Tensor, d_out: int) -> torch.Tensor:
    """F.interpolate(z, size=(d_out, h, w), mode='trilinear', align_corners=False) for fp32 NCDHW z."""
    n, c, d, h, w = z.shape
    zz = z.detach().to(device=ctx.device, dtype=torch.float32).contiguous()
    out = torch.empty((n, c, d_out, h, w), dtype=torch.float32, device=ctx.device)
    ctx.lib.trilinear_depth_fwd(_ptr(zz), None, n, c, d, d_out, h, w, c, 0, _ptr(out), ctx.sptr)
    zz.record_stream(ctx.stream)
    return out


def nan_to_num_(ctx: Ctx, t: torch.Tensor) -> torch.Tensor:
    ctx.lib.nan_to_num_f32(_ptr(t), t.numel(), ctx.sptr)
    return t
