"""Optimizer step of the training path on the HIP engine.

The reference builds `torch.optim.Adam` / `torch.optim.AdamW` over per-module parameter groups with their own learning
rates (training/train.py:172-212) and steps it once per accumulation window (training/trainer.py:237-247, through a
GradScaler under AMP).  `FusedAdamW` / `FusedAdam` are drop-ins for those two classes -- same constructor arguments, same
`param_groups` / `state` / `state_dict()` layout (`step`, `exp_avg`, `exp_avg_sq` per parameter), so LR schedulers,
GradScaler, `clip_grad_norm_` and checkpoints of the torch optimizers keep working -- whose `step()` is ONE
`ctsi_adamw_multi` launch over all tensors of all groups, followed by the engine's fast re-pack of the bf16 kernel images of
the programs that use these parameters (`engine.Program.fast_repack`).  There is no CPU path: parameters must live on a
ROCm device.

Two more passes over the parameter set belong to a diffusion trainer's step, and both ride in the same launch when asked for
(DESIGN.md section 13): `max_grad_norm=` clips by the global gradient norm (two small norm launches, then the update reads the
coefficient from device memory: no host synchronisation, no rewrite of the gradients) and `ema=` keeps an `EMAWeights` average
of the new parameters.  `clip_grad_norm_` below is the stand-alone form for users of a torch optimizer."""
from __future__ import annotations

import ctypes as C
import math
import struct
from typing import Iterable, Optional, Sequence

import torch

from .ema import EMAWeights, bump_versions, chunk_table
from .lib import CtsiError, get_lib


class FusedAdamW(torch.optim.Optimizer):
    decoupled = True     # AdamW: p *= 1 - lr * wd; FusedAdam below: grad += wd * p (torch.optim.Adam's L2 form)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize: bool = False, engine_modules: Optional[Sequence[torch.nn.Module]] = None,
                 max_grad_norm: Optional[float] = None, ema: Optional[EMAWeights] = None):
        """`engine_modules` (additive kwarg): modules (e.g. `[model.unet]`) whose cached engine programs are re-packed right
        behind the update; without it the programs notice the new parameter versions on their next use and re-pack then
        (the generic, slower path).

        `max_grad_norm`: `step()` first takes the global L2 norm of exactly the gradients it is about to consume
        (`ctsi_grad_norm_multi` + `ctsi_grad_norm_finalize`, fp64 accumulation) and the update launch multiplies them by
        torch's `clip_coef = min(1, max_norm / (norm + 1e-6))` as it reads them.  The one visible difference from
        `clip_grad_norm_(...)` followed by `step()`: the `.grad` tensors KEEP THEIR UNCLIPPED VALUES.  `last_grad_norm` is
        the norm as a 0-d device tensor (reading it is the caller's synchronisation).  Under a GradScaler the gradients are
        already unscaled when `step()` runs, so the norm is that of the true gradients.  A non-finite norm is not an error
        (torch's `error_if_nonfinite=False`) and no step is skipped here: that is GradScaler's job.

        `ema`: an `EMAWeights` over (a subset or superset of) the same parameters; the update launch averages the shadows of
        the parameters it steps from their new values, and the shadows of parameters without a gradient this step advance in
        one `ctsi_ema_multi` launch behind it, so every shadow moves once per `step()`.

        With neither, `step()` is the `ctsi_adamw_multi` launch it always was."""
        if amsgrad:
            raise CtsiError("FusedAdamW: amsgrad is not supported by the HIP engine")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not 0.0 <= weight_decay:
            raise ValueError(f"invalid optimizer hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize)
        super().__init__(params, defaults)
        self.engine_modules = list(engine_modules) if engine_modules is not None else []
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"invalid max_grad_norm={max_grad_norm}")
        if ema is not None and not isinstance(ema, EMAWeights):
            raise TypeError("ema must be an EMAWeights instance")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema = ema
        if ema is not None:
            ema._attach(self)
        self.last_grad_norm = None
        self._lib = get_lib()
        self._tables = None

    # ---- state (torch layout: state[p] = {step, exp_avg, exp_avg_sq}) ---------------------------------------------------
    def _init_state(self, p: torch.Tensor):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def state_dict(self):
        """torch's layout.  The step counters the parameters of a group share in here are written out as one tensor per
        parameter: torch's optimizers increment `step` per parameter, so aliased counters (aliasing survives the deepcopy
        in load_state_dict) would be bumped once per parameter."""
        sd = super().state_dict()
        sd["state"] = {k: ({**v, "step": v["step"].clone()} if isinstance(v, dict) and torch.is_tensor(v.get("step")) else v)
                       for k, v in sd["state"].items()}
        return sd

    def _build_tables(self, entries, dev):
        """entries: [(param, hyper-row index)] of the parameters that have a gradient this step."""
        chunk = self._lib.adamw_chunk_elems()
        chunks = chunk_table([p.numel() for p, _ in entries], chunk)
        ck = chunks.to(dev)
        n = len(entries)
        wide = self.ema is not None or self.max_grad_norm is not None
        # CtsiOptTensor rows: p, g, m, v, numel, (row | pad); the fused entry point's CtsiOptEmaTensor rows: p, g, m, v, ema,
        # numel, (row | ema group 0), pad
        cols, c_numel = (8, 5) if wide else (6, 4)
        host = torch.zeros((n, cols), dtype=torch.int64)
        for i, (p, row) in enumerate(entries):
            st = self.state[p]
            for name in ("exp_avg", "exp_avg_sq"):
                if st[name].device != p.device or st[name].dtype != torch.float32 or not st[name].is_contiguous():
                    st[name] = st[name].to(device=p.device, dtype=torch.float32).contiguous()   # (a loaded state dict)
            host[i, 0], host[i, 2], host[i, 3] = p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            host[i, c_numel], host[i, c_numel + 1] = p.numel(), row   # (little endian: the int `group` is the low word)
            if self.ema is not None and self.ema.shadow_of(p) is not None:
                host[i, 4] = self.ema.shadow_of(p).data_ptr()
        self._tables = dict(key=tuple(id(p) for p, _ in entries), rows=tuple(r for _, r in entries), chunks=ck,
                            nchunks=len(chunks), dev=dev, host=host, gptr=None, state_ptrs=self._state_ptrs(entries),
                            tensors=torch.empty((n, cols), dtype=torch.int64, device=dev),
                            groups=torch.empty(max(n, 1) * 64, dtype=torch.uint8, device=dev))
        if self.ema is not None:
            self._tables["ema_w"] = torch.empty(1, dtype=torch.float32, device=dev)
        if self.max_grad_norm is not None:                          # CtsiNormTensor rows: g, numel, (scale 1.0f | pad)
            nhost = torch.zeros((n, 3), dtype=torch.int64)
            nhost[:, 1] = host[:, c_numel]
            nhost[:, 2] = struct.unpack("<q", struct.pack("<fi", 1.0, 0))[0]
            self._tables.update(nhost=nhost, ntensors=torch.empty((n, 3), dtype=torch.int64, device=dev),
                                partials=torch.empty(max(len(chunks), 1), dtype=torch.float64, device=dev))

    def _state_ptrs(self, entries):
        """Addresses the cached tables hold (beside the gradients'): a table is rebuilt when one of them has moved."""
        shadow = self.ema.shadow_of if self.ema is not None else (lambda p: None)
        return tuple((p.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(),
                      0 if (s := shadow(p)) is None else s.data_ptr()) for p, _ in entries)

    def _hyper_rows(self):
        """Step bookkeeping + one CtsiOptGroup row per (parameter group, step count) present.  torch counts steps per
        parameter (a parameter without a gradient skips the step), so a group may hold several counts; the counters of
        parameters that move together are ONE shared CPU tensor (350 tensor increments per step would cost more host time
        than the kernel takes); a parameter that sits a step out gets its own copy first.  Returns (entries, rows)."""
        entries, rows, row_of = [], [], {}
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            live = [p for p in params if p.grad is not None]
            if not live:
                continue
            state = self.state
            first = state.get(live[0])
            shared = first["step"] if first else None
            uniform = (shared is not None and len(live) == len(params)
                       and all((st := state.get(p)) is not None and len(st) and st["step"] is shared for p in live))
            if uniform:                                  # the steady state: one counter, one row for the whole group
                shared += 1
                steps = [(live, float(shared))]
            else:
                live_counters = {id(state[q]["step"]) for q in live if state.get(q)}
                for p in params:                         # (parameters sitting this step out leave the shared counters ...)
                    st = state.get(p)
                    if p.grad is None and st and id(st["step"]) in live_counters:
                        st["step"] = st["step"].clone()
                bumped, by_t = {}, {}
                for p in live:                           # (... then the counters move on)
                    if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                        raise CtsiError("FusedAdamW runs on the HIP engine: parameters must be contiguous fp32 tensors on a "
                                        "ROCm device")
                    st = self._init_state(p)
                    key = id(st["step"])
                    if key not in bumped:
                        t_prev = float(st["step"])
                        share = next((c for c, tp in bumped.values() if tp == t_prev), None)
                        if share is not None:            # same count as a counter already seen: share it
                            st["step"] = share
                        else:
                            st["step"] += 1
                            bumped[key] = (st["step"], t_prev)
                    by_t.setdefault(float(st["step"]), []).append(p)
                steps = [(ps, t) for t, ps in by_t.items()]
            b1, b2 = group["betas"]
            lr, wd = float(group["lr"]), float(group["weight_decay"])
            for ps, t in steps:
                bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
                row_of[(gi, t)] = len(rows)
                rows.append(struct.pack("<11f5i", lr, b1, b2, float(group["eps"]), wd, lr / bc1, math.sqrt(bc2),
                                        1.0 - lr * wd, 1.0 - b1, 1.0 - b2, 1.0, int(self.decoupled),
                                        int(bool(group.get("maximize", False))), 0, 0, 0))
                entries.extend((p, row_of[(gi, t)]) for p in ps)
        return entries, rows

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ema = self.ema
        ema_w = ema._fused_weight() if ema is not None else None     # (raises inside ema.applied())
        entries, rows = self._hyper_rows()
        if not entries:
            if ema is not None:
                ema._fused_done((), ema_w)           # no gradient anywhere: the shadows still advance once per step()
            return loss
        if ema is not None:
            ema._device()                            # (shadows follow a model that was moved after construction)
        tb = self._tables
        key = tuple(id(p) for p, _ in entries)
        if (tb is None or tb["key"] != key or tb["rows"] != tuple(r for _, r in entries)
                or tb["state_ptrs"] != self._state_ptrs(entries)):
            for p, _ in entries:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise CtsiError("FusedAdamW runs on the HIP engine: parameters must be contiguous fp32 tensors on a ROCm "
                                    "device")
            self._build_tables(entries, entries[0][0].device)
            tb = self._tables
        dev = tb["dev"]
        # gradients: new tensors after every backward, usually at the addresses of the previous step (caching allocator)
        grads = []
        for p, _ in entries:
            g = p.grad
            if g.dtype is not torch.float32 or g.is_sparse or g.device != p.device or not g.is_contiguous():
                if g.is_sparse:
                    raise CtsiError("FusedAdamW does not support sparse gradients")
                g = g.to(device=p.device, dtype=torch.float32).contiguous()
            grads.append(g)
        gptr = tuple(g.data_ptr() for g in grads)
        if gptr != tb["gptr"]:
            tb["host"][:, 1] = torch.tensor(gptr, dtype=torch.int64)
            tb["tensors"].copy_(tb["host"])
            if self.max_grad_norm is not None:
                tb["nhost"][:, 0] = tb["host"][:, 1]
                tb["ntensors"].copy_(tb["nhost"])
            tb["gptr"] = gptr
        gbytes = b"".join(rows)
        tb["groups"][:len(gbytes)].copy_(torch.frombuffer(bytearray(gbytes), dtype=torch.uint8))
        stream = torch.cuda.current_stream(dev)
        sptr = C.c_void_p(stream.cuda_stream)
        with torch.cuda.device(dev):
            if ema is None and self.max_grad_norm is None:
                self._lib.adamw_multi(C.c_void_p(tb["tensors"].data_ptr()), C.c_void_p(tb["groups"].data_ptr()),
                                      C.c_void_p(tb["chunks"].data_ptr()), tb["nchunks"], sptr)
            else:
                coef_ptr = wptr = None
                if self.max_grad_norm is not None:
                    out = torch.empty(2, dtype=torch.float32, device=dev)      # {total_norm, clip_coef}: a fresh pair per
                    self._lib.grad_norm_multi(C.c_void_p(tb["ntensors"].data_ptr()),   # step, so last_grad_norm stays valid
                                              C.c_void_p(tb["chunks"].data_ptr()), tb["nchunks"],
                                              C.c_void_p(tb["partials"].data_ptr()), sptr)
                    self._lib.grad_norm_finalize(C.c_void_p(tb["partials"].data_ptr()), tb["nchunks"], self.max_grad_norm,
                                                 C.c_void_p(out.data_ptr()), sptr)
                    self.last_grad_norm = out[0]
                    coef_ptr = C.c_void_p(out.data_ptr() + 4)
                if ema is not None:
                    tb["ema_w"].copy_(torch.frombuffer(bytearray(struct.pack("<f", ema_w)), dtype=torch.float32))
                    wptr = C.c_void_p(tb["ema_w"].data_ptr())
                self._lib.adamw_ema_multi(C.c_void_p(tb["tensors"].data_ptr()), C.c_void_p(tb["groups"].data_ptr()),
                                          C.c_void_p(tb["chunks"].data_ptr()), tb["nchunks"], coef_ptr, wptr, sptr)
        for g in grads:
            g.record_stream(stream)
        # the update went through raw pointers: tell torch (and, through it, every engine program's fingerprint)
        bump_versions([p for p, _ in entries])
        if ema is not None:
            ema._fused_done([p for p, _ in entries], ema_w)
        self._repack_engine_programs()
        return loss

    def _repack_engine_programs(self):
        """Fast re-pack of the programs (training programs: they own their weight images) of `engine_modules`."""
        for mod in self.engine_modules:
            subs = mod.__dict__.get("_ctsi_submodules")
            if subs is None:
                subs = mod.__dict__["_ctsi_submodules"] = list(mod.modules())
            for m in subs:
                progs = m.__dict__.get("_ctsi_programs")
                if not progs:
                    continue
                for prog in list(progs.values()):
                    if not prog.weight_cache and not prog.needs_rebuild():
                        prog.ctx.enter()
                        try:
                            prog.fast_repack()
                        finally:
                            prog.ctx.leave()


class FusedAdam(FusedAdamW):
    """torch.optim.Adam (weight decay as an L2 term on the gradient), the reference's default optimizer
    (training/train.py:205-206)."""
    decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)


_CLIP_TABLES: dict = {}


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False,
                    foreach: Optional[bool] = None) -> torch.Tensor:
    """Drop-in for `torch.nn.utils.clip_grad_norm_` with `norm_type=2.0` on the HIP engine, for users of a torch optimizer:
    the two norm launches (`ctsi_grad_norm_multi`, `ctsi_grad_norm_finalize`: fp64 accumulation, no atomics) and ONE in-place
    scale of all gradients by `min(1, max_norm / (norm + 1e-6))` read from device memory (`ctsi_grad_scale_multi`; it writes
    nothing when the coefficient is 1).  Returns the total norm as a 0-d device tensor without synchronising
    (`error_if_nonfinite=True` reads it, as torch's does).  `foreach` is accepted and ignored."""
    if float(norm_type) != 2.0:
        raise CtsiError(f"clip_grad_norm_: only norm_type=2.0 runs on the HIP engine (got {norm_type})")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    for g in grads:
        if not g.is_cuda or g.device != dev or g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous():
            raise CtsiError("clip_grad_norm_ runs on the HIP engine: gradients must be contiguous fp32 tensors on one ROCm "
                            "device")
    lib = get_lib()
    key = tuple((g.data_ptr(), g.numel()) for g in grads)
    tb = _CLIP_TABLES.get(dev)
    if tb is None or tb["key"] != key:
        host = torch.zeros((len(grads), 3), dtype=torch.int64)      # CtsiNormTensor rows: g, numel, (scale 1.0f | pad)
        host[:, 0] = torch.tensor([k[0] for k in key], dtype=torch.int64)
        host[:, 1] = torch.tensor([k[1] for k in key], dtype=torch.int64)
        host[:, 2] = struct.unpack("<q", struct.pack("<fi", 1.0, 0))[0]
        ck = chunk_table([k[1] for k in key], lib.adamw_chunk_elems())
        tb = _CLIP_TABLES[dev] = dict(key=key, tensors=host.to(dev), chunks=ck.to(dev), nchunks=len(ck),
                                      partials=torch.empty(max(len(ck), 1), dtype=torch.float64, device=dev))
    out = torch.empty(2, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)
    sptr = C.c_void_p(stream.cuda_stream)
    tensors, chunks = C.c_void_p(tb["tensors"].data_ptr()), C.c_void_p(tb["chunks"].data_ptr())
    with torch.cuda.device(dev):
        lib.grad_norm_multi(tensors, chunks, tb["nchunks"], C.c_void_p(tb["partials"].data_ptr()), sptr)
        lib.grad_norm_finalize(C.c_void_p(tb["partials"].data_ptr()), tb["nchunks"], float(max_norm),
                               C.c_void_p(out.data_ptr()), sptr)
        lib.grad_scale_multi(tensors, chunks, tb["nchunks"], C.c_void_p(out.data_ptr() + 4), sptr)
    for g in grads:
        g.record_stream(stream)
    bump_versions(grads)
    total = out[0]
    if error_if_nonfinite and not bool(torch.isfinite(total)):
        raise RuntimeError("The total norm for gradients from `parameters` is non-finite, so it cannot be clipped")
    return total
