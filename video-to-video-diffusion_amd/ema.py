"""Exponential moving average of the weights.

Diffusion trainers sample from an average of the U-Net weights, not from the raw ones.  `EMAWeights` keeps one fp32 shadow per
trainable parameter, updates all of them in ONE launch (`ctsi_ema_multi`; or inside the optimizer's own launch when handed to
`FusedAdamW(ema=...)`), and puts them into the model for sampling by exchanging VALUES with the parameters
(`ctsi_swap_multi`): no twin model, no address changes, so pointer tables, captured graphs and the engine's content-hashed
weight cache all stay valid.  Parameters on the CPU take a plain torch path (`lerp_`, tensor swap); parameters on a device
always go through the kernels.

    ema = EMAWeights(model.unet, prefix='unet.')
    opt = FusedAdamW(model.unet.parameters(), lr=1e-4, ema=ema, max_grad_norm=1.0, engine_modules=[model.unet])
    ...                                            # loss.backward(); opt.step() averages in the same launch
    with ema.applied():
        video = model.generate(...)                # samples with the averaged weights
    model.save_checkpoint(path, optimizer=opt, ema_state_dict=ema.state_dict())
    load_model_from_checkpoint(model, path, use_ema=True)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import struct
from typing import Dict, Iterable, List, Tuple, Union

import torch

from .lib import CtsiError, get_lib


def chunk_table(numels, chunk: int) -> torch.Tensor:
    """{tensor, first element / 4} rows, one per `chunk` elements of every tensor (the layout of ctsi_adamw_multi's chunks)."""
    rows = []
    for i, n in enumerate(numels):
        rows.extend((i, q * (chunk // 4)) for q in range((n + chunk - 1) // chunk))
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 2)


def bump_versions(params) -> None:
    """A raw-pointer write is invisible to torch: move the version counters, which every engine program fingerprints."""
    bump = getattr(torch.autograd.graph, "increment_version", None)
    if bump is not None:
        bump(list(params))
    else:  # pragma: no cover  (older torch)
        with torch.no_grad():
            for p in params:
                p.add_(0)


class EMAWeights:
    def __init__(self, module_or_named_parameters: Union[torch.nn.Module, Iterable[Tuple[str, torch.Tensor]]],
                 decay: float = 0.9999, warmup: bool = True, prefix: str = ''):
        """fp32 shadows of every parameter with `requires_grad`, initialised to the current values and named `prefix` + the
        parameter's name in the module given: `EMAWeights(model)` and `EMAWeights(model.unet, prefix='unet.')` both produce
        keys of the whole model's `state_dict()`.  With `warmup`, update number n (from 0) uses
        `min(decay, (1 + n) / (10 + n))`, which equals `decay` from n >= (10 decay - 1) / (1 - decay) on."""
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"EMAWeights: decay must be in [0, 1), got {decay}")
        named = (module_or_named_parameters.named_parameters() if isinstance(module_or_named_parameters, torch.nn.Module)
                 else module_or_named_parameters)
        self.decay, self.warmup, self.prefix = float(decay), bool(warmup), prefix
        self.names: List[str] = []
        self.params: List[torch.Tensor] = []
        for name, p in named:
            if p.requires_grad:
                self.names.append(prefix + name)
                self.params.append(p)
        if not self.params:
            raise ValueError("EMAWeights: no parameter with requires_grad")
        if len(set(self.names)) != len(self.names) or len({id(p) for p in self.params}) != len(self.params):
            raise ValueError("EMAWeights: duplicate parameter names or tensors")
        self.shadows = [p.detach().to(torch.float32, copy=True).contiguous() for p in self.params]
        self.num_updates = 0
        self._index = {id(p): i for i, p in enumerate(self.params)}
        self._applied = False
        self._optimizer = None       # the fused optimizer whose step() is this instance's update
        self._tables: Dict[tuple, dict] = {}

    # ---- schedule -------------------------------------------------------------------------------------------------------
    def decay_at(self, n: int) -> float:
        """Decay of update number `n` (counting from 0), in Python doubles."""
        return min(self.decay, (1.0 + n) / (10.0 + n)) if self.warmup else self.decay

    # ---- plumbing -------------------------------------------------------------------------------------------------------
    def _device(self) -> torch.device:
        """The one device of the parameters; shadows follow a model that was moved after construction."""
        dev = self.params[0].device
        for i, p in enumerate(self.params):
            if p.device != dev:
                raise CtsiError("EMAWeights: the parameters must live on one device")
            if self.shadows[i].device != dev:
                self.shadows[i] = self.shadows[i].to(dev)
        if dev.type != "cpu":
            for p in self.params:
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise CtsiError("EMAWeights runs on the HIP engine: device parameters must be contiguous fp32 tensors")
        return dev

    def shadow_of(self, p: torch.Tensor):
        """The shadow of parameter `p`, or None when `p` is not averaged."""
        i = self._index.get(id(p))
        return None if i is None else self.shadows[i]

    def _table(self, kind: str, idx: Tuple[int, ...], dev) -> dict:
        """Device tables of one launch over the parameters `idx`, rebuilt when a parameter or a shadow has moved."""
        ptrs = tuple((self.params[i].data_ptr(), self.shadows[i].data_ptr()) for i in idx)
        tb = self._tables.get((kind, idx))
        if tb is None or tb["ptrs"] != ptrs or tb["dev"] != dev:
            host = torch.zeros((len(idx), 4), dtype=torch.int64)
            for r, i in enumerate(idx):
                p, s = self.params[i], self.shadows[i]
                if kind == "ema":                      # CtsiEmaTensor: ema, p, numel, (group 0 | pad)
                    host[r, 0], host[r, 1], host[r, 2] = s.data_ptr(), p.data_ptr(), p.numel()
                else:                                  # CtsiSwapPair: a, b, numel, pad
                    host[r, 0], host[r, 1], host[r, 2] = p.data_ptr(), s.data_ptr(), p.numel()
            ck = chunk_table([self.params[i].numel() for i in idx], get_lib().adamw_chunk_elems())
            if len(self._tables) >= 4:                 # (the full set, and the few "no gradient this step" remainders)
                self._tables.clear()
            tb = self._tables[(kind, idx)] = dict(ptrs=ptrs, dev=dev, rows=host.to(dev), chunks=ck.to(dev), nchunks=len(ck),
                                                  weights=torch.empty(1, dtype=torch.float32, device=dev))
        return tb

    def _average(self, idx: Tuple[int, ...], w: float, dev) -> None:
        """shadow += w (p - shadow) for the parameters `idx`."""
        if not idx:
            return
        if dev.type == "cpu":
            with torch.no_grad():
                for i in idx:
                    self.shadows[i].lerp_(self.params[i].detach().to(torch.float32), w)
            return
        lib = get_lib()
        tb = self._table("ema", idx, dev)
        tb["weights"].copy_(torch.frombuffer(bytearray(struct.pack("<f", w)), dtype=torch.float32))
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            lib.ema_multi(C.c_void_p(tb["rows"].data_ptr()), C.c_void_p(tb["weights"].data_ptr()),
                          C.c_void_p(tb["chunks"].data_ptr()), tb["nchunks"], C.c_void_p(stream.cuda_stream))

    def _check_can_update(self, what: str) -> None:
        if self._applied:
            raise CtsiError(f"EMAWeights: {what} inside applied(): the parameters hold the averaged weights and the shadows "
                            "the raw ones; leave the block first")

    # ---- the update -----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self) -> None:
        """One `ctsi_ema_multi` launch over every shadow.  For users of a torch optimizer: call it after `optimizer.step()`.
        An instance handed to `FusedAdamW(ema=...)` is updated by that optimizer's `step()`; calling this as well would
        average twice per step, so it raises."""
        if self._optimizer is not None:
            raise CtsiError("EMAWeights.update(): this instance is attached to a fused optimizer, whose step() is the update")
        self._check_can_update("update()")
        dev = self._device()
        self._average(tuple(range(len(self.params))), 1.0 - self.decay_at(self.num_updates), dev)
        self.num_updates += 1

    def _attach(self, optimizer) -> None:
        if self._optimizer is not None and self._optimizer is not optimizer:
            raise CtsiError("EMAWeights: already attached to another optimizer")
        self._optimizer = optimizer

    def _fused_weight(self) -> float:
        """w = 1 - decay of the update the optimizer's launch is about to perform."""
        self._check_can_update("optimizer.step()")
        return 1.0 - self.decay_at(self.num_updates)

    def _fused_done(self, covered, w: float) -> None:
        """The optimizer's launch has averaged the parameters `covered`; every other shadow advances here, in one
        `ctsi_ema_multi` launch over the remainder, so that every shadow moves once per step()."""
        done = {id(p) for p in covered}
        rest = tuple(i for i, p in enumerate(self.params) if id(p) not in done)
        if rest:
            self._average(rest, w, self._device())
        self.num_updates += 1

    # ---- sampling with the averaged weights -----------------------------------------------------------------------------
    def _swap(self) -> None:
        dev = self._device()
        with torch.no_grad():
            if dev.type == "cpu":
                for p, s in zip(self.params, self.shadows):
                    tmp = p.detach().clone()
                    p.copy_(s.to(p.dtype))
                    s.copy_(tmp.to(torch.float32))
                return                                 # (copy_ has moved the version counters)
            tb = self._table("swap", tuple(range(len(self.params))), dev)
            stream = torch.cuda.current_stream(dev)
            with torch.cuda.device(dev):
                get_lib().swap_multi(C.c_void_p(tb["rows"].data_ptr()), C.c_void_p(tb["chunks"].data_ptr()), tb["nchunks"],
                                     C.c_void_p(stream.cuda_stream))
        bump_versions(self.params)

    @contextlib.contextmanager
    def applied(self):
        """Inside the block the model's parameters hold the averaged weights (one `ctsi_swap_multi` on entry, the same swap on
        exit: the restore is exact by construction).  The parameter versions move both times, so every cached engine program
        re-packs and the content-hashed weight cache serves both sets.  Not re-entrant; `update()` and an attached
        optimizer's `step()` raise inside the block."""
        if self._applied:
            raise CtsiError("EMAWeights.applied() is already active (nested entry)")
        self._swap()
        self._applied = True
        try:
            yield self
        finally:
            self._applied = False
            self._swap()

    # ---- state ----------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """{'decay', 'warmup', 'num_updates', 'shadow': {name: tensor}}; the tensors are the live shadows (as
        `Module.state_dict()` returns live parameters).  `model.load_state_dict(sd['shadow'], strict=False)` loads them."""
        if self._applied:
            raise CtsiError("EMAWeights.state_dict() inside applied(): the shadows hold the raw weights there")
        return {'decay': self.decay, 'warmup': self.warmup, 'num_updates': self.num_updates,
                'shadow': dict(zip(self.names, self.shadows))}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        if self._applied:
            raise CtsiError("EMAWeights.load_state_dict() inside applied()")
        shadow = sd['shadow']
        if set(shadow) != set(self.names):
            raise CtsiError(f"EMAWeights.load_state_dict: shadow names do not match the parameters: "
                            f"{sorted(set(shadow) ^ set(self.names))[:8]}")
        for name, s in zip(self.names, self.shadows):
            if tuple(shadow[name].shape) != tuple(s.shape):
                raise CtsiError(f"EMAWeights.load_state_dict: shape of '{name}' is {tuple(shadow[name].shape)}, "
                                f"the parameter's is {tuple(s.shape)}")
        for name, s in zip(self.names, self.shadows):
            s.copy_(shadow[name])                      # (in place: the shadows keep their addresses)
        self.decay, self.warmup, self.num_updates = float(sd['decay']), bool(sd['warmup']), int(sd['num_updates'])
