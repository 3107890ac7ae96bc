"""Training patches sampled on the device from volumes that stay in HBM.

The reference's `PatchSliceInterpolationDataset.__getitem__` (data/patch_slice_interpolation_dataset.py:236-274) unpickles a
whole patient file per item, cuts one patch and drops the rest.  Here the volumes are uploaded once (`DeviceVolumeStore`), the
random draws of a batch are made on the host in the reference's order (`DevicePatchSampler.draw`) and one HIP launch
(ctsi_patch_sample) cuts, resamples, flips and rotates the whole batch (`DevicePatchSampler.sample`).  `DevicePatchLoader`
is what the reference's `Trainer` iterates: collated batches of `data_contract` whose tensors are already on the device.
There is no CPU path: `sample` needs a ROCm device.
"""
from __future__ import annotations

import random
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import torch

from .data_contract import read_patient_cache
from .lib import CtsiError

# one row of `draw`: which volume, its sizes, the thin window's corner, the thick slice range, flip W | flip H << 1 | k << 2
COLS = 11
C_VOL, C_DTHIN, C_DTHICK, C_H, C_W, C_Z, C_Y0, C_X0, C_K0, C_K1, C_FLAGS = range(COLS)
TABLE_COLS = 12                     # CTSI_PATCH_COLS: the volume index becomes the two pointers
STORAGE = {torch.float32: 0, torch.float16: 1}      # CTSI_PATCH_F32 / CTSI_PATCH_F16
RING = 4                            # pinned staging slots of a sampler


class DeviceVolumeStore:
    """Patient volumes kept on the device, one (D, H, W) tensor per volume, in `dtype`: torch.float32 keeps the cache values
    exactly, torch.float16 stores x.half() (windowed CT has 401 levels in [-1, 1], a step of 5e-3, against an fp16 spacing of
    at most 4.9e-4)."""

    def __init__(self, device="cuda", dtype=torch.float16):
        if dtype not in STORAGE:
            raise ValueError(f"DeviceVolumeStore: dtype must be torch.float16 or torch.float32, got {dtype}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise CtsiError(f"DeviceVolumeStore keeps its volumes on a ROCm device (got '{self.device}'); there is no CPU path")
        self.dtype = dtype
        self.thin: List[torch.Tensor] = []
        self.thick: List[Optional[torch.Tensor]] = []
        self.categories: List[object] = []
        self.patient_ids: List[object] = []
        self.nbytes = 0

    def __len__(self) -> int:
        return len(self.thin)

    def _upload(self, v: torch.Tensor, name: str) -> torch.Tensor:
        need = v.numel() * torch.empty(0, dtype=self.dtype).element_size()
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > free:
            raise CtsiError(f"DeviceVolumeStore: {name} {tuple(v.shape)} needs {need} bytes as {self.dtype}, the store holds "
                            f"{self.nbytes} bytes in {len(self)} volumes and the device has {free} bytes free")
        out = torch.empty(tuple(v.shape[1:]), dtype=self.dtype, device=self.device)
        out.copy_(v[0].detach().to(self.dtype))
        self.nbytes += need
        return out

    def add(self, thick, thin, category="unknown", patient_id="") -> int:
        """One patient: (1, D_thick, H, W) and (1, D_thin, H, W) tensors, values as they come (the checks of
        data_contract.read_patient_cache).  `thick` may be None for a store that feeds thick='measure' samplers only.
        Returns the volume's index."""
        name = f"patient {patient_id!r}" if patient_id != "" else f"volume {len(self)}"
        for what, v in (("thick", thick), ("thin", thin)):
            if v is None and what == "thick":
                continue
            if not torch.is_tensor(v) or v.dim() != 4 or v.shape[0] != 1 or v.numel() == 0:
                raise ValueError(f"{name}: {what} volume must be a non-empty (1, D, H, W) tensor, got "
                                 f"{tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}")
        if thick is not None and tuple(thick.shape[2:]) != tuple(thin.shape[2:]):
            raise ValueError(f"{name}: thick {tuple(thick.shape)} and thin {tuple(thin.shape)} differ in H, W")
        t_thin = self._upload(thin, f"the thin volume of {name}")
        t_thick = None if thick is None else self._upload(thick, f"the thick volume of {name}")
        self.thin.append(t_thin)
        self.thick.append(t_thick)
        self.categories.append(category)
        self.patient_ids.append(patient_id)
        return len(self) - 1

    def add_file(self, path) -> int:
        d = read_patient_cache(path)
        return self.add(d["thick"], d["thin"], d["category"], d["patient_id"])

    def shape(self, index: int) -> Tuple[int, int, int, int]:
        """(D_thin, D_thick, H, W) of a volume; D_thick is 0 for a volume without a thick acquisition."""
        thin, thick = self.thin[index], self.thick[index]
        return int(thin.shape[0]), 0 if thick is None else int(thick.shape[0]), int(thin.shape[1]), int(thin.shape[2])


class DevicePatchSampler:
    """The patch pair of the reference's `extract_random_patch` + `augment_patch`, for a batch at a time.  `draw` makes the
    random choices on the host, `sample` runs them on the device.  thick='stored' resamples the stored thick slices as the
    reference does; thick='measure' computes the thick patch from the augmented thin one with the slice profile of data
    consistency (`profile`: the kind / fwhm / matrix arguments of consistency.DataConsistency)."""

    def __init__(self, store: DeviceVolumeStore, patch_depth_thin=48, patch_depth_thick=8, patch_size=(192, 192), augment=True,
                 seed=None, thick="stored", profile=None):
        if not isinstance(store, DeviceVolumeStore):
            raise ValueError(f"DevicePatchSampler: store must be a DeviceVolumeStore, got {type(store).__name__}")
        ph, pw = (int(s) for s in patch_size)
        if patch_depth_thin < 1 or patch_depth_thick < 1 or ph < 1 or pw < 1:
            raise ValueError(f"DevicePatchSampler: patch sizes must be positive, got depths {patch_depth_thin} / "
                             f"{patch_depth_thick}, patch {patch_size}")
        if augment and ph != pw:
            raise ValueError(f"augment=True needs a square patch, got {ph} x {pw}: a rotation by 90 degrees changes the "
                             f"shape of the item (the reference's collate fails there)")
        if thick not in ("stored", "measure"):
            raise ValueError(f"thick must be 'stored' or 'measure', got {thick!r}")
        if thick == "stored" and profile is not None:
            raise ValueError("profile= belongs to thick='measure'")
        self.store = store
        self.depth_thin, self.depth_thick, self.ph, self.pw = int(patch_depth_thin), int(patch_depth_thick), ph, pw
        self.augment, self.thick = bool(augment), thick
        self.rng = random.Random(seed)
        self.profile = None
        if thick == "measure":
            from .consistency import SliceProfile
            self.profile = SliceProfile(self.depth_thick, self.depth_thin, **dict(profile or {}))
        self._pinned: List[Optional[torch.Tensor]] = [None] * RING
        self._events: List[Optional[torch.cuda.Event]] = [None] * RING
        self._slot = 0

    # ---- host: the draws -------------------------------------------------------------------------------------
    def draw(self, indices: Sequence[int], rng: Optional[random.Random] = None) -> torch.Tensor:
        """(n, COLS) int64 on the CPU, one row per sample.  Per sample the `random.Random` calls are those of the reference, in
        its order: y0, x0, z (only when D_thin >= depth_thin), then with augment: flip W, flip H, k."""
        rng = self.rng if rng is None else rng
        rows = []
        for index in indices:
            index = int(index)
            d_thin, d_thick, h, w = self.store.shape(index)
            if self.thick == "stored" and d_thick == 0:
                raise ValueError(f"volume {index} has no thick acquisition: it serves thick='measure' samplers only")
            if h < self.ph or w < self.pw:
                raise ValueError(f"Volume size ({h}, {w}) smaller than patch size ({self.ph}, {self.pw})")
            y0 = rng.randint(0, h - self.ph)
            x0 = rng.randint(0, w - self.pw)
            z = rng.randint(0, d_thin - self.depth_thin) if d_thin >= self.depth_thin else 0
            z1 = min(z + self.depth_thin, d_thin)
            k0 = k1 = 0
            if d_thick:         # data_contract.aligned_patch: Python float division, int() truncation
                k0 = max(0, int(z * d_thick / d_thin))
                k1 = min(d_thick, max(int(z1 * d_thick / d_thin), k0 + 1))
            flags = 0
            if self.augment:
                flags |= 1 if rng.random() > 0.5 else 0
                flags |= 2 if rng.random() > 0.5 else 0
                flags |= rng.randint(0, 3) << 2
            rows.append([index, d_thin, d_thick, h, w, z, y0, x0, k0, k1, flags])
        return torch.tensor(rows, dtype=torch.int64).reshape(-1, COLS)

    def check_rows(self, rows: torch.Tensor) -> None:
        """The kernel trusts its table; every row is held against the store here, on the host, before it goes up."""
        if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.is_cuda or rows.dim() != 2 or rows.shape[1] != COLS \
                or rows.shape[0] < 1:
            raise ValueError(f"sample: rows must be a CPU int64 tensor (n >= 1, {COLS}), as draw() returns")
        for r in rows.tolist():
            index = r[C_VOL]
            if not 0 <= index < len(self.store):
                raise ValueError(f"sample: row names volume {index}, the store holds {len(self.store)}")
            d_thin, d_thick, h, w = self.store.shape(index)
            if (r[C_DTHIN], r[C_DTHICK], r[C_H], r[C_W]) != (d_thin, d_thick, h, w):
                raise ValueError(f"sample: row carries sizes {tuple(r[C_DTHIN:C_W + 1])}, volume {index} has "
                                 f"{(d_thin, d_thick, h, w)}")
            ok = 0 <= r[C_Y0] <= h - self.ph and 0 <= r[C_X0] <= w - self.pw and 0 <= r[C_Z] < d_thin \
                and 0 <= r[C_FLAGS] < 16 and (self.ph == self.pw or not (r[C_FLAGS] >> 2) & 1)
            if self.thick == "stored":
                ok = ok and 0 <= r[C_K0] < r[C_K1] <= d_thick
            if not ok:
                raise ValueError(f"sample: row {r} does not fit volume {index} {(d_thin, d_thick, h, w)} with patch "
                                 f"{(self.depth_thin, self.depth_thick, self.ph, self.pw)}")

    # ---- device ----------------------------------------------------------------------------------------------
    def _stage(self, table: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """The next pinned slot holding `table`.  events[i] is recorded on the engine stream right behind the copy OUT of
        pinned[i]; the slot is rewritten only after that event has completed -- RING uses later, so in steady state the
        query is true and the host never waits."""
        i = self._slot
        self._slot = (i + 1) % RING
        ev = self._events[i]
        if ev is not None and not ev.query():
            ev.synchronize()
        if self._pinned[i] is None or self._pinned[i].shape[0] < table.shape[0]:
            self._pinned[i] = torch.empty((table.shape[0], TABLE_COLS), dtype=torch.int64, pin_memory=True)
        slot = self._pinned[i][:table.shape[0]]
        slot.copy_(table)
        return slot, i

    def sample(self, rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(thick (n, 1, Dk, ph, pw), thin (n, 1, Dt, ph, pw)) fp32 on the device for the rows of `draw`: one
        ctsi_patch_sample launch on the engine stream, no host synchronisation."""
        from .engine import Ctx, _ptr
        self.check_rows(rows)
        n = rows.shape[0]
        store, stored = self.store, self.thick == "stored"
        table = torch.empty((n, TABLE_COLS), dtype=torch.int64)
        table[:, 2:] = rows[:, 1:]
        for i, index in enumerate(rows[:, C_VOL].tolist()):
            table[i, 0] = store.thin[index].data_ptr()
            table[i, 1] = store.thick[index].data_ptr() if stored else 0
        ctx = Ctx.get(store.device)
        with ctx.scope():
            slot, i = self._stage(table)
            dev_table = torch.empty((n, TABLE_COLS), dtype=torch.int64, device=store.device)
            dev_table.copy_(slot, non_blocking=True)
            if self._events[i] is None:
                self._events[i] = torch.cuda.Event()
            self._events[i].record(ctx.stream)
            thin = torch.empty((n, 1, self.depth_thin, self.ph, self.pw), dtype=torch.float32, device=store.device)
            thick = torch.empty((n, 1, self.depth_thick, self.ph, self.pw), dtype=torch.float32, device=store.device) \
                if stored else None
            ctx.lib.patch_sample(_ptr(dev_table), n, STORAGE[store.dtype], self.depth_thin, self.depth_thick if stored else 0,
                                 self.ph, self.pw, _ptr(thin), _ptr(thick), ctx.sptr)
        if not stored:
            thick = self.profile.measure(thin)
        return thick, thin


class _PatchDataset:
    """What `loader.dataset` is asked for: its length."""

    def __init__(self, n: int):
        self._n = n

    def __len__(self) -> int:
        return self._n


class DevicePatchLoader:
    """The loader the reference's `Trainer` iterates: each item is the collated dict of data_contract -- 'input', 'target',
    'x_lr', 'x_hr' device tensors ('input' is 'x_lr'), 'category' and 'patient_id' lists.  An epoch visits every volume
    `patches_per_volume` times in the order of random.Random(seed + epoch).shuffle; the draws come from one
    random.Random(seed) of the loader, so the same seed gives the same batches bit for bit."""

    def __init__(self, sampler: DevicePatchSampler, batch_size=8, shuffle=True, drop_last=True, seed=42, patches_per_volume=1):
        if not isinstance(batch_size, int) or batch_size < 1 or not isinstance(patches_per_volume, int) or patches_per_volume < 1:
            raise ValueError(f"batch_size and patches_per_volume must be positive integers, got {batch_size!r}, "
                             f"{patches_per_volume!r}")
        self.sampler, self.batch_size, self.shuffle, self.drop_last = sampler, batch_size, bool(shuffle), bool(drop_last)
        self.seed, self.patches_per_volume = int(seed), patches_per_volume
        self.dataset = _PatchDataset(len(sampler.store) * patches_per_volume)
        self.rng = random.Random(self.seed)
        self.epoch = 0

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self) -> Iterator[Dict[str, object]]:
        store = self.sampler.store
        order = [i for i in range(len(store)) for _ in range(self.patches_per_volume)]
        if self.shuffle:
            random.Random(self.seed + self.epoch).shuffle(order)
        self.epoch += 1
        for b in range(len(self)):
            idx = order[b * self.batch_size:(b + 1) * self.batch_size]
            thick, thin = self.sampler.sample(self.sampler.draw(idx, rng=self.rng))
            yield {"x_lr": thick, "x_hr": thin, "input": thick, "target": thin,
                   "category": [store.categories[i] for i in idx], "patient_id": [store.patient_ids[i] for i in idx]}
