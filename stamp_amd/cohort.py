"""A cohort's tile features resident in HBM, feeding the MIL trainers: one gather launch per training batch, zero-copy views for validation.

`bags.tile_bag_dataloader` restates the reference's feed (src/stamp/modeling/data.py:532-655): every epoch, for every patient, a DataLoader worker reads all of
the patient's `.h5` files again, converts them to fp32, samples a bag, and the batch crosses PCIe as fp32.  A cohort fits on the card (1 000 patients x 10 k
tiles x 1 024 fp16 features = 20 GB of 288 GB), so `ResidentCohort` reads every file ONCE, keeps the rows packed in device memory in the files' own precision

    feats  [R, F]   fp16 when every file is fp16, else fp32      patient p = rows offsets[p] .. offsets[p] + lengths[p]
    coords [R, 2]   fp32 micrometres (h5io.get_coords)           (its slides concatenated in the order of its file list, as BagDataset does)

and builds a training batch with one `amds_bag_batch_gather` launch (csrc/bag_batch.hip: gather + `.float()` + zero padding of `_to_fixed_size_bag`,
data.py:811-862, optionally the reference's `vary_precision` transform).  The packed store IS the layout the ragged inference forwards take
(`mil_core.RaggedBags`), so a validation group is a view: a row slice and rebased offsets, no copy.

Random draws, per epoch of `train_batches`, from `generator` (None: torch's global CPU generator), in this order:
  1. shuffle: ONE `torch.randperm(len(view))` -- the patient order of the epoch;
  2. the bags' own draws
       sampler="torch" (default): `mil.fixed_size_bag_indices` per patient in that order (a `torch.randperm(n)` for every patient with more than `bag_size`
         tiles): exactly what fetching `BagDataset` items in that order with `num_workers=0` consumes;
       sampler="device": nothing from `generator`.  ONE `amds_bag_plan` launch draws `randperm(n)[:bag_size]` for every patient of the epoch as a bijection
         keyed on (`seed`, e, store patient index), e = how often the callable `train_batches` returned has been invoked before (0 for the first epoch).  A
         patient's bag depends on that key alone -- not on its place in the epoch, its batch, or the view it is reached through.  That is the reference's
         distribution, not torch's random stream (include/amdstamp.h, amds_bag_plan); it needs shuffle=True (the equidistant plan stays on the host);
  3. with `vary_precision_bits`: one `torch.randint` = the epoch's mask seed; batch j masks with (seed, stream_id = j) through the library's counter-based
     hash.  That is the reference transform's distribution, not torch's random stream (include/amdstamp.h, amds_bag_batch_gather).
With the host sampler the epoch's whole index plan is built on the host and uploaded once; with the device sampler only the patient order is.  The loop then only
launches (no host synchronisation).

`ResidentCohort.view(patients)` is a `CohortView`: a list of store patients over the SAME tensors (no copy) with the cohort's own batch methods -- the folds of
`crossval.crossval` are views of one cohort, read once.  The cohort's methods are those of the view over all its patients.
There is no spilling: a cohort that does not fit `max_bytes` or the free device memory is refused before anything is allocated.  One device; no CPU fallback."""
from __future__ import annotations

import time
from collections.abc import Iterable, Sequence
from typing import Any

import numpy as np
import torch

from . import h5io
from .bags import PatientData, parse_targets

MAX_ROWS = 2 ** 31 - 1          # the ragged forwards address tile rows with 32-bit offsets


def plan_indices(offsets: Sequence[int], lengths: Sequence[int], patients: Iterable[int], bag_size: int, deterministic: bool = False,
                 generator: torch.Generator | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (idx int64 [B, bag_size] of absolute store rows, -1 = padding row; bag_sizes int64 [B] = min(bag_size, tiles)) for the patients of a batch (or of a
    whole epoch) in the given order: `mil.fixed_size_bag_indices` per patient, so a seeded generator is consumed exactly as by `BagDataset` items fetched in
    that order.  Host only."""
    from .mil import fixed_size_bag_indices
    if bag_size < 1:
        raise ValueError("bag_size must be >= 1")
    patients = [int(p) for p in patients]
    idx = torch.full((len(patients), int(bag_size)), -1, dtype=torch.int64)
    sizes = torch.empty(len(patients), dtype=torch.int64)
    for b, p in enumerate(patients):
        local = fixed_size_bag_indices(int(lengths[p]), int(bag_size), deterministic, generator)
        idx[b, :local.numel()] = local + int(offsets[p])
        sizes[b] = local.numel()
    return idx, sizes


def _check_size(nbytes: int, max_bytes: int | None, device) -> None:
    if max_bytes is not None and nbytes > max_bytes:
        raise ValueError(f"the cohort needs {nbytes} bytes of device memory, max_bytes allows {int(max_bytes)} (there is no spilling)")
    free = torch.cuda.mem_get_info(device)[0]
    if nbytes > free:
        raise ValueError(f"the cohort needs {nbytes} bytes of device memory, {free} are free on {device} (there is no spilling)")


class ResidentCohort:
    def __init__(self, patient_data: Sequence[PatientData] | None = None, *, task: str, categories: Sequence[str] | None = None, device="cuda",
                 max_bytes: int | None = None, feature_files: Sequence[Iterable] | None = None, ground_truths: Sequence[Any] | None = None) -> None:
        """patient_data (or `feature_files` per patient + `ground_truths`), `task` / `categories` as `bags.parse_targets` takes them.  Files are read as
        `BagDataset.__getitem__` reads them (`feats` or `patch_embeddings`, `h5io.get_coords`, a patient's slides concatenated in order), one patient at a
        time through a pinned staging buffer: the host never holds more than two patients."""
        if patient_data is None:
            if feature_files is None or ground_truths is None or len(feature_files) != len(ground_truths):
                raise ValueError("give patient_data, or feature_files and as many ground_truths")
            patient_data = [PatientData(ground_truth=g, feature_files=f) for f, g in zip(feature_files, ground_truths)]
        self.files = [[f for f in p.feature_files] for p in patient_data]
        self.targets, self.categories = parse_targets(patient_data=patient_data, task=task, categories=categories)
        self.multi_target = isinstance(self.targets, list)
        self.device = torch.device(device)
        # ---- pass 1: dataset headers -> rows per patient, feature width, precision; the refusal comes before any allocation
        shapes = [[h5io.feature_shape(f) for f in fs] for fs in self.files]
        widths = {s[1] for ps in shapes for s in ps}
        if len(widths) != 1:
            raise ValueError(f"the cohort's files must share one feature width, got {sorted(widths)}")
        self.n_feats = widths.pop()
        self.dtype = torch.float16 if all(s[2] == np.float16 for ps in shapes for s in ps) else torch.float32
        self.lengths = [sum(s[0] for s in ps) for ps in shapes]
        self.offsets = [0]
        for n in self.lengths:
            self.offsets.append(self.offsets[-1] + n)
        R = self.offsets[-1]
        if R > MAX_ROWS:
            raise ValueError(f"{R} tile rows do not fit the 32-bit row index (at most {MAX_ROWS})")
        item = 2 if self.dtype == torch.float16 else 4
        self.nbytes = R * (self.n_feats * item + 8)
        _check_size(self.nbytes, max_bytes, self.device)
        # ---- pass 2: read and upload
        t0 = time.perf_counter()
        self.feats = torch.empty(R, self.n_feats, dtype=self.dtype, device=self.device)
        self.coords = torch.empty(R, 2, dtype=torch.float32, device=self.device)
        self._upload(max(self.lengths, default=0), item)
        self._offsets_dev = torch.tensor(self.offsets, dtype=torch.int32).to(self.device)
        self._lengths_dev = torch.tensor(self.lengths, dtype=torch.int64).to(self.device)
        if self.multi_target:
            self._targets_dev = {k: torch.stack([t[k] for t in self.targets]).to(self.device) for k in (self.targets[0] if self.targets else {})}
        else:
            self._targets_dev = self.targets.to(self.device)
        torch.cuda.synchronize(self.device)
        self.load_seconds = time.perf_counter() - t0

    def _upload(self, max_rows: int, item: int) -> None:
        Fd, dev = self.n_feats, self.device
        stage = [(torch.empty(max(max_rows, 1) * Fd, dtype=self.dtype).pin_memory(), torch.empty(max(max_rows, 1) * 2, dtype=torch.float32).pin_memory(),
                  torch.cuda.Event()) for _ in range(2)]
        used = [False, False]
        for p, fs in enumerate(self.files):
            fbuf, cbuf, ev = stage[p % 2]
            if used[p % 2]:
                ev.synchronize()                  # the copy that last read this staging buffer has finished
            n, o = self.lengths[p], 0
            fv, cv = fbuf[:n * Fd].view(n, Fd), cbuf[:n * 2].view(n, 2)
            for f in fs:
                d, a = h5io.read_file(f)
                if h5io.feature_type(a) in ("slide", "patient"):
                    raise ValueError(f"{f}: {h5io.feature_type(a)}-level features; a resident cohort takes tile-level feature files "
                                     "(one vector per slide or patient goes into cohort.ResidentFeatureTable, which crossval builds for such files)")
                x = np.asarray(d["feats"] if "feats" in d else d["patch_embeddings"])
                c = np.asarray(h5io.get_coords(d, a).coords_um)
                if o + x.shape[0] > n or x.shape[1] != Fd or c.shape != (x.shape[0], 2):
                    raise RuntimeError(f"{f}: shape {x.shape} / coords {c.shape} differ from the file's header (changed while loading?)")
                fv[o:o + x.shape[0]].copy_(torch.from_numpy(np.ascontiguousarray(x)))           # (the `.float()` of data.py:617 when the store is fp32)
                cv[o:o + x.shape[0]].copy_(torch.from_numpy(np.ascontiguousarray(c)))
                o += x.shape[0]
            if o != n:
                raise RuntimeError(f"patient {p}: read {o} rows, the headers announced {n}")
            a0 = self.offsets[p]
            self.feats[a0:a0 + n].copy_(fv, non_blocking=True)
            self.coords[a0:a0 + n].copy_(cv, non_blocking=True)
            ev.record()
            used[p % 2] = True

    def __len__(self) -> int:
        return len(self.lengths)

    # ---- index planning (host) -----------------------------------------------------------------------------------------------------------------
    def plan_indices(self, patients: Iterable[int], bag_size: int, deterministic: bool = False, generator: torch.Generator | None = None):
        """`plan_indices` of this cohort's offsets and lengths."""
        return plan_indices(self.offsets, self.lengths, patients, bag_size, deterministic, generator)

    def _targets_of(self, sel: torch.Tensor):
        if self.multi_target:
            return {k: v[sel] for k, v in self._targets_dev.items()}          # the dict `bags.collate_multitarget` builds
        return self._targets_dev[sel]

    # ---- views: a list of patients over the same store -------------------------------------------------------------------------------------------
    def view(self, patients: Iterable[int]) -> "CohortView":
        """The patients `patients` (store indices, in that order) as a `CohortView`: the folds of a cross-validation are views of ONE cohort."""
        return CohortView(self, patients)

    def _all(self) -> "CohortView":
        return CohortView(self, range(len(self)))

    def train_batches(self, batch_size: int, bag_size: int, shuffle: bool = True, generator: torch.Generator | None = None,
                      out_dtype: torch.dtype = torch.float32, vary_precision_bits: int | None = None, drop_last: bool = False, sampler: str = "torch",
                      seed: int = 0):
        """`CohortView.train_batches` of all patients."""
        return self._all().train_batches(batch_size, bag_size, shuffle, generator, out_dtype, vary_precision_bits, drop_last, sampler, seed)

    def barspoon_batches(self, batch_size: int, bag_size: int, shuffle: bool = True, generator: torch.Generator | None = None,
                         out_dtype: torch.dtype = torch.float32, vary_precision_bits: int | None = None, drop_last: bool = False, sampler: str = "torch",
                         seed: int = 0):
        """`CohortView.barspoon_batches` of all patients."""
        return self._all().barspoon_batches(batch_size, bag_size, shuffle, generator, out_dtype, vary_precision_bits, drop_last, sampler, seed)

    def valid_batches(self):
        """`CohortView.valid_batches` of all patients."""
        return self._all().valid_batches()

    def barspoon_valid_batches(self):
        return self._all().barspoon_valid_batches()

    def ragged_group(self, a: int, e: int):
        """Patients a .. e - 1 as `mil_core.RaggedBags` for the ragged inference forwards: a row slice of the features and of the coordinates, offsets rebased
        to the slice -- views and one small subtraction, no concatenation."""
        from .mil_core import RaggedBags
        if not 0 <= a <= e <= len(self):
            raise ValueError(f"patients {a}..{e} outside 0..{len(self)}")
        r0, r1 = self.offsets[a], self.offsets[e]
        return RaggedBags(self.feats[r0:r1], self.coords[r0:r1], self._offsets_dev[a:e + 1] - r0, tuple(self.lengths[a:e]))


SAMPLERS = ("torch", "device")


class CohortView:
    """A list of store patient indices over a `ResidentCohort`'s own `feats` / `coords` / target tensors: nothing is copied.  With `sampler="torch"` a view over
    the patients S draws from `generator` exactly what a separate `ResidentCohort` built from `[patient_data[i] for i in S]` draws (one `randperm(len(S))`, then
    `mil.fixed_size_bag_indices` per patient, which consumes by the patient's length only), so its batches are bit-identical to that cohort's."""

    def __init__(self, cohort: ResidentCohort, patients: Iterable[int]) -> None:
        self.cohort = cohort
        self.patients = [int(p) for p in patients]
        bad = [p for p in self.patients if not 0 <= p < len(cohort)]
        if bad:
            raise ValueError(f"patients {bad[:8]} outside 0..{len(cohort)}")
        self._patients_t = torch.tensor(self.patients, dtype=torch.int64)
        self._patients_dev = None

    def __len__(self) -> int:
        return len(self.patients)

    def _on_device(self) -> torch.Tensor:
        if self._patients_dev is None:
            self._patients_dev = self._patients_t.to(self.cohort.device)
        return self._patients_dev

    # ---- training batches ------------------------------------------------------------------------------------------------------------------------
    def _epoch(self, batch_size, bag_size, shuffle, generator, out_dtype, vary_precision_bits, drop_last, with_sizes, sampler, plan_seed, epoch):
        from . import ops
        c = self.cohort
        N = len(self)
        order = torch.randperm(N, generator=generator) if shuffle else torch.arange(N)
        if drop_last:
            order = order[:N - N % batch_size]
        if sampler == "device":
            idx = sizes = None                      # planned on the device, below: no per-patient draw on the host
        else:
            idx, sizes = c.plan_indices(self._patients_t[order].tolist(), bag_size, deterministic=not shuffle, generator=generator)
        bits = int(vary_precision_bits or 0)
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item()) if bits else 0
        if sampler == "device":
            order = self._on_device()[order.to(c.device)]          # store patient indices in the epoch's order
            idx, sizes = ops.bag_plan(c._offsets_dev, order, bag_size, plan_seed, epoch)
        else:
            idx, sizes, order = idx.to(c.device), sizes.to(c.device), self._patients_t[order].to(c.device)          # the epoch's plan: uploaded once
        for j, a in enumerate(range(0, order.numel(), batch_size)):
            e = min(a + batch_size, order.numel())
            bags, coords = ops.bag_batch_gather(c.feats, c.coords, idx[a:e], out_dtype, vary_precision_bits=bits, seed=seed, stream_id=j)
            targets = c._targets_of(order[a:e])
            yield (bags, coords, sizes[a:e], targets) if with_sizes else (bags, coords, targets)

    def _feed(self, batch_size, bag_size, shuffle, generator, out_dtype, vary_precision_bits, drop_last, with_sizes, sampler, seed):
        if batch_size < 1 or bag_size < 1:
            raise ValueError("batch_size and bag_size must be >= 1")
        if sampler not in SAMPLERS:
            raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
        if sampler == "device" and not shuffle:
            raise ValueError('sampler="device" draws random bags; shuffle=False asks for the equidistant plan, which is deterministic and stays on the host')
        count = iter(range(2 ** 32))          # the epoch number of the device sampler: invocations of the returned callable, from 0
        return lambda: self._epoch(batch_size, bag_size, shuffle, generator, out_dtype, vary_precision_bits, drop_last, with_sizes, sampler, int(seed),
                                   next(count))

    def train_batches(self, batch_size: int, bag_size: int, shuffle: bool = True, generator: torch.Generator | None = None,
                      out_dtype: torch.dtype = torch.float32, vary_precision_bits: int | None = None, drop_last: bool = False, sampler: str = "torch",
                      seed: int = 0):
        """-> the callable `mil_train.fit` takes: per epoch an iterable of (bags [B, bag_size, F] `out_dtype`, coords fp32 [B, bag_size, 2], bag_sizes int64
        [B], targets [B, D] -- or the dict of a multi-target cohort) on the device.  Sampling is random when shuffling and equidistant when not, like
        `tile_bag_dataloader`.  sampler="torch": the bags' draws come from `generator` on the host; sampler="device": from ONE amds_bag_plan launch keyed
        (`seed`, epoch = number of earlier invocations of the returned callable, store patient index).  The draws and their order: module docstring."""
        return self._feed(batch_size, bag_size, shuffle, generator, out_dtype, vary_precision_bits, drop_last, True, sampler, seed)

    def barspoon_batches(self, batch_size: int, bag_size: int, shuffle: bool = True, generator: torch.Generator | None = None,
                         out_dtype: torch.dtype = torch.float32, vary_precision_bits: int | None = None, drop_last: bool = False, sampler: str = "torch",
                         seed: int = 0):
        """`train_batches` as the (feats, positions, targets) 3-tuples `HipBarspoonTrainer.fit` takes."""
        return self._feed(batch_size, bag_size, shuffle, generator, out_dtype, vary_precision_bits, drop_last, False, sampler, seed)

    # ---- validation: views of the store ----------------------------------------------------------------------------------------------------------
    def _valid(self, with_sizes):
        c = self.cohort
        for p in self.patients:
            a, n = c.offsets[p], c.lengths[p]
            item = (c.feats[a:a + n].unsqueeze(0), c.coords[a:a + n].unsqueeze(0))
            targets = {k: v[p:p + 1] for k, v in c._targets_dev.items()} if c.multi_target else c._targets_dev[p:p + 1]
            yield (*item, c._lengths_dev[p:p + 1], targets) if with_sizes else (*item, targets)

    def valid_batches(self):
        """-> the callable `fit` takes for validation: one whole bag per batch (the reference's `bag_size=None`, batch 1 loader), every tensor a view of the
        store (features in the store's precision)."""
        return lambda: self._valid(True)

    def barspoon_valid_batches(self):
        return lambda: self._valid(False)

    def ragged_group(self, a: int, e: int):
        """Patients a .. e - 1 of the view as `mil_core.RaggedBags` (`ResidentCohort.ragged_group`): they must be consecutive in the store, since the group is
        one row slice; ValueError otherwise."""
        if not 0 <= a <= e <= len(self):
            raise ValueError(f"patients {a}..{e} outside 0..{len(self)}")
        p0 = self.patients[a] if a < e else 0
        if self.patients[a:e] != list(range(p0, p0 + e - a)):
            raise ValueError(f"patients {a}..{e} of the view are not consecutive in the store: {self.patients[a:e][:8]}...")
        return self.cohort.ragged_group(p0, p0 + e - a)


# ---- slide- / patient-level feature vectors: one row per entry ---------------------------------------------------------------------------------------
def parse_survival_status(value) -> int:
    """The reference's `_parse_survival_status` (data.py:1164-1201): known spellings first, then any number (> 0 is an event; "nan" compares false: 0)."""
    s = str(value).strip().lower()
    if s in {"1", "event", "dead", "deceased", "yes", "y", "true"}:
        return 1
    if s in {"0", "alive", "censored", "no", "false"}:
        return 0
    try:
        return 1 if float(s) > 0 else 0
    except ValueError:
        raise ValueError(f"Unrecognized survival status: {value!r} (expected dead / alive, event / censored, yes / no, true / false or a number)") from None


def feature_table_labels(patient_data: Sequence[PatientData], task: str, categories: Sequence[str] | None = None) -> tuple[torch.Tensor, list]:
    """-> (labels, categories) exactly as the slide / patient branch of the reference's `create_dataloader` builds them (data.py:359-406): classification a float
    one-hot [N, C] in the order of `categories` (default: the sorted unique labels); regression float [N, 1]; survival float [N, 2] = (time, event), the time
    NaN when missing or unparsable, the event through `parse_survival_status` (a ground truth that is no (time, event) pair is a time with an unknown status,
    which parses as 0).  Multi-target (dict) ground truths are refused like there."""
    gts = [p.ground_truth for p in patient_data]
    if any(isinstance(g, dict) for g in gts):
        raise ValueError("multi-target ground truths are not supported on slide- / patient-level features; provide a single target per entry")
    if task == "classification":
        raw = np.array(gts)
        cats = list(categories) if categories else [c.item() for c in np.unique(raw)]
        return torch.tensor(raw.reshape(-1, 1) == np.array(cats, dtype=object).reshape(1, -1), dtype=torch.float32).reshape(len(gts), len(cats)), cats
    if task == "regression":
        if any(g is None for g in gts):
            raise ValueError("regression on a feature table needs a numeric target for every entry")
        return torch.tensor([float(g) for g in gts], dtype=torch.float32).reshape(-1, 1), []
    if task == "survival":
        times, events = [], []
        for g in gts:
            if isinstance(g, (tuple, list)) and len(g) == 2:
                t, e = g
            elif g is None:
                t, e = None, None
            else:
                t, e = str(g), "nan"
            if t is None:
                times.append(np.nan)
            elif isinstance(t, str):
                try:
                    times.append(np.nan if t.lower() == "nan" else float(t))
                except ValueError:
                    times.append(np.nan)
            else:
                times.append(float(t))
            events.append(parse_survival_status(e))
        return torch.tensor(np.column_stack([times, events]).reshape(-1, 2), dtype=torch.float32), []
    raise ValueError(f"Unsupported task: {task}")


def read_feature_vector(path) -> np.ndarray:
    """One slide- / patient-level file -> its vector [F], by the rule of the reference's `PatientFeatureDataset.__getitem__` (data.py:690-723): `feats` of shape
    [F] or [1, F]; a tile-level file (`h5io.feature_type`) is refused."""
    d, a = h5io.read_file(path)
    if h5io.feature_type(a) == "tile":
        raise ValueError(f"{path}: tile-level features; a feature table takes slide- or patient-level files (tile bags go into a ResidentCohort)")
    if "feats" not in d:
        raise RuntimeError(f"{path}: no 'feats' dataset")
    x = np.asarray(d["feats"])
    if x.ndim == 2 and x.shape[0] == 1:
        x = x[0]
    elif x.ndim != 1:
        raise RuntimeError(f"Expected single feature vector (shape [F] or [1, F]), got {tuple(x.shape)} in {path}. Check that the features are patient-level.")
    return x


class ResidentFeatureTable:
    """One feature vector per entry (a slide or a patient), resident in device memory: the feed of `mlp_train.HipMlpTrainer` under `mil_train.fit` and
    `crossval.crossval`.  The reference's loader (data.py:355-419) opens every entry's file again for every item of every epoch; the whole table of a cohort
    is a few megabytes (1 000 entries x 2 560 fp16 features = 5 MB), so every file is read ONCE through `h5io.read_file`.

        feats [N, F]   fp16 when every file is fp16, else fp32        targets [N, C] / [N, 1] / [N, 2]  (`feature_table_labels`)

    An entry's file is the FIRST of its `feature_files` (`next(iter(p.feature_files))`, data.py:357).  Batches follow `ResidentCohort`'s protocol; `view(entries)`
    is a `FeatureTableView` over the same tensors.  No spilling: the size is checked before any allocation.  One device."""

    def __init__(self, patient_data: Sequence[PatientData], *, task: str, categories: Sequence[str] | None = None, device="cuda", max_bytes: int | None = None) -> None:
        self.files = [next(iter(p.feature_files)) for p in patient_data]
        self.targets, self.categories = feature_table_labels(patient_data, task, categories)
        self.task = task
        self.device = torch.device(device)
        rows = [read_feature_vector(f) for f in self.files]
        widths = {int(r.shape[0]) for r in rows}
        if len(widths) > 1:
            raise ValueError(f"the table's files must share one feature width, got {sorted(widths)}")
        self.n_feats = widths.pop() if widths else 0
        self.dtype = torch.float16 if rows and all(r.dtype == np.float16 for r in rows) else torch.float32
        self.nbytes = len(rows) * self.n_feats * (2 if self.dtype == torch.float16 else 4)
        if self.device.type == "cuda":
            _check_size(self.nbytes, max_bytes, self.device)
        elif max_bytes is not None and self.nbytes > max_bytes:
            raise ValueError(f"the table needs {self.nbytes} bytes, max_bytes allows {int(max_bytes)} (there is no spilling)")
        host = torch.empty(len(rows), self.n_feats, dtype=self.dtype)
        for i, r in enumerate(rows):
            host[i].copy_(torch.from_numpy(np.ascontiguousarray(r)))          # (the `.float()` of the reference's step when the store is fp32)
        self.feats = host.to(self.device)
        self._targets_dev = self.targets.to(self.device)

    def __len__(self) -> int:
        return len(self.files)

    def view(self, entries: Iterable[int]) -> "FeatureTableView":
        """The entries `entries` (store indices, in that order) as a `FeatureTableView`: the folds of a cross-validation are views of ONE table."""
        return FeatureTableView(self, entries)

    def _all(self) -> "FeatureTableView":
        return FeatureTableView(self, range(len(self)))

    def train_batches(self, batch_size: int, shuffle: bool = True, generator: torch.Generator | None = None, drop_last: bool = False):
        """`FeatureTableView.train_batches` of all entries."""
        return self._all().train_batches(batch_size, shuffle, generator, drop_last)

    def valid_batches(self):
        """`FeatureTableView.valid_batches` of all entries."""
        return self._all().valid_batches()


class FeatureTableView:
    """A list of store entries over a `ResidentFeatureTable`'s own tensors: nothing is copied."""

    def __init__(self, table: ResidentFeatureTable, entries: Iterable[int]) -> None:
        self.table = table
        self.entries = [int(e) for e in entries]
        bad = [e for e in self.entries if not 0 <= e < len(table)]
        if bad:
            raise ValueError(f"entries {bad[:8]} outside 0..{len(table)}")
        self._entries_t = torch.tensor(self.entries, dtype=torch.int64)

    def __len__(self) -> int:
        return len(self.entries)

    def epoch_plan(self, batch_size: int, shuffle: bool = True, generator: torch.Generator | None = None, drop_last: bool = False) -> list[torch.Tensor]:
        """The batches of one epoch as int64 tensors of STORE rows (host): ONE `torch.randperm(len(view))` from `generator` when shuffling (the cohort's rule 1),
        then consecutive groups of `batch_size`; the shorter tail batch is kept unless `drop_last`."""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        N = len(self)
        order = torch.randperm(N, generator=generator) if shuffle else torch.arange(N)
        if drop_last:
            order = order[:N - N % batch_size]
        rows = self._entries_t[order]
        return [rows[a:a + batch_size] for a in range(0, rows.numel(), batch_size)]

    def _epoch(self, batch_size, shuffle, generator, drop_last):
        from . import ops
        t = self.table
        if t.device.type != "cuda":
            raise RuntimeError("a feature table's batches are gathered on the GPU (no CPU fallback)")
        plan = self.epoch_plan(batch_size, shuffle, generator, drop_last)
        if not plan:
            return
        rows = torch.cat(plan).to(t.device)          # the epoch's plan: uploaded once
        a = 0
        for b in plan:
            idx = rows[a:a + b.numel()]
            a += b.numel()
            # amds_gather_rows: the bits of `feats[idx].float()`
            yield ops.gather_rows(t.feats, idx, idx.numel(), torch.float32), None, None, t._targets_dev[idx]

    def train_batches(self, batch_size: int, shuffle: bool = True, generator: torch.Generator | None = None, drop_last: bool = False):
        """-> the callable `mil_train.fit` takes: per epoch an iterable of (feats fp32 [B, F], None, None, targets [B, D]) on the device, one amds_gather_rows
        launch per batch."""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        return lambda: self._epoch(batch_size, shuffle, generator, drop_last)

    def _valid(self):
        t = self.table
        for e in self.entries:
            yield t.feats[e:e + 1], None, None, t._targets_dev[e:e + 1]

    def valid_batches(self):
        """-> the callable `fit` takes for validation: one entry per batch in the view's order ([1, F] views of the store in its own precision, no copy): the
        reference's batch-1 validation loader (src/stamp/modeling/train.py:467-477).  The callable also has `block()` -> (feats [N, F], targets [N, D]): the
        same entries in the same order as ONE gather of the store, for a caller that runs them through one forward (`fit(objective="library")`)."""
        return _ValidEntries(self)


class _ValidEntries:
    """What `FeatureTableView.valid_batches()` returns: called, it iterates one entry per batch; `block()` hands all of them over as one tensor."""

    def __init__(self, view: FeatureTableView) -> None:
        self.view = view
        self._rows = None

    def __call__(self):
        return self.view._valid()

    def block(self):
        t = self.view.table
        if t.device.type != "cuda":
            raise RuntimeError("a feature table's batches are gathered on the GPU (no CPU fallback)")
        if self._rows is None:
            self._rows = self.view._entries_t.to(t.device)          # uploaded once
        return t.feats.index_select(0, self._rows), t._targets_dev.index_select(0, self._rows)


__all__ = ["ResidentCohort", "CohortView", "plan_indices", "MAX_ROWS", "SAMPLERS", "ResidentFeatureTable", "FeatureTableView", "feature_table_labels",
           "parse_survival_status", "read_feature_vector"]
