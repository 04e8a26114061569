"""Rank metrics on the GPU: the concordance index the reference selects survival epochs on, the one-vs-rest AUROC it logs for classifiers, and
bootstrap intervals of both -- one exact pair-count kernel (`amds_concordance_counts`, csrc/rank_metrics.hip).  Tensors only, GPU only, no CPU fallback.

The statistic (include/amdstamp.h states it once): items i have a risk score_i (higher = worse), a time_i and an event_i in {0, 1}; the ordered pair
(i, j) is permissible when event_i == 1 and (time_i < time_j or (time_i == time_j and event_j == 0)), concordant when score_i > score_j, tied when
score_i == score_j; C = (concordant + tied / 2) / permissible.

* `concordance_index` -- `LitSurvivalBase.c_index` (reference src/stamp/modeling/models/__init__.py:662-694): lifelines.utils.concordance_index(time,
  -score, event).  lifelines sweeps the subjects by exit time; deaths at a time are ranked against EARLIER deaths only and then inserted, subjects censored
  at that time are ranked after the insertion and never inserted, so two deaths at one time are not comparable -- the definition above.  lifelines is not a
  dependency of this package: tests/test_cpu_rank_metrics.py pins the definition against an independent restatement of that sweep, not against lifelines.
* `multiclass_auroc` -- score = p[:, c], event = (y == c), time = (y != c): the permissible pairs are exactly the (positive, negative) pairs and C is
  `sklearn.metrics.roc_auc_score(y == c, p[:, c])` (src/stamp/statistics/categorical.py:65-68; logged per run, models/__init__.py:217, 270-277).  A class
  without a positive or without a negative is NaN and left out of the mean; what torchmetrics' MulticlassAUROC does in that case is NOT reproduced.
* `bootstrap_ci` -- the reference's intervals are quantiles over 1000 resamples with replacement (src/stamp/statistics/roc.py:161-214); all resamples
  are problems of ONE library call (an index list per resample; nothing is gathered on the host).

Curve statistics, the other half of the reference's classifier report -- a second kernel family (`amds_binary_curves`, csrc/curve_stats.hip), because
precision is a ratio per threshold and a curve needs cumulative counts along the score order: neither is a pair count.  include/amdstamp.h states the
statistic once (curve points, AP, the two areas, the two grids and their knife-edge rule); the functions below only shape tensors for it.

* `binary_curves` -- the raw call: per problem the class counts, AP, the PR area, the gridded PR area, and the ROC and PR curves on a grid.
* `average_precision`, `multiclass_auprc` -- `sklearn.metrics.average_precision_score`, ties included (src/stamp/statistics/categorical.py:71-75); a
  problem without a positive or without a negative is NaN, where sklearn returns a number with a warning.
* `categorical_stats` -- count, roc_auc_score, average_precision_score, f1_score per class (categorical.py:60-81; `p_value` is left out).
* `bootstrap_curve` -- the bands and area intervals of the reference's bootstrapped ROC and precision-recall plots (src/stamp/statistics/roc.py:161-224,
  src/stamp/statistics/prc.py:26-87): all resamples' curves in one library call.  Against sklearn + `np.interp` the grid values agree to 1e-9 except at
  knife edges (a grid point that coincides with a curve point as a rational, about 3e-5 of the points measured), which the library decides in integers.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib, ops

CONCORDANT, TIED, PERMISSIBLE, VALID = range(4)


def _event_bytes(event: torch.Tensor) -> torch.Tensor:
    """-> u8 with 0 / 1 kept and every other value (NaN included) turned into 255, the library's mark of an invalid item."""
    if event.dtype in (torch.bool, torch.uint8):
        return event.to(torch.uint8)
    one = event == 1
    return torch.where(one | (event == 0), one.to(torch.uint8), torch.full((), 255, dtype=torch.uint8, device=event.device))


def concordance_counts(score: torch.Tensor, time: torch.Tensor, event: torch.Tensor, idx: torch.Tensor | None = None) -> torch.Tensor:
    """Exact pair counts -> int64 [P, 4] = (concordant, tied, permissible, valid items) per problem.

    score [n] or [P, n] (any non-negative strides: `probs.t()` of a row-major [n, C] matrix is C problems without a copy); time / event [n] (shared by the
    problems) or [P, n].  event: bool, or numbers of which 0 and 1 are valid.  An item with a NaN score or time or an invalid event takes part in no pair.
    idx int [R, m]: problem r is the multiset of items idx[r] of the ONE problem (score, time, event all [n]); an index outside [0, n) raises.
    No host synchronisation without idx."""
    ops._dev(score, time, event, idx)
    dev = score.device
    if score.dim() not in (1, 2) or score.shape[-1] < 1:
        raise ValueError(f"score must be [n] or [P, n] with n >= 1, got {tuple(score.shape)}")
    n = int(score.shape[-1])
    P = int(score.shape[0]) if score.dim() == 2 else 1
    s = score.detach()
    if s.dtype != torch.float32:
        s = s.float()
    if n > 1 and s.stride(-1) == 0:
        s = s.contiguous()
    s_item, s_prob = max(int(s.stride(-1)), 1), int(s.stride(0)) if s.dim() == 2 else 0

    def rows(t: torch.Tensor, what: str, conv) -> tuple[torch.Tensor, int]:
        if t.shape[-1] != n or t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] not in (1, P)):
            raise ValueError(f"{what} must be [{n}] or [{P}, {n}], got {tuple(t.shape)}")
        t = conv(t.detach()).contiguous()
        return t, (n if t.dim() == 2 and t.shape[0] == P and P > 1 else 0)

    t32, t_prob = rows(time, "time", lambda t: t.to(dev, torch.float32))
    ev8, e_prob = rows(event, "event", lambda t: _event_bytes(t.to(dev)))
    lib = _lib.lib()
    if idx is not None:
        if P != 1 or score.dim() != 1 or t32.dim() != 1 or ev8.dim() != 1:
            raise ValueError("idx resamples ONE problem: score, time and event must be [n]")
        if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1 or idx.dtype.is_floating_point:
            raise ValueError(f"idx must be an integer tensor [R, m], got {tuple(idx.shape)} {idx.dtype}")
        ix = idx.detach()
        if ix.dtype != torch.int32:
            ix = ix.clamp(-1, 1 << 30).to(torch.int32)          # (n < 2^31: a value clamped here is out of range before and after)
        ix = ix.contiguous()
        P, m = int(ix.shape[0]), int(ix.shape[1])
    else:
        ix, m = None, n
    nbytes = lib.amds_concordance_workspace_bytes(m, P)
    if nbytes == 0:
        raise ValueError(f"concordance_counts: unsupported shape n={m} problems={P}")
    ws = ops.scratch("rank_metrics", dev, nbytes)
    out = torch.empty(P, 4, dtype=torch.int64, device=dev)
    _lib.check(lib.amds_concordance_counts(s.data_ptr(), s_item, s_prob, t32.data_ptr(), t_prob, ev8.data_ptr(), e_prob, ops._p(ix), n, m, P, out.data_ptr(),
                                           ws.data_ptr(), ws.numel(), ops._stream()), "concordance_counts")
    return out


def _c_of(counts: torch.Tensor) -> torch.Tensor:
    """[..., 4] counts -> C in float64, NaN where no pair is permissible."""
    c = counts.double()
    perm = c[..., PERMISSIBLE]
    return torch.where(perm > 0, (c[..., CONCORDANT] + 0.5 * c[..., TIED]) / perm.clamp(min=1.0), torch.full_like(perm, float("nan")))


def concordance_index(scores: torch.Tensor, times: torch.Tensor, events: torch.Tensor) -> torch.Tensor:
    """The reference's `c_index` (models/__init__.py:662-694) -> a 0-dim tensor on the scores' device, of the scores' dtype.  Rows with a NaN in any of the
    three are dropped; at most one valid row -> NaN; no permissible pair -> NaN (lifelines raises there, the reference catches it and returns NaN)."""
    counts = concordance_counts(scores.reshape(-1), times.reshape(-1), events.reshape(-1))[0]
    c = torch.where(counts[VALID] > 1, _c_of(counts), torch.full((), float("nan"), dtype=torch.float64, device=counts.device))
    return c.to(scores.dtype if scores.dtype.is_floating_point else torch.float32)


def _nan_mean(per: torch.Tensor) -> torch.Tensor:
    ok = ~per.isnan()
    return torch.where(ok.any(), torch.where(ok, per, torch.zeros_like(per)).sum() / ok.sum().clamp(min=1), torch.full_like(per[0], float("nan")))


def _one_vs_rest(probs: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    ops._dev(probs, target)
    if probs.dim() != 2 or target.dim() != 1 or target.shape[0] != probs.shape[0] or probs.shape[0] < 1:
        raise ValueError(f"probs must be [n, C] and target [n], got {tuple(probs.shape)} and {tuple(target.shape)}")
    return target.to(probs.device).long()[None, :] == torch.arange(probs.shape[1], device=probs.device)[:, None]          # [C, n]


def multiclass_auroc(probs: torch.Tensor, target: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """probs [n, C], target [n] class indices -> (one-vs-rest AUROC per class, float64 [C]; their mean over the classes that have both a positive and a
    negative).  A class without one is NaN and left out of the mean (all classes so: the mean is NaN)."""
    pos = _one_vs_rest(probs, target)
    per = _c_of(concordance_counts(probs.detach().float().contiguous().t(), (~pos).float(), pos))
    return per, _nan_mean(per)


def bootstrap_ci(score: torch.Tensor, time: torch.Tensor, event: torch.Tensor, *, idx: torch.Tensor | None = None, n_resamples: int = 1000,
                 generator: torch.Generator | None = None, quantiles: tuple[float, float] = (0.025, 0.975)):
    """-> (point value, lower, upper, resamples used): C of the sample and the two quantiles of C over resamples with replacement.  idx [R, m]: the
    resamples' index lists (default: `n_resamples` draws of n from torch.randint with `generator`).  Resamples without a permissible pair are skipped (the
    reference's ``len(np.unique(...)) != 2: continue``, roc.py:192-193); quantiles interpolate linearly, as `np.quantile` does.  All resamples run in one
    library call.  The three values are 0-dim float64 tensors on the device; none used -> NaN bounds."""
    ops._dev(score, time, event, idx)
    s, t, e = score.reshape(-1), time.reshape(-1), event.reshape(-1)
    n = s.shape[0]
    if idx is None:
        gdev = generator.device if generator is not None else s.device
        idx = torch.randint(0, n, (int(n_resamples), n), generator=generator, device=gdev, dtype=torch.int32).to(s.device)
    point = _c_of(concordance_counts(s, t, e)[0])
    vals = _c_of(concordance_counts(s, t, e, idx=idx))
    vals = vals[~vals.isnan()]
    used = int(vals.numel())
    if used == 0:
        nan = torch.full_like(point, float("nan"))
        return point, nan, nan.clone(), 0
    lo, hi = torch.quantile(vals, torch.tensor(list(quantiles), dtype=torch.float64, device=vals.device), interpolation="linear")
    return point, lo, hi, used


# ---- curve statistics: average precision, ROC and precision-recall curves on a grid (amds_binary_curves, csrc/curve_stats.hip) -------------------------
class BinaryCurves(NamedTuple):
    """What `binary_curves` returns, per problem.  counts int64 [P, 2] = (positives, negatives) among the valid items; the rest float64, NaN for a problem
    without a positive or without a negative: ap, pr_area (the problem's own curve), pr_area_grid (the trapezoid of the PR grid; NaN when grid == 0), and
    roc / pr [P, grid] (None when not asked for)."""
    counts: torch.Tensor
    ap: torch.Tensor
    pr_area: torch.Tensor
    pr_area_grid: torch.Tensor
    roc: torch.Tensor | None
    pr: torch.Tensor | None


class BootstrapCurve(NamedTuple):
    """What `bootstrap_curve` returns: the point value of the area and the two quantiles of the resamples' areas (0-dim float64), the grid x [grid] and the
    per-column quantiles of the resamples' curves [grid], and the number of resamples that entered them."""
    value: torch.Tensor
    lower: torch.Tensor
    upper: torch.Tensor
    x: torch.Tensor
    band_lower: torch.Tensor
    band_upper: torch.Tensor
    used: int


def binary_curves(score: torch.Tensor, positive: torch.Tensor, *, idx: torch.Tensor | None = None, grid: int = 1000, roc: bool = True,
                  pr: bool = True) -> BinaryCurves:
    """The raw call (include/amdstamp.h states the statistic).  score [n] or [P, n] (any non-negative strides: `probs.t()` of a row-major [n, C] matrix is
    C problems without a copy); positive [n] (shared) or [P, n]: bool, or numbers of which 1 (positive) and 0 (negative) are valid.  An item with a NaN
    score or an invalid label takes part in nothing.  idx int [R, m]: problem r is the multiset of items idx[r] of the ONE problem (score, positive both
    [n]); an index outside [0, n) raises.  grid: points of the two grids, 0 or 2..4096; 0 needs roc = pr = False.  No host synchronisation without idx."""
    ops._dev(score, positive, idx)
    dev = score.device
    if score.dim() not in (1, 2) or score.shape[-1] < 1:
        raise ValueError(f"score must be [n] or [P, n] with n >= 1, got {tuple(score.shape)}")
    n = int(score.shape[-1])
    P = int(score.shape[0]) if score.dim() == 2 else 1
    if P < 1:
        raise ValueError(f"score must hold at least one problem, got {tuple(score.shape)}")
    grid = int(grid)
    if grid == 0 and (roc or pr):
        raise ValueError("grid=0 computes no grid: pass roc=False, pr=False")
    s = score.detach()
    if s.dtype != torch.float32:
        s = s.float()
    if n > 1 and s.stride(-1) == 0:
        s = s.contiguous()
    s_item, s_prob = max(int(s.stride(-1)), 1), int(s.stride(0)) if s.dim() == 2 else 0
    if positive.shape[-1] != n or positive.dim() not in (1, 2) or (positive.dim() == 2 and positive.shape[0] not in (1, P)):
        raise ValueError(f"positive must be [{n}] or [{P}, {n}], got {tuple(positive.shape)}")
    lab = _event_bytes(positive.detach().to(dev)).contiguous()
    l_prob = n if lab.dim() == 2 and lab.shape[0] == P and P > 1 else 0
    lib = _lib.lib()
    if idx is not None:
        if P != 1 or score.dim() != 1 or lab.dim() != 1:
            raise ValueError("idx resamples ONE problem: score and positive must be [n]")
        if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1 or idx.dtype.is_floating_point:
            raise ValueError(f"idx must be an integer tensor [R, m], got {tuple(idx.shape)} {idx.dtype}")
        ix = idx.detach()
        if ix.dtype != torch.int32:
            ix = ix.clamp(-1, 1 << 30).to(torch.int32)          # (n <= 2^20: a value clamped here is out of range before and after)
        ix = ix.contiguous()
        P, m, n_base = int(ix.shape[0]), int(ix.shape[1]), n
    else:
        ix, m, n_base = None, n, 0
    nbytes = lib.amds_binary_curves_workspace_bytes(n_base, m, P, grid)
    if nbytes == 0:
        raise ValueError("binary_curves: " + lib.amds_last_error().decode("utf-8", "replace"))
    ws = ops.scratch("curve_stats", dev, nbytes)
    counts = torch.empty(P, 2, dtype=torch.int64, device=dev)
    scalars = torch.empty(P, 3, dtype=torch.float64, device=dev)
    roc_t = torch.empty(P, grid, dtype=torch.float64, device=dev) if roc else None
    pr_t = torch.empty(P, grid, dtype=torch.float64, device=dev) if pr else None
    _lib.check(lib.amds_binary_curves(s.data_ptr(), s_item, s_prob, lab.data_ptr(), l_prob, ops._p(ix), n_base, m, P, grid, counts.data_ptr(),
                                      scalars.data_ptr(), ops._p(roc_t), ops._p(pr_t), ws.data_ptr(), ws.numel(), ops._stream()), "binary_curves")
    return BinaryCurves(counts, scalars[:, 0], scalars[:, 1], scalars[:, 2], roc_t, pr_t)


def average_precision(score: torch.Tensor, positive: torch.Tensor) -> torch.Tensor:
    """`sklearn.metrics.average_precision_score(positive, score)`, ties included -> a 0-dim float64 tensor on the device.  Without a positive or without a
    negative: NaN (sklearn warns and returns a number there; the reference's resampling loops skip such samples, prc.py:54)."""
    return binary_curves(score.reshape(-1), positive.reshape(-1), grid=0, roc=False, pr=False).ap[0]


def multiclass_auprc(probs: torch.Tensor, target: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """probs [n, C], target [n] class indices -> (one-vs-rest average precision per class, float64 [C]; their mean over the classes that have both a
    positive and a negative).  A class without one is NaN and left out of the mean (all classes so: the mean is NaN) -- the rule of `multiclass_auroc`."""
    pos = _one_vs_rest(probs, target)
    per = binary_curves(probs.detach().float().contiguous().t(), pos, grid=0, roc=False, pr=False).ap
    return per, _nan_mean(per)


def categorical_stats(probs: torch.Tensor, target: torch.Tensor) -> dict[str, torch.Tensor]:
    """The per-class columns of the reference's `*_categorical-stats_individual.csv` (src/stamp/statistics/categorical.py:60-81) -> a dict of [C] tensors on
    the device: `count` (int64, items of the class), `roc_auc_score`, `average_precision_score` and `f1_score` (float64) of the class against the rest,
    f1 on the arg-max labels (the first maximum wins, as numpy's argmax; 0 where the class is neither predicted nor present, as sklearn's zero_division).
    `p_value` is left out: it is Student's t distribution's tail (scipy.stats.ttest_ind), which neither torch nor this library has."""
    pos = _one_vs_rest(probs, target)
    p32 = probs.detach().float().contiguous()
    auroc = _c_of(concordance_counts(p32.t(), (~pos).float(), pos))
    ap = binary_curves(p32.t(), pos, grid=0, roc=False, pr=False).ap
    pred = p32.argmax(dim=1)[None, :] == torch.arange(p32.shape[1], device=p32.device)[:, None]
    tp, fp, fn = (pred & pos).sum(1).double(), (pred & ~pos).sum(1).double(), (~pred & pos).sum(1).double()
    den = 2 * tp + fp + fn
    f1 = torch.where(den > 0, 2 * tp / den.clamp(min=1.0), torch.zeros_like(den))
    return {"count": pos.sum(1), "roc_auc_score": auroc, "average_precision_score": ap, "f1_score": f1}


def _column_quantiles(rows: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """rows [R, G] -> [len(q), G], linear; in column blocks, because torch.quantile takes at most 2^24 elements."""
    step = max(1, (1 << 24) // max(int(rows.shape[0]), 1))
    return torch.cat([torch.quantile(rows[:, c:c + step], q, dim=0, interpolation="linear") for c in range(0, rows.shape[1], step)], dim=1)


def bootstrap_curve(score: torch.Tensor, positive: torch.Tensor, *, kind: str = "roc", idx: torch.Tensor | None = None, n_resamples: int = 1000,
                    generator: torch.Generator | None = None, quantiles: tuple[float, float] = (0.025, 0.975), grid: int = 1000) -> BootstrapCurve:
    """The numbers behind the reference's bootstrapped ROC (kind="roc", src/stamp/statistics/roc.py:161-224) and precision-recall (kind="pr",
    src/stamp/statistics/prc.py:26-87) plots.  Every resample's curve is interpolated onto x = linspace(0, 1, grid); band_lower / band_upper are the two
    quantiles per grid column over the resamples (linear, as `np.quantile`).  kind="roc": value = the AUROC of the sample (the pair counts of
    `concordance_counts`), lower / upper the quantiles of the resamples' AUROC.  kind="pr": value = the area under the sample's own precision-recall curve
    (`auc(recall, precision)`, prc.py:81-82), lower / upper the quantiles of the resamples' GRIDDED areas (prc.py:62), as the reference does.  idx [R, m]: the
    resamples' index lists (default: `n_resamples` draws of n from torch.randint with `generator`).  A resample without a positive or without a negative
    is dropped (roc.py:192, prc.py:54).  All resamples' curves run in ONE library call (the resamples' AUROC in one call of the pair kernel).  None used ->
    NaN bounds and bands."""
    if kind not in ("roc", "pr"):
        raise ValueError(f"kind must be 'roc' or 'pr', got {kind!r}")
    ops._dev(score, positive, idx)
    s, y = score.reshape(-1), positive.reshape(-1)
    n = s.shape[0]
    if idx is None:
        gdev = generator.device if generator is not None else s.device
        idx = torch.randint(0, n, (int(n_resamples), n), generator=generator, device=gdev, dtype=torch.int32).to(s.device)
    q = torch.tensor(list(quantiles), dtype=torch.float64, device=s.device)
    x = torch.arange(grid, dtype=torch.float64, device=s.device) / (grid - 1)
    res = binary_curves(s, y, idx=idx, grid=grid, roc=kind == "roc", pr=kind == "pr")
    if kind == "roc":
        pos = _event_bytes(y.to(s.device))
        time = (pos != 1).float()                              # (a label byte above 1 is an invalid event of the pair statistic too)
        point = _c_of(concordance_counts(s, time, pos)[0])
        vals, rows = _c_of(concordance_counts(s, time, pos, idx=idx)), res.roc
    else:
        point = binary_curves(s, y, grid=0, roc=False, pr=False).pr_area[0]
        vals, rows = res.pr_area_grid, res.pr
    keep = ~res.ap.isnan()
    vals, rows = vals[keep], rows[keep]
    used = int(vals.numel())
    if used == 0:
        nan, nans = torch.full_like(point, float("nan")), torch.full_like(x, float("nan"))
        return BootstrapCurve(point, nan, nan.clone(), x, nans, nans.clone(), 0)
    lo, hi = torch.quantile(vals, q, interpolation="linear")
    band = _column_quantiles(rows, q)
    return BootstrapCurve(point, lo, hi, x, band[0], band[1], used)
