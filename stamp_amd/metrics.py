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

The survival and regression reports -- a third kernel family (`amds_survival_groups`, `amds_regression_moments`, csrc/survival_stats.hip): risk sets
along the TIME order, split into two groups at a cut-off.  include/amdstamp.h states both statistics once.

* `survival_groups` -- the raw call: per problem the group counts, the log-rank sums O, E, V, the comparable pairs, the medians, and both groups'
  Kaplan-Meier curves and at-risk tables on a grid of times.
* `logrank_test`, `kaplan_meier`, `survival_stats` -- the reference's survival report (src/stamp/statistics/survival.py:37-87, 90-157) from tensors;
  lifelines is not a dependency: tests/survival_oracle.py restates the published algorithms over exact rationals.
* `bootstrap_survival` -- pointwise bands of the two curves and intervals of chi2 and the medians; all resamples in one library call.
* `regression_stats`, `bootstrap_regression`, `regression_moments` -- the reference's regression report (src/stamp/statistics/regression.py:14-39, 70).
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


# ---- survival report: log-rank test, Kaplan-Meier curves, at-risk table, medians (amds_survival_groups, csrc/survival_stats.hip) -----------------------
LOW, HIGH = 0, 1
ITEMS, DEATHS, CENSORED = range(3)


class SurvivalGroups(NamedTuple):
    """What `survival_groups` returns, per problem; group 0 = LOW (score <= cut-off), 1 = HIGH (include/amdstamp.h states every number).  counts int64
    [P, 2, 3] = (items, deaths, censored) per group; observed / expected / variance float64 [P]: the log-rank sums O, E, V of the HIGH group, NaN for a
    problem with an empty group; pairs int64 [P]: the reference's `comparable_pairs`; median float64 [P, 2] (+inf: never reached, NaN: empty group);
    km float64 [P, 2, G] and at_risk int64 [P, 2, G, 3] = (items with time >= x, deaths with time <= x, censored with time <= x) on grid_times, None
    without a grid; cut_off float64 [P]; grid_times float32 [G] or [P, G], or None."""
    counts: torch.Tensor
    observed: torch.Tensor
    expected: torch.Tensor
    variance: torch.Tensor
    pairs: torch.Tensor
    median: torch.Tensor
    km: torch.Tensor | None
    at_risk: torch.Tensor | None
    cut_off: torch.Tensor
    grid_times: torch.Tensor | None


class LogRank(NamedTuple):
    """What `logrank_test` returns, float64 [P]: chi2 = (O - E)^2 / V on one degree of freedom, p = erfc(sqrt(chi2 / 2)), and the three sums."""
    chi2: torch.Tensor
    p: torch.Tensor
    observed: torch.Tensor
    expected: torch.Tensor
    variance: torch.Tensor


class KaplanMeier(NamedTuple):
    """What `kaplan_meier` returns: x float32 [G] or [P, G]; km float64 [P, 2, G]; at_risk int64 [P, 2, G, 3]; median float64 [P, 2]; counts int64
    [P, 2, 3] -- group 0 = LOW, 1 = HIGH, as `SurvivalGroups`."""
    x: torch.Tensor
    km: torch.Tensor
    at_risk: torch.Tensor
    median: torch.Tensor
    counts: torch.Tensor


class BootstrapSurvival(NamedTuple):
    """What `bootstrap_survival` returns: x [G]; km [2, G] the sample's two curves; band_lower / band_upper [2, G] the per-point quantiles of the resamples'
    curves; chi2 and median [2] of the sample with the quantiles of the resamples' values; used = the resamples that entered; dropped_share = the share
    left out because a group was empty."""
    x: torch.Tensor
    km: torch.Tensor
    band_lower: torch.Tensor
    band_upper: torch.Tensor
    chi2: torch.Tensor
    chi2_lower: torch.Tensor
    chi2_upper: torch.Tensor
    median: torch.Tensor
    median_lower: torch.Tensor
    median_upper: torch.Tensor
    used: int
    dropped_share: float


def _index_rows(idx: torch.Tensor) -> torch.Tensor:
    if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1 or idx.dtype.is_floating_point:
        raise ValueError(f"idx must be an integer tensor [R, m], got {tuple(idx.shape)} {idx.dtype}")
    ix = idx.detach()
    if ix.dtype != torch.int32:
        ix = ix.clamp(-1, 1 << 30).to(torch.int32)          # (n <= 2^20: a value clamped here is out of range before and after)
    return ix.contiguous()


def _median_cut_off(s: torch.Tensor, t32: torch.Tensor, ev8: torch.Tensor) -> torch.Tensor:
    """numpy's `nanmedian` of the valid items' scores in float64 (the midpoint for an even count; NaN without a valid item) -> [P]; no host
    synchronisation."""
    valid = ~(s.isnan() | t32.isnan()) & (ev8 <= 1)
    v = torch.where(valid, s.double(), torch.full((), float("nan"), dtype=torch.float64, device=s.device))
    v = v.reshape(-1, v.shape[-1]) if v.dim() == 2 else v[None]
    srt = torch.sort(v, dim=1).values                        # NaN last
    k = valid.reshape(v.shape).sum(1)
    lo, hi = ((k - 1) // 2).clamp(min=0), (k // 2).clamp(max=v.shape[1] - 1)
    mid = (srt.gather(1, lo[:, None]) + srt.gather(1, hi[:, None]))[:, 0] * 0.5
    return torch.where(k > 0, mid, torch.full_like(mid, float("nan")))


def survival_groups(score: torch.Tensor, time: torch.Tensor, event: torch.Tensor, *, cut_off=None, grid_times: torch.Tensor | None = None,
                    idx: torch.Tensor | None = None) -> SurvivalGroups:
    """The raw call (include/amdstamp.h states the statistic).  score [n] or [P, n] (any non-negative strides), time / event [n] (shared) or [P, n], as
    `concordance_counts`; an item with a NaN score or time or an invalid event takes part in nothing.  cut_off: a number, a tensor [P] or 0-dim, or None =
    numpy's `nanmedian` of each problem's valid scores in float64, computed on the device (the reference's `np.nanmedian(risk)`, survival.py:63); an item
    is HIGH when float64(score) > cut_off.  grid_times: float [G] (shared) or [P, G], 2 <= G <= 4096, or None for no grid.  idx int [R, m]: problem r is
    the multiset of items idx[r] of the ONE problem (score, time, event all [n]; the default cut-off is the WHOLE sample's median); an index outside
    [0, n) raises.  No host synchronisation without idx."""
    ops._dev(score, time, event, idx, grid_times)
    dev = score.device
    if score.dim() not in (1, 2) or score.shape[-1] < 1 or score.shape[0] < 1:
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
    if cut_off is None:
        cut = _median_cut_off(s, t32.reshape(-1, n)[0] if t_prob == 0 else t32, ev8.reshape(-1, n)[0] if e_prob == 0 else ev8)
    else:
        cut = torch.as_tensor(cut_off, dtype=torch.float64, device=dev).detach().reshape(-1)
        if cut.numel() not in (1, P) and idx is None:
            raise ValueError(f"cut_off must be a number or hold one value per problem ({P}), got {cut.numel()}")
    lib = _lib.lib()
    if idx is not None:
        if P != 1 or score.dim() != 1 or t32.dim() != 1 or ev8.dim() != 1:
            raise ValueError("idx resamples ONE problem: score, time and event must be [n]")
        ix = _index_rows(idx)
        P, m, n_base = int(ix.shape[0]), int(ix.shape[1]), n
        if cut.numel() not in (1, P):
            raise ValueError(f"cut_off must be a number or hold one value per problem ({P}), got {cut.numel()}")
    else:
        ix, m, n_base = None, n, 0
    cut = cut.contiguous()
    c_prob = 1 if cut.numel() == P and P > 1 else 0
    G, g32, g_prob = 0, None, 0
    if grid_times is not None:
        if grid_times.dim() not in (1, 2) or (grid_times.dim() == 2 and grid_times.shape[0] not in (1, P)):
            raise ValueError(f"grid_times must be [G] or [{P}, G], got {tuple(grid_times.shape)}")
        g32 = grid_times.detach().to(dev, torch.float32).contiguous()
        G = int(g32.shape[-1])
        g_prob = G if g32.dim() == 2 and g32.shape[0] == P and P > 1 else 0
    nbytes = lib.amds_survival_groups_workspace_bytes(n_base, m, P, G, int(g_prob == 0))
    if nbytes == 0:
        raise ValueError("survival_groups: " + lib.amds_last_error().decode("utf-8", "replace"))
    ws = ops.scratch("survival_stats", dev, nbytes)
    counts = torch.empty(P, 2, 3, dtype=torch.int64, device=dev)
    logrank = torch.empty(P, 3, dtype=torch.float64, device=dev)
    median = torch.empty(P, 2, dtype=torch.float64, device=dev)
    pairs = torch.empty(P, dtype=torch.int64, device=dev)
    km = torch.empty(P, 2, G, dtype=torch.float64, device=dev) if G else None
    table = torch.empty(P, 2, G, 3, dtype=torch.int64, device=dev) if G else None
    _lib.check(lib.amds_survival_groups(s.data_ptr(), s_item, s_prob, t32.data_ptr(), t_prob, ev8.data_ptr(), e_prob, cut.data_ptr(), c_prob, ops._p(ix), n_base,
                                        m, P, ops._p(g32), g_prob, G, counts.data_ptr(), logrank.data_ptr(), median.data_ptr(), pairs.data_ptr(), ops._p(km),
                                        ops._p(table), ws.data_ptr(), ws.numel(), ops._stream()), "survival_groups")
    return SurvivalGroups(counts, logrank[:, 0], logrank[:, 1], logrank[:, 2], pairs, median, km, table, cut.expand(P) if cut.numel() == 1 else cut, g32)


def _chi2_p(observed: torch.Tensor, expected: torch.Tensor, variance: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """chi2 = (O - E)^2 / V and p = erfc(sqrt(chi2 / 2)) = scipy's `chi2.sf(chi2, 1)`, float64; V == 0 with both groups present (no death, or no risk
    set that holds both groups) -> chi2 0, p 1; an empty group (NaN sums) -> NaN."""
    diff = observed - expected
    chi2 = torch.where(variance > 0, diff * diff / variance.clamp(min=torch.finfo(torch.float64).tiny), torch.zeros_like(variance))
    chi2 = torch.where(variance.isnan(), variance, chi2)
    return chi2, torch.special.erfc(torch.sqrt(chi2 * 0.5))


def logrank_test(score: torch.Tensor, time: torch.Tensor, event: torch.Tensor, *, cut_off=None, idx: torch.Tensor | None = None) -> LogRank:
    """The two-sample log-rank test between the groups score <= cut_off and score > cut_off (`lifelines.statistics.logrank_test`, reference
    src/stamp/statistics/survival.py:63-75) -> float64 [P] tensors on the device.  chi2 and p are formed from the library's O, E and V by torch ops in
    float64.  An empty group -> NaN, as the reference; V == 0 with both groups present -> chi2 0, p 1.  Arguments as `survival_groups`."""
    g = survival_groups(score, time, event, cut_off=cut_off, idx=idx)
    chi2, p = _chi2_p(g.observed, g.expected, g.variance)
    return LogRank(chi2, p, g.observed, g.expected, g.variance)


def _default_grid(time: torch.Tensor, valid: torch.Tensor, points: int) -> torch.Tensor:
    """`points` times from 0 to the largest valid time, float32 [..., points] (NaN without a valid item)."""
    tmax = torch.where(valid, time.double(), torch.full((), float("-inf"), dtype=torch.float64, device=time.device)).amax(dim=-1, keepdim=True)
    tmax = torch.where(tmax.isinf(), torch.full_like(tmax, float("nan")), tmax)
    return (torch.arange(points, dtype=torch.float64, device=time.device) / (points - 1) * tmax).float()


def kaplan_meier(score: torch.Tensor, time: torch.Tensor, event: torch.Tensor, *, cut_off=None, grid_times: torch.Tensor | None = None,
                 idx: torch.Tensor | None = None, points: int = 256) -> KaplanMeier:
    """The Kaplan-Meier curves of the two risk groups (`KaplanMeierFitter`, reference src/stamp/statistics/survival.py:116-137), the table under the plot
    and the median survival times, on grid_times; default: `points` = 256 times from 0 to the largest valid time (of the one problem; with [P, n] inputs a
    grid per problem).  The table is the library's own definition (include/amdstamp.h), not lifelines' `add_at_risk_counts`."""
    if grid_times is None:
        ops._dev(score, time, event)
        s, t, e = torch.broadcast_tensors(score.detach().float(), time.detach().to(score.device).float(), _event_bytes(event.detach().to(score.device)))
        grid_times = _default_grid(t, ~(s.isnan() | t.isnan()) & (e <= 1), int(points))
    g = survival_groups(score, time, event, cut_off=cut_off, grid_times=grid_times, idx=idx)
    return KaplanMeier(g.grid_times, g.km, g.at_risk, g.median, g.counts)


def survival_stats(score: torch.Tensor, time: torch.Tensor, event: torch.Tensor, *, cut_off=None) -> dict[str, torch.Tensor]:
    """The row of the reference's survival table (src/stamp/statistics/survival.py:77-87) -> a dict of 0-dim tensors on the device: `c_index`
    (`concordance_index`), `logrank_p`, `count`, `events`, `censored` (int64, over the valid items), `comparable_pairs` (int64) and `threshold` (the
    cut-off used, float64).  `comparable_pairs` is the reference's own count #{(i, j): time_i < time_j, event_i == 1}; it is NOT the permissible count of
    `concordance_counts`, which also holds the (death, censored) pairs at one time, so the survival kernel counts it."""
    s, t, e = score.reshape(-1), time.reshape(-1), event.reshape(-1)
    g = survival_groups(s, t, e, cut_off=cut_off)
    tot = g.counts[0].sum(0)
    return {"c_index": concordance_index(s, t, e), "logrank_p": _chi2_p(g.observed, g.expected, g.variance)[1][0], "count": tot[ITEMS], "events": tot[DEATHS],
            "censored": tot[CENSORED], "comparable_pairs": g.pairs[0], "threshold": g.cut_off[0]}


def _draw(n: int, n_resamples: int, generator: torch.Generator | None, dev: torch.device) -> torch.Tensor:
    gdev = generator.device if generator is not None else dev
    return torch.randint(0, n, (int(n_resamples), n), generator=generator, device=gdev, dtype=torch.int32).to(dev)


def bootstrap_survival(score: torch.Tensor, time: torch.Tensor, event: torch.Tensor, *, cut_off=None, grid_times: torch.Tensor | None = None,
                       idx: torch.Tensor | None = None, n_resamples: int = 1000, generator: torch.Generator | None = None,
                       quantiles: tuple[float, float] = (0.025, 0.975), points: int = 256) -> BootstrapSurvival:
    """Pointwise bands of the two Kaplan-Meier curves and intervals of the log-rank chi2 and of the two medians over resamples with replacement -- the
    resampling `bootstrap_ci` and `bootstrap_curve` offer, for the survival report.  Every resample is split at the FULL sample's cut-off, and all of them
    run in ONE `amds_survival_groups` call.  A resample with an empty group is left out; dropped_share reports their share.  Bands and the chi2 interval
    interpolate linearly, as `np.quantile`; the medians' interval takes the order statistics below the lower and above the upper quantile
    (`method="lower"` / `"higher"`), because a median may be +inf.  idx [R, m]: the resamples' index lists (default: `n_resamples` draws of n from
    torch.randint with `generator`).  None used -> NaN bounds and bands."""
    ops._dev(score, time, event, idx)
    s, t, e = score.reshape(-1), time.reshape(-1), event.reshape(-1)
    if grid_times is None:
        t32, e8 = t.detach().to(s.device).float(), _event_bytes(e.detach().to(s.device))
        grid_times = _default_grid(t32, ~(s.detach().float().isnan() | t32.isnan()) & (e8 <= 1), int(points))
    full = survival_groups(s, t, e, cut_off=cut_off, grid_times=grid_times.reshape(-1))
    chi2 = _chi2_p(full.observed, full.expected, full.variance)[0][0]
    if idx is None:
        idx = _draw(int(s.shape[0]), n_resamples, generator, s.device)
    res = survival_groups(s, t, e, cut_off=full.cut_off[:1], grid_times=full.grid_times, idx=idx)
    keep = ~res.observed.isnan()
    used = int(keep.sum())
    total = int(keep.numel())
    x, point, med = full.grid_times, full.km[0], full.median[0]
    if used == 0:
        nans, nan, nan2 = torch.full_like(point, float("nan")), torch.full_like(chi2, float("nan")), torch.full_like(med, float("nan"))
        return BootstrapSurvival(x, point, nans, nans.clone(), chi2, nan, nan.clone(), med, nan2, nan2.clone(), 0, 1.0)
    q = torch.tensor(list(quantiles), dtype=torch.float64, device=s.device)
    rows = res.km[keep].reshape(used, -1)
    band = _column_quantiles(rows, q).reshape(2, 2, -1)
    c_lo, c_hi = torch.quantile(_chi2_p(res.observed[keep], res.expected[keep], res.variance[keep])[0], q, interpolation="linear")
    meds = res.median[keep]
    m_lo = torch.quantile(meds, q[0], dim=0, interpolation="lower")
    m_hi = torch.quantile(meds, q[1], dim=0, interpolation="higher")
    return BootstrapSurvival(x, point, band[0], band[1], chi2, c_lo, c_hi, med, m_lo, m_hi, used, 1.0 - used / total)


# ---- regression report: R^2, Pearson r, MAE, RMSE, the fitted line (amds_regression_moments, csrc/survival_stats.hip) ----------------------------------
N, MEAN_T, MEAN_P, SXX, SYY, SXY, SAE, SSE = range(8)
REGRESSION_KEYS = ("r2_score", "pearson_r", "mae", "rmse", "count", "slope", "intercept", "stderr")


def regression_moments(pred: torch.Tensor, truth: torch.Tensor, *, idx: torch.Tensor | None = None) -> torch.Tensor:
    """The raw call -> float64 [P, 8] = (n, mean_t, mean_p, Sxx, Syy, Sxy, sum |p - t|, sum (p - t)^2) over the items without a NaN, the S terms centred
    on the problem's own means (include/amdstamp.h).  pred / truth [n] or [P, n] (any positive item stride, non-negative problem stride; a 1-D one is
    shared by the problems of the other).  idx int [R, m]: problem r is the multiset idx[r] of the ONE problem; an index outside [0, n) raises."""
    ops._dev(pred, truth, idx)
    dev = pred.device
    if pred.dim() not in (1, 2) or truth.dim() not in (1, 2) or pred.shape[-1] != truth.shape[-1] or pred.shape[-1] < 1:
        raise ValueError(f"pred and truth must be [n] or [P, n] with the same n >= 1, got {tuple(pred.shape)} and {tuple(truth.shape)}")
    n = int(pred.shape[-1])
    Ps = {int(a.shape[0]) for a in (pred, truth) if a.dim() == 2}
    if len(Ps) > 1 or 0 in Ps:
        raise ValueError(f"pred and truth must hold the same number of problems, got {tuple(pred.shape)} and {tuple(truth.shape)}")
    P = Ps.pop() if Ps else 1

    def arg(a: torch.Tensor) -> tuple[torch.Tensor, int, int]:
        a = a.detach().to(dev)
        if a.dtype != torch.float32:
            a = a.float()
        if n > 1 and a.stride(-1) < 1:
            a = a.contiguous()
        return a, max(int(a.stride(-1)), 1), (int(a.stride(0)) if a.dim() == 2 and P > 1 else 0)

    (p32, p_item, p_prob), (t32, t_item, t_prob) = arg(pred), arg(truth)
    lib = _lib.lib()
    if idx is not None:
        if pred.dim() != 1 or truth.dim() != 1:
            raise ValueError("idx resamples ONE problem: pred and truth must be [n]")
        ix = _index_rows(idx)
        P, m, n_base = int(ix.shape[0]), int(ix.shape[1]), n
    else:
        ix, m, n_base = None, n, 0
    nbytes = lib.amds_regression_moments_workspace_bytes(n_base, m, P)
    if nbytes == 0:
        raise ValueError("regression_moments: " + lib.amds_last_error().decode("utf-8", "replace"))
    ws = ops.scratch("regression_stats", dev, nbytes)
    out = torch.empty(P, 8, dtype=torch.float64, device=dev)
    _lib.check(lib.amds_regression_moments(t32.data_ptr(), t_item, t_prob, p32.data_ptr(), p_item, p_prob, ops._p(ix), n_base, m, P, out.data_ptr(), ws.data_ptr(),
                                           ws.numel(), ops._stream()), "regression_moments")
    return out


def regression_from_moments(m: torch.Tensor) -> dict[str, torch.Tensor]:
    """[..., 8] moments -> the numbers of `regression_stats`, float64 [...] (count int64).  Plain torch ops; works on any device."""
    nan = torch.full_like(m[..., N], float("nan"))
    n, sxx, syy, sxy, sse = m[..., N], m[..., SXX], m[..., SYY], m[..., SXY], m[..., SSE]
    n1 = n.clamp(min=1.0)
    r2 = torch.where(sxx > 0, 1.0 - sse / sxx.clamp(min=torch.finfo(torch.float64).tiny), torch.where(sse == 0, torch.ones_like(n), torch.zeros_like(n)))
    r2 = torch.where(n >= 2, r2, nan)
    den = torch.sqrt(sxx) * torch.sqrt(syy)
    r_any = (sxy / den.clamp(min=torch.finfo(torch.float64).tiny)).clamp(-1.0, 1.0)
    pearson = torch.where((sxx > 0) & (syy > 0), r_any, nan)
    line = (sxx > 0) & (n >= 2)
    slope = torch.where(line, sxy / sxx.clamp(min=torch.finfo(torch.float64).tiny), nan)
    r_line = torch.where(den > 0, r_any, torch.zeros_like(n))
    err = torch.sqrt((1.0 - r_line * r_line).clamp(min=0.0) * syy / sxx.clamp(min=torch.finfo(torch.float64).tiny) / (n - 2.0).clamp(min=1.0))
    stderr = torch.where(line, torch.where(n > 2, err, torch.zeros_like(n)), nan)
    return {"r2_score": r2, "pearson_r": pearson, "mae": torch.where(n > 0, m[..., SAE] / n1, nan), "rmse": torch.where(n > 0, torch.sqrt(sse / n1), nan),
            "count": n.long(), "slope": slope, "intercept": m[..., MEAN_P] - slope * m[..., MEAN_T], "stderr": stderr}


def regression_stats(pred: torch.Tensor, truth: torch.Tensor) -> dict[str, torch.Tensor]:
    """The row of the reference's regression table (src/stamp/statistics/regression.py:14-39) and the line of its scatter plot (:70) -> a dict of 0-dim
    tensors on the device: `r2_score`, `mean_absolute_error` as `mae`, the root of `mean_squared_error` as `rmse` (sklearn's definitions), `pearson_r`
    (NaN when either column is constant, as the reference), `count` (int64, the rows without a NaN), and `slope`, `intercept`, `stderr` of
    `scipy.stats.linregress(truth, pred)` (stderr 0 for two rows; NaN where scipy raises: fewer than two rows or a constant truth).  `r2_score` follows
    sklearn: NaN for fewer than two rows; for a constant truth 1 when every prediction is exact, else 0.  `pearson_p` is left out: it is the tail of
    Student's t distribution, which neither torch nor this library has -- as `p_value` in `categorical_stats`."""
    return {k: v[0] for k, v in regression_from_moments(regression_moments(pred.reshape(-1), truth.reshape(-1))).items()}


def bootstrap_regression(pred: torch.Tensor, truth: torch.Tensor, *, idx: torch.Tensor | None = None, n_resamples: int = 1000,
                         generator: torch.Generator | None = None, quantiles: tuple[float, float] = (0.025, 0.975)) -> dict[str, tuple]:
    """-> {name: (value of the sample, lower, upper)} for every number of `regression_stats` but `count`: the two quantiles over resamples with replacement
    (linear, as `np.quantile`; resamples where the number is NaN -- a constant column -- are left out of that number's interval; none left -> NaN).  All
    resamples are ONE `amds_regression_moments` call.  idx [R, m]: the resamples' index lists (default: `n_resamples` draws of n from torch.randint with
    `generator`)."""
    ops._dev(pred, truth, idx)
    p, t = pred.reshape(-1), truth.reshape(-1)
    if idx is None:
        idx = _draw(int(p.shape[0]), n_resamples, generator, p.device)
    point = regression_from_moments(regression_moments(p, t))
    res = regression_from_moments(regression_moments(p, t, idx=idx))
    q = torch.tensor(list(quantiles), dtype=torch.float64, device=p.device)
    out = {}
    for k in REGRESSION_KEYS:
        if k == "count":
            continue
        lo, hi = torch.nanquantile(res[k], q, interpolation="linear")
        out[k] = (point[k][0], lo, hi)
    return out
