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
"""
from __future__ import annotations

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


def multiclass_auroc(probs: torch.Tensor, target: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """probs [n, C], target [n] class indices -> (one-vs-rest AUROC per class, float64 [C]; their mean over the classes that have both a positive and a
    negative).  A class without one is NaN and left out of the mean (all classes so: the mean is NaN)."""
    ops._dev(probs, target)
    if probs.dim() != 2 or target.dim() != 1 or target.shape[0] != probs.shape[0] or probs.shape[0] < 1:
        raise ValueError(f"probs must be [n, C] and target [n], got {tuple(probs.shape)} and {tuple(target.shape)}")
    C = probs.shape[1]
    pos = target.to(probs.device).long()[None, :] == torch.arange(C, device=probs.device)[:, None]          # [C, n]
    per = _c_of(concordance_counts(probs.detach().float().contiguous().t(), (~pos).float(), pos))
    ok = ~per.isnan()
    mean = torch.where(ok.any(), torch.where(ok, per, torch.zeros_like(per)).sum() / ok.sum().clamp(min=1), torch.full_like(per[0], float("nan")))
    return per, mean


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
