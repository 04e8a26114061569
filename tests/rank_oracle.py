"""Brute-force oracles of the concordance statistic for the rank-metric tests (test_cpu_rank_metrics.py, test_gpu_rank_metrics.py).

The definition (include/amdstamp.h, `amds_concordance_counts`): items i have a risk score_i (higher = worse), a time_i and an event_i in {0, 1}.  The ordered
pair (i, j) is permissible when event_i == 1 and (time_i < time_j or (time_i == time_j and event_j == 0)), concordant when score_i > score_j, tied when
score_i == score_j; C = (concordant + tied / 2) / permissible.

* `pair_counts` -- the definition, literally, as O(n^2) numpy broadcasting in fp32.
* `sweep_counts` -- an independent restatement of what lifelines.utils.concordance_index(time, -score, event) does: subjects swept by exit time, the
  predictions of the deaths so far kept sorted; the deaths at a time are ranked against the EARLIER deaths only and then inserted, the subjects censored at
  that time are ranked after the insertion and never inserted.  (lifelines itself is not a dependency; this is its algorithm, not its code.)
"""
from __future__ import annotations

import bisect

import numpy as np


def valid_mask(score, time, event) -> np.ndarray:
    """Items that take part: score and time not NaN, event 0 or 1."""
    e = np.asarray(event, dtype=np.float64)
    return ~(np.isnan(np.asarray(score, np.float32)) | np.isnan(np.asarray(time, np.float32))) & ((e == 0) | (e == 1))


def pair_counts(score, time, event) -> tuple[int, int, int, int]:
    """(concordant, tied, permissible, valid items) by the definition, over all ordered pairs."""
    ok = valid_mask(score, time, event)
    s = np.asarray(score, np.float32)[ok]
    t = np.asarray(time, np.float32)[ok]
    e = np.asarray(event, np.float64)[ok] == 1
    perm = e[:, None] & ((t[:, None] < t[None, :]) | ((t[:, None] == t[None, :]) & ~e[None, :]))
    conc = perm & (s[:, None] > s[None, :])
    tied = perm & (s[:, None] == s[None, :])
    return int(conc.sum()), int(tied.sum()), int(perm.sum()), int(ok.sum())


def c_of(counts) -> float:
    conc, tied, perm = counts[:3]
    return float("nan") if perm == 0 else (conc + 0.5 * tied) / perm


def sweep_counts(score, time, event) -> tuple[int, int, int]:
    """(concordant, tied, permissible) by the time-ordered sweep over NaN-free data."""
    pred = -np.asarray(score, np.float64)          # lifelines: a higher prediction = a longer survival
    time = np.asarray(time, np.float64)
    event = np.asarray(event).astype(bool)
    deaths: list[float] = []                       # predictions of the deaths seen so far, sorted
    correct = tied = pairs = 0

    def rank(p):
        nonlocal correct, tied, pairs
        lo, hi = bisect.bisect_left(deaths, p), bisect.bisect_right(deaths, p)
        pairs += len(deaths)
        correct += lo                              # earlier deaths predicted to live SHORTER than this subject
        tied += hi - lo

    for t in np.unique(time):
        at = time == t
        died = pred[at & event]
        for p in died:                             # deaths at one time are not compared with one another
            rank(p)
        for p in died:
            bisect.insort(deaths, p)
        for p in pred[at & ~event]:                # censored at t: outlived the deaths at t
            rank(p)
    return correct, tied, pairs


def heavy_ties(n: int, seed: int, p_event: float = 0.6):
    """The GPU tests' data: scores rounded to 8 values, integer times 0..9, random events -> (score f32, time f32, event u8)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 8, n).astype(np.float32) / 8, rng.integers(0, 10, n).astype(np.float32), (rng.random(n) < p_event).astype(np.uint8))
