"""The survival and regression statistics of include/amdstamp.h (amds_survival_groups, amds_regression_moments), independent of the kernels: the
authority of test_cpu_survival_stats.py and test_gpu_survival_stats.py.

* `survival` loops over the distinct times of one problem (for a resample: of the gathered arrays) and forms the log-rank sums O, E, V and the two
  Kaplan-Meier products EXACTLY over `fractions.Fraction`; floats appear only when a finished rational is converted.  The at-risk table, the medians and
  the comparable pairs are brute force.  This restates the published algorithms -- the two-sample log-rank test with its hypergeometric variance (Mantel
  1966; Peto & Peto 1972) and the product-limit estimator (Kaplan & Meier 1958) -- as lifelines' `logrank_test` and `KaplanMeierFitter` compute them;
  lifelines is not a dependency, and this is its algorithm, not its code.
* `moments` / `regression` are the eight regression moments in numpy float64, every sum exactly rounded (`math.fsum`), and the numbers sklearn and scipy
  form from them.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import rank_oracle as R

NAN = float("nan")


def median_cut_off(score, time, event) -> float:
    """numpy's nanmedian of the valid items' scores in float64."""
    ok = R.valid_mask(score, time, event)
    return float(np.nanmedian(np.asarray(score, np.float32)[ok].astype(np.float64))) if ok.any() else NAN


def survival(score, time, event, cut_off=None, grid=None) -> dict:
    """-> counts [(items, deaths, censored) of LOW, of HIGH], O / E / V / chi2 / p (floats; NaN with an empty group), exact (O, E, V as Fractions),
    pairs, median [LOW, HIGH], cut_off, and with a grid km [2][G] and table [2][G][3]."""
    ok = R.valid_mask(score, time, event)
    s = np.asarray(score, np.float32)[ok].astype(np.float64)
    t = np.asarray(time, np.float32)[ok]
    e = np.asarray(event, np.float64)[ok] == 1
    if cut_off is None:
        cut_off = float(np.nanmedian(s)) if len(s) else NAN
    high = s > cut_off
    groups = [~high, high]
    counts = [(int(g.sum()), int((g & e).sum()), int((g & ~e).sum())) for g in groups]
    both = counts[0][0] > 0 and counts[1][0] > 0
    E = V = Fraction(0)
    S = [Fraction(1), Fraction(1)]
    steps = []                                                   # (t_k, S_LOW after t_k, S_HIGH after t_k)
    for tk in np.unique(t):                                      # ascending; -0.0 and +0.0 are one time
        at, risk = t == tk, t >= tk
        n, d = int(risk.sum()), int((at & e).sum())
        ng = [int((risk & g).sum()) for g in groups]
        dg = [int((at & e & g).sum()) for g in groups]
        if d:
            E += Fraction(d * ng[1], n)
            if n > 1:
                V += Fraction(d * (n - d), n - 1) * Fraction(ng[1], n) * Fraction(n - ng[1], n)
        for g in range(2):
            if dg[g]:
                S[g] *= Fraction(ng[g] - dg[g], ng[g])
        steps.append((tk, S[0], S[1]))
    O = counts[1][1]
    out = {"counts": counts, "cut_off": cut_off, "exact": (Fraction(O), E, V) if both else None,
           "pairs": int(((t[:, None] < t[None, :]) & e[:, None]).sum()) if len(t) <= 6000 else None}
    if both:
        chi2 = float((O - E) ** 2 / V) if V > 0 else 0.0
        out.update(O=float(O), E=float(E), V=float(V), chi2=chi2, p=math.erfc(math.sqrt(chi2 / 2)))
    else:
        out.update(O=NAN, E=NAN, V=NAN, chi2=NAN, p=NAN)
    med = []
    for g in range(2):
        if counts[g][0] == 0:
            med.append(NAN)
            continue
        reached = [float(tk) for tk, *Sk in steps if Sk[g] <= Fraction(1, 2)]
        med.append(reached[0] if reached else math.inf)
    out["median"] = med
    if grid is not None:
        grid = np.asarray(grid, np.float32)
        km = np.full((2, len(grid)), NAN)
        table = np.full((2, len(grid), 3), -1, np.int64)
        for k, x in enumerate(grid):
            if np.isnan(x):
                continue
            past = [st for st in steps if st[0] <= x]
            for g in range(2):
                if counts[g][0]:
                    km[g, k] = float(past[-1][1 + g]) if past else 1.0
                m = groups[g]
                table[g, k] = (int((m & (t >= x)).sum()), int((m & (t <= x) & e).sum()), int((m & (t <= x) & ~e).sum()))
        out.update(km=km, table=table)
    return out


def moments(truth, pred) -> list:
    """[n, mean_t, mean_p, Sxx, Syy, Sxy, sum |p - t|, sum (p - t)^2] over the rows without a NaN, float64, every sum exactly rounded."""
    t, p = np.asarray(truth, np.float32).astype(np.float64), np.asarray(pred, np.float32).astype(np.float64)
    ok = ~(np.isnan(t) | np.isnan(p))
    t, p = t[ok], p[ok]
    n = len(t)
    if n == 0:
        return [0.0, NAN, NAN, 0.0, 0.0, 0.0, 0.0, 0.0]
    mt, mp = math.fsum(t) / n, math.fsum(p) / n
    dt, dp, r = t - mt, p - mp, p - t
    return [float(n), mt, mp, math.fsum(dt * dt), math.fsum(dp * dp), math.fsum(dt * dp), math.fsum(np.abs(r)), math.fsum(r * r)]


def regression(m) -> dict:
    """The report's numbers from the eight moments: sklearn's r2_score / mean_absolute_error / root of mean_squared_error, scipy's pearsonr (NaN for a
    constant column, as the reference) and linregress(truth, pred)."""
    n, mt, mp, sxx, syy, sxy, sae, sse = m
    out = {"count": int(n), "mae": sae / n if n else NAN, "rmse": math.sqrt(sse / n) if n else NAN}
    out["r2_score"] = NAN if n < 2 else (1.0 - sse / sxx if sxx > 0 else (1.0 if sse == 0 else 0.0))
    den = math.sqrt(sxx) * math.sqrt(syy)
    r = max(-1.0, min(1.0, sxy / den)) if den > 0 else 0.0
    out["pearson_r"] = r if sxx > 0 and syy > 0 else NAN
    if n >= 2 and sxx > 0:
        slope = sxy / sxx
        out.update(slope=slope, intercept=mp - slope * mt, stderr=math.sqrt(max(0.0, 1.0 - r * r) * syy / sxx / (n - 2)) if n > 2 else 0.0)
    else:
        out.update(slope=NAN, intercept=NAN, stderr=NAN)
    return out
