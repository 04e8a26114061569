"""The curve statistics of include/amdstamp.h (amds_binary_curves) as plain numpy: every decision -- the order, the ties, the segment a grid point
falls into -- is made on integers or on fp32 compares, ratios are formed in float64 from integers, sums are exact (math.fsum).  No sklearn here:
tests/test_cpu_curve_stats.py pins this file against sklearn + np.interp, tests/test_gpu_curve_stats.py pins the library against this file."""
from __future__ import annotations

import math

import numpy as np

NAN = float("nan")


def curve_points(score, label, weight=None):
    """-> (TP, FP): int64 arrays, the weighted positives / negatives with score >= threshold t, for the distinct scores that carry weight, descending.
    label 1 = positive, 0 = negative, anything else invalid; a NaN score is invalid; compares are fp32's (np.unique: -0 == +0, denormals kept)."""
    score = np.asarray(score, np.float32).reshape(-1)
    label = np.asarray(label).reshape(-1)
    w = np.ones(score.shape[0], np.int64) if weight is None else np.asarray(weight, np.int64).reshape(-1)
    valid = ~np.isnan(score) & ((label == 0) | (label == 1))
    s, y, w = score[valid], label[valid].astype(np.int64), w[valid]
    levels, inv = np.unique(s, return_inverse=True)
    wp, wn = np.zeros(len(levels), np.int64), np.zeros(len(levels), np.int64)
    np.add.at(wp, inv, w * y)
    np.add.at(wn, inv, w * (1 - y))
    wp, wn = wp[::-1], wn[::-1]
    keep = (wp + wn) > 0
    return np.cumsum(wp[keep]), np.cumsum(wn[keep])


def _trapezoid(x, y):
    return math.fsum((x[1:] - x[:-1]) * ((y[1:] + y[:-1]) * 0.5))


def curves(score, label, grid=1000, weight=None) -> dict:
    """-> counts (P, N), ap, pr_area, pr_area_grid, roc [grid], pr [grid]; the float values NaN for a problem without a positive or a negative,
    pr_area_grid NaN and the grids empty for grid == 0."""
    TP, FP = curve_points(score, label, weight)
    P, N = (int(TP[-1]), int(FP[-1])) if len(TP) else (0, 0)
    G = int(grid)
    if P == 0 or N == 0:
        return {"counts": (P, N), "ap": NAN, "pr_area": NAN, "pr_area_grid": NAN, "roc": np.full(G, NAN), "pr": np.full(G, NAN)}
    prec = TP / (TP + FP)
    tp0, prec0 = np.r_[0, TP[:-1]], np.r_[1.0, prec[:-1]]
    dr = (TP - tp0) / float(P)
    out = {"counts": (P, N), "ap": math.fsum(dr * prec), "pr_area": math.fsum(dr * ((prec + prec0) * 0.5)), "pr_area_grid": NAN,
           "roc": np.zeros(0), "pr": np.zeros(0)}
    if G == 0:
        return out
    S, k = G - 1, np.arange(G, dtype=np.int64)
    # ROC: points (FP, TP) preceded by (0, 0); j = the last point with FP_j * (G - 1) <= k * N
    xs, ys = np.r_[0, FP], np.r_[0, TP]
    j = np.searchsorted(xs * S, k * N, side="right") - 1
    j1 = np.minimum(j + 1, len(xs) - 1)
    last = j == len(xs) - 1
    den = np.where(last, 1, xs[j1] - xs[j])
    val = (ys[j] + ((k * N) / float(S) - xs[j]) / den * (ys[j1] - ys[j])) / float(P)
    out["roc"] = np.where(last, 1.0, val)
    # PR: points (TP, precision) preceded by (0, 1.0); j = the last point with TP_j * (G - 1) <= k * P
    xs, ys = np.r_[0, TP], np.r_[1.0, prec]
    j = np.searchsorted(xs * S, k * P, side="right") - 1
    j1 = np.minimum(j + 1, len(xs) - 1)
    last = j == len(xs) - 1
    den = np.where(last, 1, xs[j1] - xs[j])
    val = ys[j] + ((k * P) / float(S) - xs[j]) / den * (ys[j1] - ys[j])
    out["pr"] = np.where(last, ys[j], val)
    out["pr_area_grid"] = _trapezoid(k / float(S), out["pr"])
    return out


def knife_edges(score, label, grid, weight=None):
    """-> (roc mask, pr mask) over the grid points k: k * N == FP_t * (G - 1), k * P == TP_t * (G - 1) for some curve point t -- the points at which
    floating-point grids and rates may fall on either side of an equality this definition decides exactly."""
    TP, FP = curve_points(score, label, weight)
    S, k = int(grid) - 1, np.arange(int(grid), dtype=np.int64)
    return np.isin(k * int(FP[-1]), FP * S), np.isin(k * int(TP[-1]), TP * S)
