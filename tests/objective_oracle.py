"""The four training objectives of include/amdstamp.h ("Training objectives"), their gradients with respect to the logits and the per-row values, in fp64
numpy: written from the formulas there, closed-form gradients (no autograd), independent of `stamp_amd.losses` and of the kernels.

Each function takes array-likes, computes in float64 and returns (loss: float, dlogits: float64 array shaped like the logits, has_grad: int)."""
from __future__ import annotations

import numpy as np

CE, L1, COX_EFRON, COX_BRESLOW = range(4)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def ce_rows(logits, targets, weight=None) -> np.ndarray:
    """Row n: sum_c -w_c y_nc log softmax(x_n)_c, max-shifted."""
    x, y = _f64(logits), _f64(targets)
    w = np.ones(x.shape[1]) if weight is None else _f64(weight)
    d = x - x.max(axis=1, keepdims=True)
    logp = d - np.log(np.exp(d).sum(axis=1, keepdims=True))
    return -(w[None, :] * y * logp).sum(axis=1)


def ce(logits, targets, weight=None):
    x, y = _f64(logits), _f64(targets)
    B = x.shape[0]
    w = np.ones(x.shape[1]) if weight is None else _f64(weight)
    d = x - x.max(axis=1, keepdims=True)
    p = np.exp(d)
    p /= p.sum(axis=1, keepdims=True)
    wy = w[None, :] * y
    return float(ce_rows(x, y, w).sum() / B), (p * wy.sum(axis=1, keepdims=True) - wy) / B, 1


def l1_rows(pred, target) -> np.ndarray:
    return np.abs(_f64(pred).reshape(-1) - _f64(target).reshape(-1))


def l1(pred, target):
    p = _f64(pred)
    d = p.reshape(-1) - _f64(target).reshape(-1)
    return float(np.abs(d).mean()), (np.sign(d) / d.size).reshape(p.shape), 1


def _cox(scores, time, event, efron: bool):
    """loss = -(1/G) sum_{events i} [(lh_i - mx) - log(R_i - f_i D_i)]; Efron: f_i = r_i / d_i, G = distinct event times; Breslow: f_i = 0, G = events.
    Straight loops over the items: this is the statement, not an implementation."""
    s = _f64(scores)
    lh, t, ev = s.reshape(-1), _f64(time).reshape(-1), _f64(event).reshape(-1) != 0
    n = lh.size
    if not ev.any():
        return 0.0, np.zeros_like(s), 0
    e = np.exp(lh - lh.max())
    inv_q, f_q, total, groups = np.zeros(n), np.zeros(n), 0.0, 0
    for i in np.nonzero(ev)[0]:
        tied = (t == t[i]) & ev
        r = int(tied[:i].sum())
        f = r / int(tied.sum()) if efron else 0.0
        q = e[t >= t[i]].sum() - f * e[tied].sum()
        total += (lh[i] - lh.max()) - np.log(q)
        inv_q[i], f_q[i] = 1.0 / q, f / q
        groups += r == 0
    G = groups if efron else int(ev.sum())
    grad = np.empty(n)
    for k in range(n):
        a = inv_q[t <= t[k]].sum()
        b = f_q[t == t[k]].sum() if ev[k] else 0.0
        grad[k] = (e[k] * (a - b) - float(ev[k])) / G
    return float(-total / G), grad.reshape(s.shape), 1


def cox_efron(scores, time, event):
    return _cox(scores, time, event, True)


def cox_breslow(scores, time, event):
    return _cox(scores, time, event, False)


def step(kind: int, logits, targets, weight=None):
    """The oracle of amds_objective_step on the targets layout the entry takes (CE [B, C]; L1 [B]; Cox [B, 2] = time, event)."""
    if kind == CE:
        return ce(logits, targets, weight)
    if kind == L1:
        return l1(logits, targets)
    y = _f64(targets).reshape(-1, 2)
    return _cox(logits, y[:, 0], y[:, 1], kind == COX_EFRON)


def rows(kind: int, logits, targets, weight=None) -> np.ndarray:
    return ce_rows(logits, targets, weight) if kind == CE else l1_rows(logits, targets)
