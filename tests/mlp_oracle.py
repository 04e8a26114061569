"""fp64 forward and backward of the MLP / Linear chain (reference src/stamp/modeling/models/mlp.py:24-32) with GIVEN keep masks: the oracle of
amds_mlp_forward / amds_mlp_train_forward / amds_mlp_train_backward (tests/test_gpu_mlp_train.py), pinned by tests/test_cpu_mlp_oracle.py.

Written out by hand -- no autograd -- so that the GPU tests compare against something other than the rule they implement:
    a_0 = x;  z_i = a_i W_i^T + b_i;  a_(i+1) = m_i * scale * relu(z_i)  (hidden layers);  logits = z_(L-1)
    dz_(L-1) = dlogits;  dW_i = dz_i^T a_i;  db_i = colsum(dz_i);  da_i = dz_i W_i;  dz_(i-1) = da_i * m_(i-1) * scale * [z_(i-1) > 0]
"""
from __future__ import annotations

import torch


def forward(x, ws, bs, masks=None, scale: float = 1.0):
    """x [rows, F]; ws / bs: per-layer [out, in] / [out]; masks: per HIDDEN layer a 0/1 tensor [rows, hidden] or None (no dropout).
    -> (logits fp64 [rows, C], cache for `backward`)."""
    a = x.double()
    acts, pre = [a], []
    L = len(ws)
    for i in range(L):
        z = a @ ws[i].double().t() + bs[i].double()
        pre.append(z)
        if i < L - 1:
            a = torch.clamp(z, min=0.0)
            if masks is not None and masks[i] is not None:
                a = a * masks[i].double() * float(scale)
            acts.append(a)
    return pre[-1], dict(acts=acts, pre=pre, masks=masks, scale=float(scale), ws=[w.double() for w in ws])


def backward(cache, dlogits):
    """-> (dWs, dbs, dx), all fp64."""
    acts, pre, masks, scale, ws = cache["acts"], cache["pre"], cache["masks"], cache["scale"], cache["ws"]
    L = len(ws)
    dz = dlogits.double()
    dWs, dbs = [None] * L, [None] * L
    dx = None
    for i in range(L - 1, -1, -1):
        dWs[i] = dz.t() @ acts[i]
        dbs[i] = dz.sum(dim=0)
        da = dz @ ws[i]
        if i == 0:
            dx = da
        else:
            g = (pre[i - 1] > 0).double()
            if masks is not None and masks[i - 1] is not None:
                g = g * masks[i - 1].double() * scale
            dz = da * g
    return dWs, dbs, dx


def rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    want = want.double().cpu()
    return float((got.double().cpu() - want).norm() / want.norm().clamp_min(1e-300))
