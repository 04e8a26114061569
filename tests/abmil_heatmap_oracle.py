"""The heat-map scores of the gated-attention MIL head (amds_abmil_heatmap, stamp_amd/heatmaps.py) in plain torch, at any dtype, on tests/abmil_oracle.py:

* `cam_autograd`: the reference's own definition (src/stamp/heatmaps/__init__.py:43-54): per class, | mean_f x_nf d logit_c / d x_nf |, the derivative from
  torch's autograd on `abmil_oracle._forward`.  Bags are independent, so d (sum over the bags of logit_c) / d x gives every row its own bag's derivative.
* `closed_form`: the same quantity from the chain rule written out (include/amdstamp.h, "Heat-map scores"): one class-independent vector r_n per row, then
  three dots per row and class.  Pinned against `cam_autograd` in fp64 by test_cpu_abmil_heatmap_oracle.py.
* `tile_logits`: every row as a bag of its own through `abmil_oracle.forward` (reference :417-427).
"""
from __future__ import annotations

import torch

import abmil_oracle as A


def cam_autograd(x: torch.Tensor, lengths, w: dict, dtype: torch.dtype) -> torch.Tensor:
    """-> cam_raw [C, rows] at `dtype`."""
    xs = x.detach().to(dtype).clone().requires_grad_(True)
    logits = A._forward(xs, lengths, w, None, dtype)["logits"]
    cams = []
    for c in range(logits.shape[1]):
        jac, = torch.autograd.grad(logits[:, c].sum(), xs, retain_graph=True)
        cams.append((xs.detach() * jac).mean(-1).abs())
    return torch.stack(cams)


def closed_form(x: torch.Tensor, lengths, w: dict, dtype: torch.dtype) -> dict:
    """-> dict(cam_raw [C, rows], probs [rows], logits [bags, C], gbar [bags, C]) at `dtype`, eval mode."""
    w = {k: w[k].to(x.device, dtype) for k in A.KEYS}
    x = x.to(dtype)
    h = torch.relu(x @ w[A.FC_W].T + w[A.FC_B])
    t = torch.tanh(h @ w[A.A_W].T + w[A.A_B])
    q = torch.sigmoid(h @ w[A.B_W].T + w[A.B_B])
    wc = w[A.C_W].reshape(-1)
    s = (t * q) @ wc + w[A.C_B]
    u = wc * q * (1 - t * t)
    v = wc * t * q * (1 - q)
    r = u @ w[A.A_W] + v @ w[A.B_W]                                   # [rows, L]: the one product, the same for every class
    e = (h - w[A.FC_B]) * (h > 0)                                      # x W_fc^T on the live units
    B = (e * r).sum(-1)                                                # [rows]
    Anc = e @ w[A.CLS_W].T                                             # [rows, C]
    g = h @ w[A.CLS_W].T                                               # [rows, C]
    cams, probs, logits, gbars = [], [], [], []
    for sb, hb, Bb, Ab, gb in zip(s.split(list(lengths)), h.split(list(lengths)), B.split(list(lengths)), Anc.split(list(lengths)), g.split(list(lengths))):
        p = torch.softmax(sb, dim=0)
        gbar = p @ gb                                                  # [C] = logits - b_cls
        cams.append((p[:, None] * (Ab + (gb - gbar) * Bb[:, None])).abs() / x.shape[1])
        probs.append(p)
        gbars.append(gbar)
        logits.append((p @ hb) @ w[A.CLS_W].T + w[A.CLS_B])
    return {"cam_raw": torch.cat(cams).T.contiguous(), "probs": torch.cat(probs), "logits": torch.stack(logits), "gbar": torch.stack(gbars)}


def tile_logits(x: torch.Tensor, w: dict, dtype: torch.dtype) -> torch.Tensor:
    """-> [rows, C]: the logits of every row as a one-row bag."""
    return A.forward(x, [1] * x.shape[0], w, dtype=dtype)["logits"]
