"""The gated-attention MIL head (stamp_amd/abmil.py, csrc/abmil.hip) in plain torch, at any dtype, on the device of its inputs:

    h = m_h * relu(x Wfc^T + bfc);  a = m_a * tanh(h Wa^T + ba);  g = m_g * sigmoid(h Wb^T + bb);  s = (a * g) c^T + cb
    P = softmax over the bag's rows of s;  M_b = sum_n P_n h_n;  logits_b = Wcls M_b + bcls

Weights are addressed by the reference's state-dict keys (KEYS).  `masks` are the three MULTIPLIERS (keep mask times 1 / (1 - p)) or None (eval).
Gradients come from torch's autograd on this very graph (`gradients`).

Tensors that are zero in exact arithmetic.  The softmax's backward is ds_n = P_n g_n - P_n sum_k P_k g_k, and every gradient that reaches a parameter through the
score alone (a, b, c weights and biases) is LINEAR in ds.  d c_b = sum_n ds_n is zero for every input; with equal rows in a bag ds itself is zero and all six
vanish.  fp64 then returns rounding noise (1e-17) and "error relative to max |fp64|" measures nothing.  `gradients` therefore also returns "scale:<key>" =
max |T(ds+)| with ds+_n = P_n g_n, the first of the two terms that cancel, pushed through the same linear map T: the size of what is being subtracted.  `rel_err`
takes it as the denominator ONLY where max |fp64| < 1e-9 x scale, i.e. where the fp64 value is itself nothing but rounding noise; everywhere else the
denominator is max |fp64| as stated.  Pinned against the reference's own CHIEFModel by test_cpu_abmil_oracle.py
(tests/golden/abmil_xs.npz); the yardstick and the fp64 reference of test_gpu_abmil.py.
"""
from __future__ import annotations

import torch

from gap_oracle import gamma  # noqa: F401  (the floor of the GPU test's bars)

KEYS = ("attention_net.0.weight", "attention_net.0.bias", "attention_net.3.attention_a.0.weight", "attention_net.3.attention_a.0.bias",
        "attention_net.3.attention_b.0.weight", "attention_net.3.attention_b.0.bias", "attention_net.3.attention_c.weight", "attention_net.3.attention_c.bias",
        "classifiers.weight", "classifiers.bias")
FC_W, FC_B, A_W, A_B, B_W, B_B, C_W, C_B, CLS_W, CLS_B = KEYS


def random_weights(F: int, L: int, D: int, C: int, seed: int, bias: float = 0.1) -> dict:
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {FC_W: r(L, F) / F ** 0.5, FC_B: r(L) * bias, A_W: r(D, L) / L ** 0.5, A_B: r(D) * bias, B_W: r(D, L) / L ** 0.5, B_B: r(D) * bias,
            C_W: r(1, D) / D ** 0.5, C_B: r(1) * bias, CLS_W: r(C, L) / L ** 0.5, CLS_B: r(C) * bias}


def forward(x: torch.Tensor, lengths, w: dict, masks=None, dtype: torch.dtype | None = None) -> dict:
    out = _forward(x, lengths, w, masks, dtype)
    out.pop("_probs")
    return out


def _forward(x: torch.Tensor, lengths, w: dict, masks=None, dtype: torch.dtype | None = None) -> dict:
    """x [rows, F] (bag b = the next lengths[b] rows) -> dict(logits [bags, C], attn_raw [rows], probs [rows], pooled [bags, L]) at `dtype` (default: x's)."""
    dtype = dtype or x.dtype
    w = {k: w[k].to(x.device, dtype) for k in KEYS}
    x = x.to(dtype)
    h = torch.relu(x @ w[FC_W].T + w[FC_B])
    if masks is not None:
        h = h * masks[0].to(x.device, dtype)
    a = torch.tanh(h @ w[A_W].T + w[A_B])
    g = torch.sigmoid(h @ w[B_W].T + w[B_B])
    if masks is not None:
        a, g = a * masks[1].to(x.device, dtype), g * masks[2].to(x.device, dtype)
    s = ((a * g) @ w[C_W].T + w[C_B]).reshape(-1)
    probs, pooled = [], []
    for sb, hb in zip(s.split(list(lengths)), h.split(list(lengths))):
        p = torch.softmax(sb, dim=0)
        probs.append(p)
        pooled.append(p @ hb)
    pooled = torch.stack(pooled)
    return {"logits": pooled @ w[CLS_W].T + w[CLS_B], "attn_raw": s, "probs": torch.cat(probs), "pooled": pooled, "_probs": probs}


def gradients(x: torch.Tensor, lengths, w: dict, dlogits: torch.Tensor | None = None, masks=None, dtype: torch.dtype | None = None, loss_fn=None) -> dict:
    """Forward + autograd -> the forward's dict plus "dx" and "g:<key>" for every weight.  The scalar differentiated is sum(logits * dlogits) or
    loss_fn(logits)."""
    dtype = dtype or x.dtype
    xs = x.detach().to(dtype).clone().requires_grad_(True)
    ws = {k: w[k].detach().to(x.device, dtype).clone().requires_grad_(True) for k in KEYS}
    out = _forward(xs, lengths, ws, masks, dtype)
    scalar = loss_fn(out["logits"]) if loss_fn is not None else (out["logits"] * dlogits.to(x.device, dtype)).sum()
    leaves = [xs] + [ws[k] for k in KEYS]
    plist = out.pop("_probs")
    grads = torch.autograd.grad(scalar, leaves, retain_graph=True)
    g_rows = torch.autograd.grad(scalar, plist, retain_graph=True)                      # g_n = d scalar / d P_n
    ds_plus = torch.cat([p.detach() * g for p, g in zip(plist, g_rows)])               # the first of the softmax backward's two terms
    t_plus = torch.autograd.grad(out["attn_raw"], leaves, grad_outputs=ds_plus, allow_unused=True)
    res = {k: v.detach() for k, v in out.items()}
    res["dx"] = grads[0]
    res.update({"g:" + k: g for k, g in zip(KEYS, grads[1:])})
    res.update({"scale:" + ("dx" if i == 0 else "g:" + KEYS[i - 1]): float(t.abs().max()) for i, t in enumerate(t_plus) if t is not None})
    return res


def rel_err(got: torch.Tensor, ref64: torch.Tensor, scale: float = 0.0) -> float:
    """max |got - ref| / max |ref|, per tensor; the denominator is `scale` where the reference is rounding noise against it (module docstring)."""
    ref64 = ref64.double().cpu()
    den = float(ref64.abs().max())
    if den < 1e-9 * scale:
        den = scale
    return float((got.double().cpu().reshape(ref64.shape) - ref64).abs().max()) / max(den, 1e-300)
