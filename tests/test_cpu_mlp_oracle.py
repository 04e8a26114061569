"""tests/mlp_oracle.py (the fp64 oracle of the one-call MLP / Linear entries) pinned to the reference's own `MLP` / `Linear` outputs (tests/golden/mlp.npz, written
by tools/make_golden.py from src/stamp/modeling/models/mlp.py) and to torch's fp64 autograd, at num_layers 1, 2 and 4, with and without keep masks."""
from pathlib import Path

import numpy as np
import pytest
import torch

import mlp_oracle

G = Path(__file__).parent / "golden"


def _layers(sd, prefixes):
    return [sd[p + ".weight"] for p in prefixes], [sd[p + ".bias"] for p in prefixes]


def test_forward_matches_the_references_mlp_and_linear():
    z = np.load(G / "mlp.npz")
    sm = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("mlp:")}
    sl = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("lin:")}
    ws, bs = _layers(sm, ["mlp.0", "mlp.3", "mlp.6"])          # num_layers = 3: Linear at 0, 3, 6 of the Sequential (mlp.py:24-32)
    lw, lb = _layers(sl, ["fc"])
    x2, x3 = torch.from_numpy(z["x2"]), torch.from_numpy(z["x3"])
    for x, key in ((x2, "2"), (x3.mean(dim=1), "3")):          # a [B, T, F] batch is mean-pooled first (mlp.py:40-41)
        y, _ = mlp_oracle.forward(x, ws, bs)
        np.testing.assert_allclose(y.numpy(), z[f"mlp_y{key}"], rtol=1e-5, atol=1e-6)
        y, _ = mlp_oracle.forward(x, lw, lb)
        np.testing.assert_allclose(y.numpy(), z[f"lin_y{key}"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("num_layers", [1, 2, 4])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_forward_and_backward_match_torch_fp64_autograd(num_layers, p):
    g = torch.Generator().manual_seed(10 * num_layers + int(p * 100))
    rows, F, H, C = 11, 13, 9, 3
    ins = [F if i == 0 else H for i in range(num_layers)]
    outs = [C if i == num_layers - 1 else H for i in range(num_layers)]
    ws = [torch.randn(o, i, generator=g, dtype=torch.float64).requires_grad_() for i, o in zip(ins, outs)]
    bs = [torch.randn(o, generator=g, dtype=torch.float64).requires_grad_() for o in outs]
    x = torch.randn(rows, F, generator=g, dtype=torch.float64).requires_grad_()
    scale = 1.0 / (1.0 - p)
    masks = [(torch.rand(rows, H, generator=g) >= p).to(torch.uint8) for _ in range(num_layers - 1)] if p else None
    a = x
    for i in range(num_layers):
        a = torch.nn.functional.linear(a, ws[i], bs[i])
        if i < num_layers - 1:
            a = torch.relu(a)
            if masks is not None:
                a = a * masks[i].double() * scale
    dl = torch.randn(rows, C, generator=g, dtype=torch.float64)
    grads = torch.autograd.grad(a, [x] + ws + bs, dl)
    y, cache = mlp_oracle.forward(x.detach(), [w.detach() for w in ws], [b.detach() for b in bs], masks, scale)
    dWs, dbs, dx = mlp_oracle.backward(cache, dl)
    assert mlp_oracle.rel_l2(y, a.detach()) < 1e-14
    assert mlp_oracle.rel_l2(dx, grads[0]) < 1e-13
    for i in range(num_layers):
        assert mlp_oracle.rel_l2(dWs[i], grads[1 + i]) < 1e-13
        assert mlp_oracle.rel_l2(dbs[i], grads[1 + num_layers + i]) < 1e-13
