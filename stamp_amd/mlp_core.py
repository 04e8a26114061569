"""Thin wrappers of the three one-call entries of the MLP / Linear heads (csrc/mlp.hip; reference src/stamp/modeling/models/mlp.py:6-62):
`forward_infer` (amds_mlp_forward), `forward_train` (amds_mlp_train_forward), `backward` (amds_mlp_train_backward).

dims = (dim_input, dim_hidden, dim_output, num_layers); num_layers = 1 is the `Linear` head (dim_hidden is then ignored).  Weights are contiguous fp32 device
tensors in torch's [out][in] layout, read in place (views of one flat buffer are fine: the library asks for no alignment beyond 4 bytes).  x is [rows, F] fp16 or
fp32 with unit column stride and any row stride >= F; other dtypes are converted to fp32 first.  Every product is exact fp32 at every
`torch.get_float32_matmul_precision()` setting.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib, ops

MAX_LAYERS = _lib.MLP_MAX_LAYERS


def linear_layers(model: nn.Module) -> list[tuple[str, nn.Linear]]:
    """The chain's Linear modules with their state-dict prefixes, in order: `mlp.0`, `mlp.3`, ... of `mil.MLP` (mlp.py:24-32), `fc` of `mil.Linear` (:47-62)."""
    if hasattr(model, "mlp"):
        return [(f"mlp.{i}", m) for i, m in enumerate(model.mlp) if isinstance(m, nn.Linear)]
    if hasattr(model, "fc"):
        return [("fc", model.fc)]
    raise TypeError(f"expected stamp_amd.mil.MLP or Linear, got {type(model).__name__}")


def model_dims(model: nn.Module) -> tuple[int, int, int, int]:
    """(dim_input, dim_hidden, dim_output, num_layers) of a `mil.MLP` / `mil.Linear`; more layers than the library takes is a ValueError."""
    lin = [m for _, m in linear_layers(model)]
    check_layers(len(lin))
    hidden = lin[0].out_features if len(lin) > 1 else 1
    for i, m in enumerate(lin):
        want_in = lin[0].in_features if i == 0 else hidden
        want_out = lin[-1].out_features if i == len(lin) - 1 else hidden
        if (m.in_features, m.out_features) != (want_in, want_out):
            raise ValueError(f"layer {i} is {m.in_features} -> {m.out_features}, expected {want_in} -> {want_out} (one hidden width throughout)")
    return lin[0].in_features, hidden, lin[-1].out_features, len(lin)


def check_layers(num_layers: int) -> None:
    if not 1 <= int(num_layers) <= MAX_LAYERS:
        raise ValueError(f"num_layers={num_layers}: the HIP MLP head takes 1 to {MAX_LAYERS} layers")


def _cfg(dims) -> "_lib.MlpCfg":
    check_layers(dims[3])
    return _lib.MlpCfg(*[int(v) for v in dims])


def _need(fn, cfg, rows: int, what: str) -> int:
    n = fn(C.byref(cfg), int(rows))
    if n == 0:
        _lib.check(-1, what)
    return n


def weights_struct(ws, bs, cls=None):
    """amds_mlp_weights (or amds_mlp_grads with cls=_lib.MlpGrads) over per-layer fp32 device tensors -> (struct, the tensors kept alive)."""
    s = (cls or _lib.MlpWeights)()
    keep = []
    for i, (w, b) in enumerate(zip(ws, bs)):
        assert w.dtype == torch.float32 and b.dtype == torch.float32 and w.is_contiguous() and b.is_contiguous() and w.is_cuda and b.is_cuda
        s.w[i], s.b[i] = w.data_ptr(), b.data_ptr()
        keep += [w, b]
    return s, keep


def _rows(x: torch.Tensor, dims) -> torch.Tensor:
    ops._dev(x)
    if x.dim() != 2 or x.shape[1] != dims[0]:
        raise ValueError(f"features must be [rows, {dims[0]}], got {tuple(x.shape)}")
    if x.dtype not in (torch.float16, torch.float32):
        x = x.float()
    if x.shape[0] > 1 and (x.stride(1) != 1 or x.stride(0) < dims[0]) or x.shape[0] <= 1 and x.stride(1) != 1:
        x = x.contiguous()
    return x


def _ld(x: torch.Tensor) -> int:
    return int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1])


def forward_infer(w, dims, x: torch.Tensor) -> torch.Tensor:
    """[rows, F] -> logits fp32 [rows, C]: amds_mlp_forward, ONE call.  A row's bits depend on that row and the weights only."""
    x = _rows(x, dims)
    dev, rows = x.device, x.shape[0]
    lib, cfg = _lib.lib(), _cfg(dims)
    ws = ops.scratch("mlp", dev, _need(lib.amds_mlp_workspace_bytes, cfg, rows, "mlp_workspace_bytes"))
    logits = torch.empty(rows, dims[2], dtype=torch.float32, device=dev)
    _lib.check(lib.amds_mlp_forward(C.byref(cfg), C.byref(w), x.data_ptr(), ops._DT[x.dtype], _ld(x), rows, logits.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()),
               "mlp_forward")
    return logits


def forward_train(w, dims, x: torch.Tensor, *, p: float, seed: int):
    """-> (logits [rows, C], saved): amds_mlp_train_forward.  `saved` holds what `backward` needs (the hidden activations, the rows, the dropout setting)."""
    x = _rows(x, dims)
    dev, rows = x.device, x.shape[0]
    lib, cfg = _lib.lib(), _cfg(dims)
    arena = ops.alloc(_need(lib.amds_mlp_train_saved_bytes, cfg, rows, "mlp_train_saved_bytes"), torch.uint8, dev)
    ws = ops.scratch("mlp_train", dev, _need(lib.amds_mlp_train_workspace_bytes, cfg, rows, "mlp_train_workspace_bytes"))
    logits = torch.empty(rows, dims[2], dtype=torch.float32, device=dev)
    seed = int(seed) & (2 ** 64 - 1)
    _lib.check(lib.amds_mlp_train_forward(C.byref(cfg), C.byref(w), x.data_ptr(), ops._DT[x.dtype], _ld(x), rows, float(p), seed, logits.data_ptr(), arena.data_ptr(),
                                          arena.numel(), ws.data_ptr(), ws.numel(), ops._stream()), "mlp_train_forward")
    return logits, dict(arena=arena, x=x, dims=tuple(dims), w=w, p=float(p), seed=seed)


def backward(saved: dict, dlogits: torch.Tensor, *, grads: "_lib.MlpGrads | None" = None, need_params: bool = True, need_x: bool = False):
    """amds_mlp_train_backward.  grads: an amds_mlp_grads over the caller's buffers (the trainer's flat G); without one and need_params, fresh tensors are returned as
    ([dW_i], [db_i]).  -> (G or None, dx [rows, F] or None)."""
    x, dims = saved["x"], saved["dims"]
    dev, rows = x.device, x.shape[0]
    lib, cfg = _lib.lib(), _cfg(dims)
    Fd, H, Cc, L = dims
    G = None
    if grads is None and need_params:
        ins = [Fd if i == 0 else H for i in range(L)]
        outs = [Cc if i == L - 1 else H for i in range(L)]
        G = ([ops.alloc((o, i), torch.float32, dev) for i, o in zip(ins, outs)], [ops.alloc((o,), torch.float32, dev) for o in outs])
        grads, _ = weights_struct(G[0], G[1], _lib.MlpGrads)
    dx = ops.alloc((rows, Fd), torch.float32, dev) if need_x else None
    ws = ops.scratch("mlp_train", dev, _need(lib.amds_mlp_train_workspace_bytes, cfg, rows, "mlp_train_workspace_bytes"))
    dlogits = dlogits.detach().to(dev, torch.float32).contiguous()
    _lib.check(lib.amds_mlp_train_backward(C.byref(cfg), C.byref(saved["w"]), x.data_ptr(), ops._DT[x.dtype], _ld(x), rows, saved["p"], saved["seed"], dlogits.data_ptr(),
                                           saved["arena"].data_ptr(), saved["arena"].numel(), C.byref(grads) if grads is not None else None, 1 if need_x else 0, ops._p(dx),
                                           ws.data_ptr(), ws.numel(), ops._stream()), "mlp_train_backward")
    return G, dx


__all__ = ["MAX_LAYERS", "linear_layers", "model_dims", "check_layers", "weights_struct", "forward_infer", "forward_train", "backward"]
