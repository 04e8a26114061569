"""Training of the TransMIL head on the HIP path without autograd through the network: `HipTransMilTrainer`, the `flat_trainer.FlatTrainer` of `trans_mil`.

One `step` (`flat_trainer.py`: the flat `P` / `G` / `m` / `v` buffers, their views, the step protocol, the schedule) runs around
`amds_transmil_train_forward` / `_backward` (ONE library call each, csrc/transmil_train.hip).  What is this head's own:
* Every TransMIL tensor holds a multiple of 4 elements except the last one (`_fc2.bias`), so every view starts 16-byte aligned.
* `amds_transmil_weights` is built ONCE over the views of `P`: the training forward, the backward, `amds_transmil_forward` and the ragged forward all read fp32
  weights, so there is no packed operand copy and nothing to refresh after an optimiser step.
* `amds_transmil_grads` is built ONCE over the views of `G`: the library writes every gradient where AdamW reads it.  PPEG's six gradients are windows of the
  [50, dim_hidden] tap-correlation table the backward fills (a persistent buffer); `amds_ppeg_grads_unpack` cuts it into `G` in one launch
  (the `nn.Module` path slices it with about ten torch ops, `transmil_core.backward`).
* per step the host allocates the saved-activation arena (as `transmil_core.forward_train` does; torch's caching allocator hands the same block back), the
  [Bb, C] logits it returns and the loss's few [Bb, C] tensors; the backward's workspace is `ops.scratch`.

Precision follows `torch.get_float32_matmul_precision()` at every call like the module (exact fp32 MFMA at "highest", bf16 x 3 below;
`ops.sync_float32_matmul_precision`): fp32's range either way, so there is no operand cast and no loss scale.
Dropout: the reference's one site (`to_out`'s Dropout(0.1), trans_mil.py:63-66) with the module's counter-based masks.  Train-mode `mask` does not exist on
this path (the reference's Lightning wrappers pass none, models/__init__.py:286-313).  `coords` are ignored, as the reference's TransMIL ignores them
(trans_mil.py:299-301).  There is no CPU fallback: `step` / `predict*` raise on CPU tensors (the constructor itself only lays out buffers, on whatever
`device` names).
"""
from __future__ import annotations

import torch

from . import _lib, transmil_core
from . import train_ops as T
from .flat_trainer import FlatTrainer, flat_layout
from .mil import TransMIL

_PPEG = ("pos_layer.proj.weight", "pos_layer.proj1.weight", "pos_layer.proj2.weight", "pos_layer.proj.bias", "pos_layer.proj1.bias", "pos_layer.proj2.bias")


class HipTransMilTrainer(FlatTrainer):
    valid_max_rows_per_call = 262144          # padded token rows one ragged validation call may hold (`group_valid_bags`; the workspace scales with them)

    def __init__(self, model: TransMIL, *, device="cuda", max_lr: float = 1e-4, div_factor: float = 25.0, total_steps: int = 1000,
                 weight_decay: float = 0.01, dropout: bool | None = None, sched_interval: str = "epoch") -> None:
        """dropout: None = the reference's train mode (Dropout(0.1) on both `to_out`s, `transmil_core.P_OUT`); False = off (deterministic steps).
        sched_interval: "epoch" (what Lightning does with the reference's bare scheduler; `fit` calls `epoch_end()`) or "step"."""
        super().__init__(model, device, max_lr=max_lr, div_factor=div_factor, total_steps=total_steps, weight_decay=weight_decay, sched_interval=sched_interval)
        self.dims = (model._fc1[0].in_features, model.dim_hidden, model.n_classes)
        self.use_dropout = True if dropout is None else bool(dropout)
        Cd = self.dims[1]
        self._corr = torch.zeros(50, Cd, device=self.dev)
        self._w, self._w_keep = transmil_core._c_weights(self.p, Cd)          # (the reshapes inside are views of P: every tensor is contiguous)
        assert all(t.untyped_storage().data_ptr() == self.P.untyped_storage().data_ptr() for t in self._w_keep.values())
        self._gc = self._c_grads()

    def _c_grads(self) -> "_lib.TransMilGrads":
        g = lambda name: self.g(name).data_ptr()  # noqa: E731
        gc = _lib.TransMilGrads()
        gc.fc1_w, gc.fc1_b, gc.cls_token, gc.ppeg_corr = g("_fc1.0.weight"), g("_fc1.0.bias"), g("cls_token"), self._corr.data_ptr()
        gc.norm_w, gc.norm_b, gc.fc2_w, gc.fc2_b = g("norm.weight"), g("norm.bias"), g("_fc2.weight"), g("_fc2.bias")
        for i, nm in enumerate(("layer1", "layer2")):
            gc.layer[i] = _lib.TransMilLayerGrads(g(f"{nm}.norm.weight"), g(f"{nm}.norm.bias"), g(f"{nm}.attn.to_qkv.weight"), g(f"{nm}.attn.to_out.0.weight"),
                                                  g(f"{nm}.attn.to_out.0.bias"), g(f"{nm}.attn.res_conv.weight"))
        return gc

    def _check(self, bags: torch.Tensor) -> None:
        if not bags.is_cuda:
            raise RuntimeError("HipTransMilTrainer needs bags on the GPU (no CPU fallback)")
        if bags.shape[-1] != self.dims[0]:
            raise ValueError(f"bags must be [..., {self.dims[0]}], got {tuple(bags.shape)}")

    # ---- the head's part of `FlatTrainer.step` -------------------------------------------------------------------------------------------------------
    @property
    def dropout_live(self) -> bool:
        return self.use_dropout

    def _check_bags(self, bags: torch.Tensor) -> None:
        """bags [Bb, T, F] fp16 / bf16 / fp32 on the GPU (taken as they are: the forward converts while it reads)."""
        if bags.dim() != 3:
            raise ValueError(f"bags must be [batch, tile, {self.dims[0]}], got {tuple(bags.shape)}")
        self._check(bags)

    def _forward_train(self, bags, coords, seed):
        # (the class-row tail is resolved in there, once per step; the backward below reads the same `amds_transmil_cfg` out of `saved`)
        return transmil_core.forward_train(None, bags, self.dims, training=self.use_dropout, seed=seed, weights=(self._w, self._w_keep))

    def _backward(self, saved, dlogits) -> None:
        # the backward writes the views of G, then PPEG's six leave the correlation table in one launch
        transmil_core.backward(saved, dlogits, grads=self._gc)
        T.ppeg_grads_unpack(self._corr, *[self.g(k) for k in _PPEG])

    # ---- evaluation (validation / deploy): the inference forwards on the master weights themselves ------------------------------------------------------
    @torch.no_grad()
    def predict(self, bags: torch.Tensor, coords: torch.Tensor | None = None) -> torch.Tensor:
        """[Bb, T, F] -> logits [Bb, C]: `TransMIL.forward` in eval mode on the current `P` (amds_transmil_forward), bit for bit what `self.model.eval()` gives
        after `sync_to_model()`."""
        self._check(bags)
        return transmil_core.forward_infer(self._w, self.dims, bags)

    @torch.no_grad()
    def predict_ragged(self, bags, coords=None) -> torch.Tensor:
        """Bags of different lengths (a list of [T_i, F] tensors) in ONE library call -> logits [N, C], row i what the reference computes for bag i at batch 1
        (`TransMIL.forward_ragged`); grouping is the caller's (`group_valid_bags`)."""
        bags = list(bags)
        if not bags:
            return torch.empty(0, self.dims[2], dtype=torch.float32, device=self.dev)
        for b in bags:
            self._check(b)
        return transmil_core.forward_ragged(self._w, self.dims, bags)

    @torch.no_grad()
    def predict_infer_ragged(self, rb) -> torch.Tensor:
        """Bags that are already packed (`ResidentCohort.ragged_group`: a view of the resident store, used as it is) -> logits [n_bags, C] in ONE library call."""
        if rb.n_bags == 0:
            return torch.empty(0, self.dims[2], dtype=torch.float32, device=self.dev)
        self._check(rb.feats)
        return transmil_core.forward_infer_ragged(self._w, self.dims, rb)

    def group_valid_bags(self, lengths, per_call: int) -> list[tuple[int, int]]:
        """The hook of `mil_train.fit(valid_bags_per_call=)`: consecutive validation bags -> [start, end) groups by PADDED token rows
        (`transmil_core.group_bags_padded`, at most `valid_max_rows_per_call` rows and MAX_BAGS_PER_CALL bags a call)."""
        return transmil_core.group_bags_padded(lengths, self.dims[1], per_call, self.valid_max_rows_per_call)


__all__ = ["HipTransMilTrainer", "flat_layout"]
