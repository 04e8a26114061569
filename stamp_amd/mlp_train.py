"""`HipMlpTrainer`: training of `stamp_amd.mil.MLP` / `Linear` on slide- and patient-level feature vectors without autograd through the network -- the
`flat_trainer.FlatTrainer` of these heads.

One `step` (`flat_trainer.py`: the flat `P` / `G` / `m` / `v` buffers, their views, the step protocol, the schedule) is the reference's
`LitSlideClassifier._step` (src/stamp/modeling/models/__init__.py:324-351; `LitSlideRegressor._step` with `losses.l1_loss`,
`LitSlideSurvival.training_step` with `losses.cox_survival_loss`; the `LitPatient*` wrappers are the same steps, :803-855) around amds_mlp_train_forward /
amds_mlp_train_backward (ONE library call each, csrc/mlp.hip).  The library's weight and gradient structs are built ONCE over the views (no alignment is
asked of a weight or gradient tensor), so there is nothing to refresh after a step.  Every product is exact fp32: no loss scale.  `mil_train.fit` is the
epoch loop; validation of batch-1 entries (reference src/stamp/modeling/train.py:467-477) runs as ONE forward over the stacked rows with
`fit(valid_bags_per_call=k)` -- a logits row does not depend on what else is in the call (include/amdstamp.h), so the history is the one-row loop's.
"""
from __future__ import annotations

import torch

from . import _lib, mlp_core, ops
from .flat_trainer import FlatTrainer


class HipMlpTrainer(FlatTrainer):
    valid_max_rows_per_call = 262144          # rows one validation call may hold (`group_valid_bags`; the workspace scales with them)

    def __init__(self, model, *, device="cuda", max_lr: float = 1e-4, div_factor: float = 25.0, total_steps: int = 1000, weight_decay: float = 0.01,
                 dropout: bool | None = None, sched_interval: str = "epoch") -> None:
        """model: `mil.MLP` or `mil.Linear`.  dropout: None = the module's rate after every hidden ReLU (train mode); False = off (deterministic steps)."""
        self.dims = mlp_core.model_dims(model)          # (raises ValueError past the library's layer limit)
        super().__init__(model, device, max_lr=max_lr, div_factor=div_factor, total_steps=total_steps, weight_decay=weight_decay, sched_interval=sched_interval)
        rate = float(getattr(model, "dropout_p", 0.0))
        self.p_drop = rate if (dropout is None or dropout) and self.dims[3] > 1 else 0.0
        self.prefixes = [p for p, _ in mlp_core.linear_layers(model)]
        if self.dev.type == "cuda":
            self._w, self._w_keep = mlp_core.weights_struct([self.p(f"{q}.weight") for q in self.prefixes], [self.p(f"{q}.bias") for q in self.prefixes])
            self._gc, self._g_keep = mlp_core.weights_struct([self.g(f"{q}.weight") for q in self.prefixes], [self.g(f"{q}.bias") for q in self.prefixes], _lib.MlpGrads)

    @property
    def dropout_live(self) -> bool:
        return self.p_drop > 0

    def _check_bags(self, bags: torch.Tensor) -> None:
        """[B, F] or [B, T, F] fp16 / fp32 on the GPU."""
        if not bags.is_cuda:
            raise RuntimeError("HipMlpTrainer needs features on the GPU (no CPU fallback)")
        if bags.dim() not in (2, 3) or bags.shape[-1] != self.dims[0]:
            raise ValueError(f"features must be [batch, {self.dims[0]}] or [batch, tile, {self.dims[0]}], got {tuple(bags.shape)}")

    @staticmethod
    def _rows(bags: torch.Tensor) -> torch.Tensor:
        """[B, F] as it is; [B, T, F] mean-pooled over the tiles first (mlp.py:40-41) by amds_mean_pool -> fp32 [B, F]."""
        return ops.mean_pool(bags.contiguous()) if bags.dim() == 3 else bags

    def _forward_train(self, bags, coords, seed):
        return mlp_core.forward_train(self._w, self.dims, self._rows(bags), p=self.p_drop, seed=seed)

    def _backward(self, saved, dlogits) -> None:
        mlp_core.backward(saved, dlogits, grads=self._gc)

    @torch.no_grad()
    def predict(self, bags: torch.Tensor, coords: torch.Tensor | None = None) -> torch.Tensor:
        """[B, F] or [B, T, F] -> logits [B, C]: the eval forward on the current `P`, what `self.model.eval()` gives after `sync_to_model()`."""
        self._check_bags(bags)
        return mlp_core.forward_infer(self._w, self.dims, self._rows(bags))

    @torch.no_grad()
    def predict_ragged(self, rows, coords=None) -> torch.Tensor:
        """A list of [F] rows (the entries of consecutive batch-1 validation batches) in ONE library call -> logits [N, C], row i bit-identical to
        `predict(rows[i][None])`; grouping is the caller's."""
        rows = list(rows)
        if not rows:
            return torch.empty(0, self.dims[2], dtype=torch.float32, device=self.dev)
        for r in rows:
            if r.dim() != 1 or r.shape[0] != self.dims[0]:
                raise ValueError(f"every entry must be [{self.dims[0]}], got {tuple(r.shape)}")
        return self.predict(torch.stack(rows))

    def group_valid_bags(self, lengths, per_call: int) -> list[tuple[int, int]]:
        """The hook of `mil_train.fit(valid_bags_per_call=)`: consecutive validation entries -> [start, end) groups by COUNT (an entry is one row whatever its
        width), at most `per_call` entries and `valid_max_rows_per_call` rows a call."""
        step = max(1, min(int(per_call), int(self.valid_max_rows_per_call)))
        n = len(list(lengths))
        return [(a, min(a + step, n)) for a in range(0, n, step)]


__all__ = ["HipMlpTrainer"]
