"""`HipMlpTrainer`: training of `stamp_amd.mil.MLP` / `Linear` on slide- and patient-level feature vectors without autograd through the network -- the
`HipAbmilTrainer` of these heads.

One `step` = the reference's `LitSlideClassifier._step` (src/stamp/modeling/models/__init__.py:324-351; `LitSlideRegressor._step` with `losses.l1_loss`,
`LitSlideSurvival.training_step` with `losses.cox_survival_loss`; the `LitPatient*` wrappers are the same steps, :803-855) around amds_mlp_train_forward /
amds_mlp_train_backward (ONE library call each, csrc/mlp.hip), then AdamW under OneCycleLR (:133-141) as ONE fused launch (`amds_adamw`) with torch's own
schedule (`mil_train.OneCycleClock`).  `P`, `G`, `m`, `v`: one flat fp32 buffer each, the module's tensors back to back in `state_dict` order; the library's
weight and gradient structs are built ONCE over their views (no alignment is asked of a weight or gradient tensor), so there is nothing to refresh after a step.
Every product is exact fp32: no loss scale (`skipped_steps` 0, `current_loss_scale` 1.0).  `mil_train.fit` is the epoch loop; validation of batch-1 entries
(reference src/stamp/modeling/train.py:467-477) runs as ONE forward over the stacked rows with `fit(valid_bags_per_call=k)` -- a logits row does not depend on
what else is in the call (include/amdstamp.h), so the history is the one-row loop's.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib, mlp_core, ops
from . import train_ops as T
from .distributed import average_gradients
from .mil_train import OneCycleClock
from .transmil_train import flat_layout


class HipMlpTrainer:
    valid_max_rows_per_call = 262144          # rows one validation call may hold (`group_valid_bags`; the workspace scales with them)
    skipped_steps = 0
    current_loss_scale = 1.0

    def __init__(self, model, *, device="cuda", max_lr: float = 1e-4, div_factor: float = 25.0, total_steps: int = 1000, weight_decay: float = 0.01,
                 dropout: bool | None = None, sched_interval: str = "epoch") -> None:
        """model: `mil.MLP` or `mil.Linear`.  dropout: None = the module's rate after every hidden ReLU (train mode); False = off (deterministic steps)."""
        self.model = model
        self.dev = torch.device(device)
        self.dims = mlp_core.model_dims(model)          # (raises ValueError past the library's layer limit)
        rate = float(getattr(model, "dropout_p", 0.0))
        self.p_drop = rate if (dropout is None or dropout) and self.dims[3] > 1 else 0.0
        self.prefixes = [p for p, _ in mlp_core.linear_layers(model)]
        sd = model.state_dict()
        self.names = list(sd.keys())
        self.shapes = {k: tuple(v.shape) for k, v in sd.items()}
        self.offs, n = flat_layout(self.shapes)
        self.P = torch.cat([sd[k].detach().float().reshape(-1) for k in self.names]).to(self.dev).contiguous()
        self.G = torch.zeros(n, device=self.dev)
        self.m = torch.zeros(n, device=self.dev)
        self.v = torch.zeros(n, device=self.dev)
        self._pv = {k: self.P[o:o + c].view(self.shapes[k]) for k, (o, c) in self.offs.items()}
        self._gv = {k: self.G[o:o + c].view(self.shapes[k]) for k, (o, c) in self.offs.items()}
        self.step_count = 0
        self.wd = weight_decay
        self.clock = OneCycleClock(total_steps, max_lr, div_factor, sched_interval)
        self.train_pred_median = None
        if self.dev.type == "cuda":
            self._w, self._w_keep = mlp_core.weights_struct([self.p(f"{q}.weight") for q in self.prefixes], [self.p(f"{q}.bias") for q in self.prefixes])
            self._gc, self._g_keep = mlp_core.weights_struct([self.g(f"{q}.weight") for q in self.prefixes], [self.g(f"{q}.bias") for q in self.prefixes], _lib.MlpGrads)

    def p(self, name: str) -> torch.Tensor:
        return self._pv[name]

    def g(self, name: str) -> torch.Tensor:
        return self._gv[name]

    def sync_to_model(self) -> None:
        self.model.load_state_dict({k: self.p(k).detach().clone() for k in self.names})

    def load_from_model(self) -> None:
        sd = self.model.state_dict()
        self.P.copy_(torch.cat([sd[k].detach().float().reshape(-1) for k in self.names]).to(self.dev))

    def _refresh(self) -> None:
        """`fit` calls this after it restored `P`: the library reads `P` itself, there is no derived copy to rebuild."""

    def _rows(self, bags: torch.Tensor) -> torch.Tensor:
        """[B, F] as it is; [B, T, F] mean-pooled over the tiles first (mlp.py:40-41) by amds_mean_pool -> fp32 [B, F]."""
        if not bags.is_cuda:
            raise RuntimeError("HipMlpTrainer needs features on the GPU (no CPU fallback)")
        if bags.dim() not in (2, 3) or bags.shape[-1] != self.dims[0]:
            raise ValueError(f"features must be [batch, {self.dims[0]}] or [batch, tile, {self.dims[0]}], got {tuple(bags.shape)}")
        return ops.mean_pool(bags.contiguous()) if bags.dim() == 3 else bags

    def step(self, bags: torch.Tensor, targets: torch.Tensor, class_weights: torch.Tensor | None = None, *, update: bool = True, data_parallel: bool = False,
             coords: torch.Tensor | None = None, loss_fn=None, seed: int | None = None):
        """bags [B, F] (or [B, T, F]: pooled first) fp16 / fp32 on the GPU, targets as `loss_fn` wants them (default: float one-hot [B, C], the classifier's
        weighted cross-entropy; `losses.l1_loss`, `losses.cox_survival_loss` for regression / survival).  -> (loss, logits).  A batch whose loss has no gradient
        (a Cox batch without events) takes no step.  seed: this step's dropout seed (default: drawn from torch's CPU generator when dropout is live).  coords:
        accepted and ignored.  update=False computes loss, logits and gradients only."""
        x = self._rows(bags)
        dev = self.dev
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if self.p_drop > 0 else 0
        logits, saved = mlp_core.forward_train(self._w, self.dims, x, p=self.p_drop, seed=seed)
        with torch.enable_grad():
            lg = logits.detach().clone().requires_grad_(True)
            if loss_fn is None:
                loss = F.cross_entropy(lg, targets.to(dev, torch.float32), weight=None if class_weights is None else class_weights.to(dev, torch.float32))
            else:
                loss = loss_fn(lg, targets.to(dev))
            if not update and not loss.requires_grad:
                return loss.detach(), logits
            dlogits = torch.autograd.grad(loss, lg, allow_unused=True)[0] if loss.requires_grad else None
        if dlogits is None:
            return loss.detach(), logits
        mlp_core.backward(saved, dlogits, grads=self._gc)
        if data_parallel:
            average_gradients(self.G)
        if update:
            self.step_count += 1
            lr, b1 = self.clock.current()
            T.adamw(self.P, self.G, self.m, self.v, lr, self.step_count, betas=(b1, 0.999), weight_decay=self.wd)
            self.clock.after_step()
        return loss.detach(), logits

    def epoch_end(self) -> None:
        self.clock.epoch_end()

    @torch.no_grad()
    def predict(self, bags: torch.Tensor, coords: torch.Tensor | None = None) -> torch.Tensor:
        """[B, F] or [B, T, F] -> logits [B, C]: the eval forward on the current `P`, what `self.model.eval()` gives after `sync_to_model()`."""
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
