"""`FlatTrainer`: the host side every HIP-path trainer shares (`mil_train.HipMilVitTrainer`, `transmil_train.HipTransMilTrainer`, `abmil.HipAbmilTrainer`,
`mlp_train.HipMlpTrainer`).  No HIP in here: a head's library calls live in its own module.

What is flat, what is a view:
* `P`, `G`, `m`, `v` -- one fp32 buffer each (master parameters and buffers, gradients, Adam moments), the module's tensors back to back (`flat_layout`) in
  its `state_dict` order, or in `order` where a head's library wants another one.  `names` stays the `state_dict` order (checkpoints, `sync_to_model`).
* `p(name)` / `g(name)` are views of `P` / `G`, made once.  A head builds its library's weight and gradient structs once over them, so the library reads the
  master weights and writes every gradient where AdamW reads it; a head that keeps a derived copy rebuilds it in `_refresh`.

One `step` = the reference's `_step` (src/stamp/modeling/models/__init__.py:239-279) and its optimiser (:133-141), written once:
1. `_check_bags(bags)`;
2. the dropout seed, drawn from torch's CPU generator only when `dropout_live` and no `seed` is given -- before the forward, so a seeded run consumes the
   generator in one order;
3. `_forward_train(bags, coords, seed) -> (logits, saved)`;
4. the loss on the [batch, classes] logits, the one tiny piece left to torch (`task_loss`), and `dlogits` by autograd on a detached copy.  A loss without a
   gradient (a Cox batch without events, cox.py:219-224 returns a constant 0) ends the step here: nothing to learn from, no backward, no optimiser step.
   `step(objective="library")` takes both from ONE `amds_objective_step` launch instead, the head's loss scale folded in (`_dlogits_scale`);
5. `_backward(saved, _scale_dlogits(dlogits))`, which leaves every gradient in `G`;
6. `distributed.average_gradients(G)` when `data_parallel`;
7. `_apply(update)`: ONE fused AdamW launch (`amds_adamw`) on the `(lr, beta1)` of torch's own OneCycle schedule (`OneCycleClock`); nothing when `update` is
   false, so `P`, `m`, `v`, `step_count` and the schedule's position stay.

`mil_train.fit` is the epoch loop; it reads `skipped_steps` / `current_loss_scale` (fp32's range: 0 and 1.0 unless a head scales its loss) and calls
`epoch_end()` after every epoch and `_refresh()` after it restored `P`.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import train_ops as T
from .distributed import average_gradients


def flat_layout(shapes: dict) -> tuple[dict, int]:
    """name -> shape (in `state_dict` order) -> ({name: (offset, numel)}, total): the tensors back to back, in that order, in elements."""
    offs, n = {}, 0
    for k, s in shapes.items():
        offs[k] = (n, math.prod(s))
        n += offs[k][1]
    return offs, n


def onecycle_schedule(total_steps: int, max_lr: float, div_factor: float) -> tuple[list[float], list[float]]:
    """(lr, beta1) per optimiser step exactly as torch's OneCycleLR drives AdamW (reference models/__init__.py:133-141)."""
    dummy = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = torch.optim.lr_scheduler.OneCycleLR(dummy, total_steps=total_steps, max_lr=max_lr, div_factor=div_factor)
    lrs, b1s = [], []
    for i in range(total_steps):
        lrs.append(dummy.param_groups[0]["lr"])
        b1s.append(dummy.param_groups[0]["betas"][0])
        dummy.step()
        if i + 1 < total_steps:
            sched.step()
    return lrs, b1s


class OneCycleClock:
    """Position of a trainer on torch's OneCycle (lr, beta1) table.  interval "epoch": the position moves in `epoch_end()` only
    (what Lightning does with the reference's bare scheduler); "step": it moves after every optimiser step.  Past the table's end
    the last entry is held (torch's scheduler would raise; Lightning never gets there: max_epochs <= total_steps)."""

    def __init__(self, total_steps: int, max_lr: float, div_factor: float, interval: str = "epoch") -> None:
        if interval not in ("epoch", "step"):
            raise ValueError(f"sched_interval must be 'epoch' or 'step', got {interval!r}")
        self.interval = interval
        self.lrs, self.b1s = onecycle_schedule(total_steps, max_lr, div_factor)
        self.pos = 0

    def current(self) -> tuple[float, float]:
        i = min(self.pos, len(self.lrs) - 1)
        return self.lrs[i], self.b1s[i]

    def after_step(self) -> None:
        if self.interval == "step":
            self.pos += 1

    def epoch_end(self) -> None:
        if self.interval == "epoch":
            self.pos += 1


def task_loss(logits: torch.Tensor, targets: torch.Tensor, dev, class_weights, loss_fn) -> torch.Tensor:
    """loss_fn(logits, targets) -> scalar selects the task (`stamp_amd.losses`); None = the classifier's weighted cross-entropy with float one-hot targets
    (reference models/__init__.py:254-258)."""
    if loss_fn is None:
        return F.cross_entropy(logits, targets.to(dev, torch.float32), weight=None if class_weights is None else class_weights.to(dev, torch.float32))
    return loss_fn(logits, targets.to(dev))


OBJECTIVES = ("torch", "library")


def objective_kind(loss_fn) -> int:
    """`loss_fn` -> the library's objective (`train_ops.OBJ_*`): None = the classifier's weighted cross-entropy, `losses.l1_loss`,
    `losses.cox_survival_loss` (Efron), `losses.cox_slide_survival_loss` (Breslow).  Any other callable has no kernel: ValueError."""
    from . import losses
    kinds = {None: T.OBJ_CE, losses.l1_loss: T.OBJ_L1, losses.cox_survival_loss: T.OBJ_COX_EFRON, losses.cox_slide_survival_loss: T.OBJ_COX_BRESLOW}
    try:
        return kinds[loss_fn]
    except (KeyError, TypeError):
        raise ValueError(f"objective='library' takes loss_fn None (weighted cross-entropy), losses.l1_loss, losses.cox_survival_loss or "
                         f"losses.cox_slide_survival_loss, got {loss_fn!r}") from None


def check_objective(objective: str) -> str:
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be 'torch' or 'library', got {objective!r}")
    return objective


class FlatTrainer:
    # ---- the read-outs `fit` asks every trainer for: fp32's range, so no loss scale and no skipped step ----------------------------------------------
    skipped_steps = 0
    current_loss_scale = 1.0
    dropout_live = False          # a head with dropout sites overrides this: does a step without `seed` draw one?
    epoch_acc = None              # fp64 [2] on the device once a step ran with objective="library": sum(loss * batch), sum(batch) since `fit` zeroed it

    def __init__(self, model, device, *, max_lr: float, div_factor: float, total_steps: int, weight_decay: float, sched_interval: str,
                 order: list | None = None) -> None:
        """order: the names in the order the flat buffers hold them (default: the `state_dict`'s).
        sched_interval: "epoch" (what Lightning does with the reference's bare scheduler; `fit` calls `epoch_end()`) or "step"."""
        self.model = model
        self.dev = torch.device(device)
        sd = model.state_dict()
        self.names = list(sd.keys())
        self.shapes = {k: tuple(v.shape) for k, v in sd.items()}
        self.order = self.names if order is None else list(order)
        self.offs, n = flat_layout({k: self.shapes[k] for k in self.order})
        self.P = self._flat_state()
        self.G = torch.zeros(n, device=self.dev)
        self.m = torch.zeros(n, device=self.dev)
        self.v = torch.zeros(n, device=self.dev)
        self._pv = {k: self.P[o:o + c].view(self.shapes[k]) for k, (o, c) in self.offs.items()}
        self._gv = {k: self.G[o:o + c].view(self.shapes[k]) for k, (o, c) in self.offs.items()}
        self.step_count = 0
        self.wd = weight_decay
        self.clock = OneCycleClock(total_steps, max_lr, div_factor, sched_interval)
        self.train_pred_median = None

    def _flat_state(self) -> torch.Tensor:
        sd = self.model.state_dict()
        return torch.cat([sd[k].detach().float().reshape(-1) for k in self.order]).to(self.dev).contiguous()

    # ---- parameter views -------------------------------------------------------------------------------------------------------------------------------
    def p(self, name: str) -> torch.Tensor:
        return self._pv[name]

    def g(self, name: str) -> torch.Tensor:
        return self._gv[name]

    def sync_to_model(self) -> None:
        self.model.load_state_dict({k: self.p(k).detach().clone() for k in self.names})

    def load_from_model(self) -> None:
        self.P.copy_(self._flat_state())
        self._refresh()

    def _refresh(self) -> None:
        """Called whenever `P` changed under the head (`load_from_model`, `fit` after it restored `P`): a head whose library reads `P` itself has no derived
        copy to rebuild."""

    # ---- one optimisation step (module docstring) ------------------------------------------------------------------------------------------------------
    def step(self, bags: torch.Tensor, targets: torch.Tensor, class_weights: torch.Tensor | None = None, *, update: bool = True,
             data_parallel: bool = False, coords: torch.Tensor | None = None, loss_fn=None, seed: int | None = None, objective: str = "torch"):
        """bags on the GPU as the head takes them, targets as `loss_fn` wants them (default: float one-hot [batch, classes], the classifier's weighted
        cross-entropy; `losses.l1_loss`, `losses.cox_survival_loss` for regression / survival).  -> (loss, logits).  A batch whose loss has no gradient takes
        no step.  seed: this step's dropout seed (default: drawn from torch's CPU generator when dropout is live).  coords: accepted, and ignored by every head
        without a positional term.  data_parallel=True: every rank of the initialised process group holds a replica and its own bags; the flat gradient is
        averaged with ONE all-reduce before AdamW.  update=False computes loss, logits and gradients and leaves `P`, `m`, `v`, `step_count` and the schedule's
        position as they were.
        objective="library": loss and dlogits come from ONE `amds_objective_step` launch (`objective_kind(loss_fn)` names the kernel; the head's loss scale is
        folded into it) instead of torch's loss and autograd.  The loss is a 0-d device tensor and, for cross-entropy and L1, the step reads nothing back;
        the two Cox kinds read the 4-byte `has_grad` (where the torch path reads `event.sum()`) and a batch without an event takes no step.  The launch also
        adds loss * batch and batch to `self.epoch_acc` (fp64 [2] on the device), which `fit` reads once per epoch."""
        check_objective(objective)
        kind = objective_kind(loss_fn) if objective == "library" else None
        self._check_bags(bags)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if self.dropout_live else 0
        logits, saved = self._forward_train(bags, coords, seed)
        if kind is not None:
            scale, scale_dev = self._dlogits_scale()
            if self.epoch_acc is None:
                self.epoch_acc = torch.zeros(2, dtype=torch.float64, device=self.dev)
            loss, dlogits, has_grad = T.objective_step(kind, logits.detach().float(), targets.to(self.dev, torch.float32),
                                                       None if class_weights is None or kind != T.OBJ_CE else class_weights.to(self.dev, torch.float32),
                                                       scale=scale, scale_dev=scale_dev, epoch_acc=self.epoch_acc)
            if kind in (T.OBJ_COX_EFRON, T.OBJ_COX_BRESLOW) and int(has_grad.item()) == 0:
                return loss, logits
            self._backward(saved, dlogits)
            if data_parallel:
                average_gradients(self.G)
            self._apply(update)
            return loss, logits
        with torch.enable_grad():
            lg = logits.detach().clone().requires_grad_(True)
            loss = task_loss(lg, targets, self.dev, class_weights, loss_fn)
            if not update and not loss.requires_grad:
                return loss.detach(), logits
            dlogits = torch.autograd.grad(loss, lg, allow_unused=True)[0] if loss.requires_grad else None
        if dlogits is None:
            return loss.detach(), logits
        self._backward(saved, self._scale_dlogits(dlogits))
        if data_parallel:
            average_gradients(self.G)
        self._apply(update)
        return loss.detach(), logits

    def _check_bags(self, bags: torch.Tensor) -> None:
        """Raises on input the head's forward must not see."""

    def _forward_train(self, bags: torch.Tensor, coords, seed: int):
        """-> (logits [batch, classes], whatever `_backward` needs)."""
        raise NotImplementedError

    def _backward(self, saved, dlogits: torch.Tensor) -> None:
        """Every parameter gradient of the step into `G`."""
        raise NotImplementedError

    def _scale_dlogits(self, dlogits: torch.Tensor) -> torch.Tensor:
        return dlogits

    def _dlogits_scale(self) -> tuple[float, torch.Tensor | None]:
        """`_scale_dlogits` as the (host factor, 0-d device factor or None) that `amds_objective_step` multiplies into dlogits itself."""
        return 1.0, None

    def _apply(self, update: bool) -> None:
        if update:
            self.step_count += 1
            lr, b1 = self.clock.current()
            T.adamw(self.P, self.G, self.m, self.v, lr, self.step_count, betas=(b1, 0.999), weight_decay=self.wd)
            self.clock.after_step()

    def epoch_end(self) -> None:
        """Lightning steps an epoch-interval scheduler once after every training epoch."""
        self.clock.epoch_end()


__all__ = ["FlatTrainer", "OneCycleClock", "flat_layout", "onecycle_schedule", "task_loss", "objective_kind", "check_objective", "OBJECTIVES"]
