"""Training of the MIL `vit` head on the HIP path: one optimisation step (forward + backward + AdamW, no autograd through the
network) and the epoch loop around it.  The flat `P` / `G` / `m` / `v` buffers, their views, the step protocol and the schedule's clock are
`flat_trainer.FlatTrainer`'s (described there, once); this head adds its 16-bit operands and loss scale, the ALiBi buffers and the packed operand copy.

Mirrors what `stamp train` does for tile-level models:
* per batch -- reference src/stamp/modeling/models/__init__.py:239-279 (`LitTileClassifier._step`: ``logits = self.model(bags,
  coords=coords, mask=None)``, the cross-entropy of the logits against float one-hot targets under `class_weights`: `flat_trainer.task_loss`), :444-483 (L1), :751-776
  (Cox); train mode, i.e. WITH the reference's dropout sites (`dropout` on project_features and inside nn.MultiheadAttention, the
  hard-coded 0.5 on both feed-forward Dropouts, vision_tranformer.py:157-169 / 268-271) and with every ALiBi `_RunningMeanScaler`
  updated before use (:24-29);
* optimiser -- :133-141: ``AdamW(lr=1e-3)`` with torch defaults wrapped in ``OneCycleLR(total_steps, max_lr, div_factor)``.  torch's
  OneCycleLR also cycles AdamW's beta1 (cycle_momentum=True: 0.95 -> 0.85 at the LR peak -> 0.95); both the LR and beta1 are read
  off torch's own scheduler evaluated on a dummy optimiser and fed to the fused kernel.  HOW OFTEN the schedule advances is not
  STAMP's decision: `configure_optimizers` returns a bare ``[optimizer], [scheduler]`` pair, and Lightning wraps an un-annotated
  scheduler in its default config ``interval="epoch", frequency=1`` -- so under `stamp train` the schedule, although sized in STEPS
  (``total_steps = len(train_dl) * max_epochs``, train.py:197-198), moves ONE position per EPOCH and the learning rate stays on the
  first ``max_epochs`` positions of the warm-up ramp.  `sched_interval="epoch"` (the default here) reproduces that;
  `sched_interval="step"` is the per-step OneCycle the schedule's size suggests was intended;
* epochs -- src/stamp/modeling/train.py:504-564: validation after every epoch (the caller's validation loader: full bags,
  batch size 1, :467-477), early stopping with `patience` on the validation loss (mode min), the best epoch's weights restored
  at the end (`shutil.copy(best_model_path)` + reload).  Survival runs are monitored on `val_cindex`, mode max, instead (train.py:521-540):
  `fit(monitor="val_cindex")`, computed over the whole validation set by `stamp_amd.metrics`.

Mixed precision (stated, not hidden): 16-bit MFMA operands for activations, weights and gradients, fp32 accumulation, fp32 residual
stream and its gradient, fp32 LayerNorm / softmax statistics, fp32 master weights, gradients and Adam moments.  WHICH 16-bit type
follows torch's own flag, like the TransMIL head's products do: the reference calls `torch.set_float32_matmul_precision("high")` before
training (src/stamp/modeling/train.py:519) -- TF32-class products, 10 explicit mantissa bits per operand -- so under "high" (and
"highest") the operands are **fp16** (10 explicit bits, like TF32) and the loss is scaled by 2^10 on its way into the backward
(fp16's exponent range; the fp32 gradients are un-scaled before AdamW); under "medium" (bf16 products in torch's own wording) they are
**bf16** (8 bits, fp32's exponent range, no loss scaling) -- the only mode before round 6.  `precision=` overrides the flag.
fp16's range is finite, and one inf / NaN gradient would enter P, m and v through AdamW for good (the reference's TF32 products have fp32's
range and cannot fail so).  So the fp16 scale is DYNAMIC by default, as torch's GradScaler: a device-resident state
(`amds_loss_scale_state`) whose scale multiplies dlogits as a 0-d tensor; the un-scaling pass over the flat gradient also counts its
non-finite values (`amds_grad_unscale_check`, replacing the plain multiply); AdamW is skipped ON THE DEVICE when the count is non-zero
(`amds_adamw_guarded`: no write to P, m, v; bias corrections by applied steps, as torch's AdamW under GradScaler); a one-lane launch then
halves the scale (floored at `min_loss_scale`) or doubles it after `scale_growth_interval` clean steps, capped at `loss_scale` -- so a
run that never overflows keeps 2^10 and the static scale's bits exactly.  No host synchronisation inside a step; `skipped_steps` and
`current_loss_scale` read the state when asked, `fit` records the skipped steps per epoch.  `dynamic_loss_scale=False`: the static scale.
The loss on the [batch, classes] logits is the one tiny piece left to torch by default; `step(objective="library")` / `fit(objective="library")`
take it from amds_objective_step / amds_objective_rows instead, with this head's loss scale folded into the launch (`_dlogits_scale`).
"""
from __future__ import annotations

import math
from typing import TYPE_CHECKING

import torch

from . import losses, metrics, mil_core
from . import train_ops as T
from .distributed import average_buffers
from .flat_trainer import FlatTrainer, OneCycleClock, check_objective, objective_kind, onecycle_schedule, task_loss  # noqa: F401  (the schedule names stay importable from here)
from .mil import VisionTransformer
from .mil_core import PackedVit

if TYPE_CHECKING:
    from .transmil_train import HipTransMilTrainer

BF = torch.bfloat16


class HipMilVitTrainer(FlatTrainer):
    def __init__(self, model: VisionTransformer, *, device="cuda", max_lr: float = 1e-4, div_factor: float = 25.0,
                 total_steps: int = 1000, weight_decay: float = 0.01, split_k: int = 32, dropout: bool | None = None,
                 sched_interval: str = "epoch", precision: str | None = None, loss_scale: float = 1024.0, dynamic_loss_scale: bool = True,
                 scale_growth_interval: int = 2000, min_loss_scale: float = 1.0) -> None:
        """dropout: None = as the reference's train mode (live when the model's rates are > 0; the feed-forward rate is always 0.5);
        False = all dropout sites off (deterministic steps, e.g. for parity tests against autograd).
        sched_interval: "epoch" (default; what Lightning does with the reference's bare scheduler, see the module docstring: call
        `epoch_end()` after every epoch -- `fit` does) or "step" (OneCycle advanced after every optimiser step).
        precision: None = torch.get_float32_matmul_precision() at construction ("high" under the reference's train_model_, train.py:519); "high" /
        "highest" -> fp16 operands + loss scale `loss_scale`; "medium" -> bf16 operands, no scaling (module docstring).
        dynamic_loss_scale (fp16 only): `loss_scale` is the initial scale and the cap; a step with a non-finite gradient is skipped on the device
        and the scale halved (not below `min_loss_scale`); `scale_growth_interval` clean steps double it.  False = the static scale, unchecked."""
        self.precision = precision or torch.get_float32_matmul_precision()
        if self.precision not in ("medium", "high", "highest"):
            raise ValueError(f"precision must be 'medium', 'high' or 'highest', got {self.precision!r}")
        self.act = BF if self.precision == "medium" else torch.float16
        # fp16 gradients: a static power-of-two scale on dlogits (exact) lifts the 16-bit gradient tensors out of fp16's subnormal range; un-scaled in fp32
        self.loss_scale = 1.0 if self.act == BF else float(loss_scale)
        self._ls = None                  # the device-resident loss-scale state (train_ops.loss_scale_state), fp16 + dynamic only
        self.dims = model.dims
        self.alibi = bool(model.use_alibi)
        if torch.device(device).type != "cuda":
            raise RuntimeError("HipMilVitTrainer runs on the GPU only")
        self.use_dropout = True if dropout is None else bool(dropout)
        self.split_k = split_k
        # order inside the flat buffers: ALiBi's per-head tensors stacked (mil_core.flat_order); `names` stays the reference's state_dict order
        super().__init__(model, device, max_lr=max_lr, div_factor=div_factor, total_steps=total_steps, weight_decay=weight_decay, sched_interval=sched_interval,
                         order=mil_core.flat_order(self.dims, list(model.state_dict().keys())))
        # ALiBi: running_mean / items_so_far are BUFFERS of the reference module (no gradient, no optimiser update)
        stat = [k for k in self.names if mil_core.is_buffer(k)]
        self._stat_idx = torch.tensor([self.offs[k][0] for k in stat], dtype=torch.long, device=self.dev)
        self._dist_on = False
        self._eval_pk, self._eval_pk_step = None, -1
        self.pk = PackedVit(self.dims, self.p, self.act, train=True)
        if dynamic_loss_scale and self.act != BF:
            self._ls = T.loss_scale_state(self.dev, self.loss_scale, growth_interval=scale_growth_interval, min_scale=min_loss_scale)
            self._ls_scale = T.loss_scale_of(self._ls)

    # ---- loss-scale read-outs (each synchronises when read; nothing inside a step does) ------------------------------------------------
    @property
    def skipped_steps(self) -> int:
        """Optimiser steps skipped so far because a gradient was not finite (0 without a dynamic scale)."""
        return 0 if self._ls is None else int(self._ls[T.LS_SKIPPED].item())

    @property
    def current_loss_scale(self) -> float:
        return self.loss_scale if self._ls is None else float(T.loss_scale_of(self._ls).item())

    @property
    def dropout_live(self) -> bool:
        return self.use_dropout

    # ---- one optimisation step: `FlatTrainer.step` with this head's loss scale and ALiBi buffers -----------------------------------------------
    def step(self, bags: torch.Tensor, targets: torch.Tensor, class_weights: torch.Tensor | None = None, *, update: bool = True,
             data_parallel: bool = False, coords: torch.Tensor | None = None, loss_fn=None, seed: int | None = None, objective: str = "torch"):
        """bags [Bb,T,F] fp16/bf16/fp32 on the GPU, targets float one-hot [Bb,C]. Returns (loss, logits).  The arguments are `FlatTrainer.step`'s; the flat
        fp32 gradient buffer (14.7 MB for the default head) is averaged with ONE RCCL all-reduce before AdamW (the reference itself is
        single-device, src/stamp/modeling/train.py:541-547).

        update=False computes loss, logits and gradients and leaves EVERY piece of state as it was: no optimiser step, and the ALiBi
        running-mean buffers (which a train-mode forward updates before use, vision_tranformer.py:24-29) are put back afterwards.  (With a
        dynamic loss scale the gradients are un-scaled and checked; scale and counters stay.)

        A step the dynamic loss scale skips (non-finite gradient) still advances the OneCycle clock (torch's scheduler under GradScaler),
        keeps the forward's ALiBi running-mean update (as the reference module would) and returns its loss and logits."""
        self._dist_on = data_parallel and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        kw = dict(update=update, data_parallel=data_parallel, coords=coords, loss_fn=loss_fn, seed=seed, objective=objective)
        if update or not self.alibi:
            return super().step(bags, targets, class_weights, **kw)
        stats_before = self.P[self._stat_idx].clone()
        try:
            return super().step(bags, targets, class_weights, **kw)
        finally:
            self.P[self._stat_idx] = stats_before
            self._refresh()

    def _forward_train(self, bags, coords, seed):
        if self.alibi:
            if coords is None:
                raise ValueError("use_alibi=True needs coords")
            cc = mil_core._coords_with_cls(coords, bags.shape[0], self.dev)
            mil_core.update_running_means(self.p, self.dims, cc)
            if self._dist_on:      # replicas see different bags: keep the scaler buffers identical (mean of the ranks' updates)
                self.P[self._stat_idx] = average_buffers(self.P[self._stat_idx])
            self._refresh()
        return mil_core.forward_train(self.pk, bags, coords, training=self.use_dropout, seed=seed)

    def _scale_dlogits(self, dlogits):
        if self._ls is not None:
            return dlogits * self._ls_scale          # 0-d device tensor: no synchronisation
        return dlogits * self.loss_scale if self.loss_scale != 1.0 else dlogits

    def _dlogits_scale(self):
        return (1.0, self._ls_scale) if self._ls is not None else (self.loss_scale, None)

    def _backward(self, saved, dlogits) -> None:
        G, _ = mil_core.backward(self.pk, saved, dlogits, need_params=True, need_bags=False, split_k=self.split_k, grad_views=self.g)
        grouped = self._copy_grouped_grads(G) if self.alibi else ()
        for k, gk in G.items():          # (unpadded geometries: the library wrote into the flat buffer's views themselves -- nothing to copy)
            if k not in grouped and gk.data_ptr() != self.g(k).data_ptr():
                self.g(k).copy_(gk)
        if self._ls is None and self.loss_scale != 1.0:
            self.G.mul_(1.0 / self.loss_scale)

    def _apply(self, update: bool) -> None:
        """(The gradient was averaged over the ranks before this: with a dynamic scale every rank counts the same values and takes the same decision.)"""
        if self._ls is not None:
            T.grad_unscale_check(self.G, self._ls)
        if not update:
            if self._ls is not None:
                T.loss_scale_update(self._ls, apply=False)
            return
        stats = self.P[self._stat_idx].clone() if self.alibi else None      # buffers: not touched by the optimiser (weight decay)
        if self._ls is None:
            super()._apply(True)
        else:
            self.step_count += 1
            lr, b1 = self.clock.current()
            T.adamw_guarded(self.P, self.G, self.m, self.v, lr, self.step_count, self._ls, betas=(b1, 0.999), weight_decay=self.wd)
            T.loss_scale_update(self._ls, apply=True)
            self.clock.after_step()
        if stats is not None:
            self.P[self._stat_idx] = stats
        self._refresh()

    def _copy_grouped_grads(self, G: dict) -> set:
        """ALiBi: the per-head Linears are 3 x H weights + 3 x H biases + H bias scales per layer -- separate tensors in the reference's state_dict, equally
        pitched slices both of the library's packed gradient and of this trainer's flat buffer.  One strided copy per group instead of one launch per
        tensor (~110 per layer and step, which the GPU then waited for).  -> the names served."""
        d, done = self.dims, set()
        first = mil_core.layer_prefix(0) + f"0.mhsa.{mil_core._ENC[0]}.0.weight"
        if G[first].data_ptr() == self.g(first).data_ptr():
            return done                  # (the library wrote into the flat buffer itself: mil_core._direct_grad_structs)
        for l in range(d.L):
            p = mil_core.layer_prefix(l)
            groups = [[[p + f"0.mhsa.{e}.{h}.{kind}" for h in range(d.H)] for e in mil_core._ENC] for kind in ("weight", "bias")]
            groups.append([[p + f"0.mhsa.attentions.{h}.bias_scale" for h in range(d.H)]])
            for grp in groups:
                dst = mil_core._stack([mil_core._stack([self.g(n) for n in row]) for row in grp])
                if dst.untyped_storage().data_ptr() != self.G.untyped_storage().data_ptr():
                    continue             # (not a view of the flat buffer: the per-tensor loop serves these)
                dst.copy_(mil_core._stack([mil_core._stack([G[n] for n in row]) for row in grp]))
                done.update(n for row in grp for n in row)
        return done

    def _refresh(self) -> None:
        """The packed operands follow the master parameters; any cached inference pack is stale from here on."""
        self.pk.refresh(self.p)
        self._eval_pk_step = -1

    # ---- evaluation (validation / deploy): inference kernels, fp16 operands, any bag length ---------------------------------------------
    def _eval_pack(self) -> PackedVit:
        # the fp16 inference pack is rebuilt whenever the master parameters or buffers changed since it was made (`_refresh`)
        if self._eval_pk_step != self.step_count or self._eval_pk is None:
            self._eval_pk = PackedVit(self.dims, self.p, torch.float16, train=False)
            self._eval_pk_step = self.step_count
        return self._eval_pk

    @torch.no_grad()
    def predict(self, bags: torch.Tensor, coords: torch.Tensor | None = None) -> torch.Tensor:
        return mil_core.forward_infer(self._eval_pack(), bags, coords, None)

    @torch.no_grad()
    def predict_ragged(self, bags, coords=None) -> torch.Tensor:
        """Bags of different lengths (a list of [T_i, F] tensors, coords a list of [T_i, 2] or None) in ONE library call -> logits [N, C]; row i equals
        `predict(bags[i][None], coords[i][None])` bit for bit (mil_core.forward_ragged: a bag longer than `max_shared_tiles()` runs alone)."""
        bags = list(bags)
        if not bags:
            return torch.empty(0, self.dims.C, dtype=torch.float32, device=self.dev)
        return mil_core.forward_ragged(self._eval_pack(), bags, coords, device=self.dev)

    def max_shared_tiles(self) -> int:
        return mil_core.max_shared_tiles(self._eval_pack())


def _validate_ragged(trainer, valid_batches, dev, class_weights, loss_fn, per_call: int, keep: list | None = None, with_loss: bool = True) -> tuple[float, int]:
    """The validation sum of `fit` with consecutive one-bag batches run `per_call` at a time through `predict_ragged` (mil_core.group_bags decides the
    groups, or the trainer's `group_valid_bags(lengths, per_call) -> [(start, end)]` if it has one): each batch's loss comes from its own logits row(s) exactly as in the one-bag loop, the group's losses reach the host in one read, and the
    sum runs in batch order.  Batches of several bags keep the one-call `predict` of the default loop.
    keep: a list that receives every batch's (logits, targets) in batch order, both left on the device; with_loss=False: no per-batch loss and no host read."""
    vtot, vcnt = 0.0, 0
    pend: list = []

    def flush():
        nonlocal vtot, vcnt
        if not pend:
            return
        one = [i for i, (b, *_rest) in enumerate(pend) if b.shape[0] == 1]
        rows: dict = {}
        if one:
            lens = [pend[i][0].shape[1] for i in one]
            if hasattr(trainer, "group_valid_bags"):          # the trainer's own grouping rule (TransMIL: by padded token rows)
                groups = trainer.group_valid_bags(lens, per_call)
            else:
                limit = trainer.max_shared_tiles() if hasattr(trainer, "max_shared_tiles") else mil_core.MAX_SOLO_TILES
                groups = mil_core.group_bags(lens, per_call, 1 << 62, limit)
            for a, e in groups:
                idx = one[a:e]
                cs = None if pend[idx[0]][1] is None else [pend[i][1][0].to(dev) for i in idx]
                lg = trainer.predict_ragged([pend[i][0][0].to(dev) for i in idx], cs)
                for k, i in enumerate(idx):
                    rows[i] = lg[k:k + 1]
        losses = []
        for i, (bags, coords, targets) in enumerate(pend):
            lg = rows[i] if i in rows else trainer.predict(bags.to(dev), None if coords is None else coords.to(dev))
            if keep is not None:
                keep.append((lg, targets.to(dev)))
            if with_loss:
                losses.append(task_loss(lg, targets, dev, class_weights, loss_fn).reshape(()))
        for (bags, _c, _t), v in zip(pend, torch.stack(losses).tolist() if losses else ()):
            vtot += float(v) * bags.shape[0]
            vcnt += bags.shape[0]
        pend.clear()

    for bags, coords, _sizes, targets in valid_batches():
        pend.append((bags, coords, targets))
        if sum(b.shape[0] for b, *_ in pend) >= per_call:
            flush()
    flush()
    return vtot, vcnt


def _rows_loss_sum(kept: list, dev, class_weights, loss_fn) -> tuple[float, int]:
    """The validation sum of `fit(objective="library")`: the kept (logits, targets) of every batch -> one concatenation, ONE `amds_objective_rows` launch,
    ONE host read of the row losses, added in batch order in Python doubles."""
    kind = objective_kind(loss_fn)
    lg = torch.cat([l.float().reshape(l.shape[0], -1) for l, _ in kept])
    y = torch.cat([t.to(dev, torch.float32).reshape(t.shape[0], -1) for _, t in kept])
    w = None if class_weights is None or kind != T.OBJ_CE else class_weights.to(dev, torch.float32)
    vtot = 0.0
    for v in T.objective_rows(kind, lg, y, w).tolist():
        vtot += v
    return vtot, lg.shape[0]


def _validate_block(trainer, valid_batches, per_call: int, keep: list) -> None:
    """Validation entries that are already one tensor (`valid_batches.block()`): `predict` on slices of the trainer's `group_valid_bags` size (or of `per_call`
    rows), no per-entry view; keep receives each slice's (logits, targets)."""
    feats, targets = valid_batches.block()
    N = feats.shape[0]
    groups = trainer.group_valid_bags([feats.shape[1]] * N, per_call) if hasattr(trainer, "group_valid_bags") else \
        [(a, min(a + per_call, N)) for a in range(0, N, per_call)]
    for a, e in groups:
        keep.append((trainer.predict(feats[a:e]), targets[a:e]))


def fit(trainer: "HipMilVitTrainer | HipTransMilTrainer", train_batches, valid_batches, *, max_epochs: int, patience: int = 16, class_weights=None,
        loss_fn=None, log=None, valid_bags_per_call: int = 1, monitor: str = "validation_loss", valid_auroc: bool = False,
        valid_auprc: bool = False, objective: str = "torch") -> dict:
    """The epoch loop of the reference's `train_model_` (src/stamp/modeling/train.py:504-564) around `HipMilVitTrainer.step` or
    `transmil_train.HipTransMilTrainer.step` (any object with their step / predict / predict_ragged / epoch_end / P drives it).

    train_batches / valid_batches: callables returning an iterable of (bags, coords, bag_sizes, targets) per epoch -- the
    reference's loaders (train: fixed-size bags, batch 64, shuffled; validation: full bags, batch 1, `bag_size=None`, train.py:455-477).
    After every epoch the validation loss (same objective, eval mode: no dropout, frozen scalers; Lightning's mean over batches
    weighted by batch size) is computed; training stops when it has not improved for `patience` epochs (EarlyStopping, mode min);
    the best epoch's weights are restored and copied into `trainer.model` (the reference copies the best checkpoint and reloads
    it).  `num_sanity_val_steps=0` like the reference.  Returns the history; `skipped_steps` holds the optimiser steps per epoch the dynamic
    loss scale skipped (fp16 gradients not finite), and `log` is warned about each epoch that skipped any.
    valid_bags_per_call > 1: consecutive one-bag validation batches run that many at a time through ONE ragged call (`predict_ragged`), with one host
    read of their losses per call instead of one per bag; the losses, and so the history and the restored epoch, are those of the default loop.

    monitor="val_cindex" -- what the reference monitors for EVERY survival run, mode max, for early stopping and for the kept checkpoint (train.py:521-540);
    targets are [time, event], dim_output 1.  The per-batch validation loss is not evaluated (on the reference's one-bag validation batches the Cox partial
    likelihood is the score minus the log-sum-exp over that same score: the same value every epoch).  Instead every validation bag's score
    (``logits.squeeze(-1)``), time and event stay on the device -- through the one-bag loop, batches of several bags and the ragged path alike, no host read per
    bag -- and after the epoch, as `LitSurvivalBase.on_validation_epoch_end` (models/__init__.py:696-715) does over the WHOLE validation set:
    ``val_cox_loss = losses.cox_breslow_loss(all)`` and ``val_cindex = metrics.concordance_index(all)`` (exact pair counts, amds_concordance_counts).  The
    history gains both lists and `validation_loss` holds val_cox_loss.  An epoch improves when its val_cindex is STRICTLY greater (Lightning's `torch.gt` at
    min_delta 0: the first maximum wins); `patience` counts from the best epoch.  A validation set without any event raises RuntimeError (the reference logs
    nothing there and Lightning's EarlyStopping raises on the missing val_cindex).  A non-finite val_cindex ends the loop at that epoch (EarlyStopping's
    check_finite) and the best finite epoch is restored; if no epoch had a finite value the weights of the last trained epoch stay.  Also, as
    `on_train_epoch_end` (:717-728): `train_pred_median` = torch.median over all training-step scores of the epoch (kept on the device, concatenated once per
    epoch) goes into hist["train_pred_median"] and, the last epoch's, into `trainer.train_pred_median` -- the cut-off `deploy.to_survival_prediction_df(cut_off=)`
    takes.  WHICH epoch's median Lightning writes into the kept checkpoint is not reproduced: the history has them all.

    valid_auroc=True (classification, loss_fn=None): hist["validation_auroc"] holds, per epoch, the mean one-vs-rest AUROC
    ``metrics.multiclass_auroc(softmax(logits), argmax(targets))`` over the validation set (the reference logs it for every classification run,
    models/__init__.py:217, 270-277); selection is unchanged.
    valid_auprc=True (same conditions): hist["validation_auprc"] holds, per epoch, the mean one-vs-rest average precision
    ``metrics.multiclass_auprc(softmax(logits), argmax(targets))`` over the whole validation set (amds_binary_curves), from the same kept logits as
    valid_auroc; selection is unchanged, and with the flag off neither the history nor a bit of the run changes.

    objective="library" (`FlatTrainer` heads; default "torch": today's calls and bits): every training step takes loss and dlogits from ONE
    `amds_objective_step` launch and `fit` reads no loss per step -- the launches add into `trainer.epoch_acc`, zeroed before an epoch and read once after it:
    train_loss = acc[0] / acc[1].  Under monitor="validation_loss" every validation batch's logits stay on the device; after the last batch ONE
    `amds_objective_rows` launch gives the loss of every row as a batch of its own, ONE read brings them to the host, and the host adds them in batch order
    in Python doubles (a batch of B bags contributes its B rows: its mean times B).  A row's value depends on that row alone, so the history under
    valid_bags_per_call = k IS the history under 1, float for float, for every trainer.  A `valid_batches` callable with a `block()` method
    (`FeatureTableView.valid_batches`) is, under valid_bags_per_call > 1, not iterated: `block()` hands over (feats [N, F], targets [N, D]) as one gather and
    `predict` runs on `group_valid_bags`-sized slices of it.  The Cox kinds have no per-row value (a one-bag Cox batch is a constant): they need
    monitor="val_cindex", whose whole-set Breslow value stays in torch."""
    check_objective(objective)
    library = objective == "library"
    if library and objective_kind(loss_fn) in (T.OBJ_COX_EFRON, T.OBJ_COX_BRESLOW) and monitor != "val_cindex":
        raise ValueError("objective='library' with a Cox loss_fn needs monitor='val_cindex' (a one-bag Cox validation batch is a constant)")
    if valid_bags_per_call < 1:
        raise ValueError("valid_bags_per_call must be >= 1")
    if monitor not in ("validation_loss", "val_cindex"):
        raise ValueError(f"monitor must be 'validation_loss' or 'val_cindex', got {monitor!r}")
    if valid_auroc and (loss_fn is not None or monitor != "validation_loss"):
        raise ValueError("valid_auroc=True applies to classification: loss_fn=None, monitor='validation_loss'")
    if valid_auprc and (loss_fn is not None or monitor != "validation_loss"):
        raise ValueError("valid_auprc=True applies to classification: loss_fn=None, monitor='validation_loss'")
    cindex = monitor == "val_cindex"
    dev = trainer.dev
    best = {"loss": float("-inf") if cindex else float("inf"), "epoch": -1, "P": None}
    hist = {"train_loss": [], "validation_loss": [], "skipped_steps": [], "best_epoch": -1, "stopped_epoch": None}
    if cindex:
        hist.update(val_cox_loss=[], val_cindex=[], train_pred_median=[])
    if valid_auroc:
        hist["validation_auroc"] = []
    if valid_auprc:
        hist["validation_auprc"] = []
    wait = 0
    skipped = getattr(trainer, "skipped_steps", 0)          # (any object with the trainer's step / predict / epoch_end drives this loop)
    step_kw = {"objective": objective} if library else {}
    rows_loss = library and not cindex                      # validation losses from one amds_objective_rows launch
    for epoch in range(max_epochs):
        tot, cnt, steps = 0.0, 0, 0
        train_scores = []
        if library and trainer.epoch_acc is not None:
            trainer.epoch_acc.zero_()
        for bags, coords, _sizes, targets in train_batches():
            loss, step_logits = trainer.step(bags.to(dev), targets, class_weights, coords=None if coords is None else coords.to(dev), loss_fn=loss_fn,
                                             **step_kw)
            if cindex:
                train_scores.append(step_logits.detach().reshape(-1))
            if not library:
                tot += float(loss) * bags.shape[0]
                cnt += bags.shape[0]
            steps += 1
        if library and steps:          # the epoch's one read: what every step's launch added
            tot, cnt = trainer.epoch_acc.tolist()
        trainer.epoch_end()
        hist["train_loss"].append(tot / max(cnt, 1))
        if cindex and train_scores:
            trainer.train_pred_median = float(torch.cat(train_scores).median())
            hist["train_pred_median"].append(trainer.train_pred_median)
        now = getattr(trainer, "skipped_steps", 0)
        hist["skipped_steps"].append(now - skipped)
        if log and now > skipped:
            log(f"warning: epoch {epoch}: {now - skipped} of {steps} optimiser steps skipped (fp16 gradients not finite); "
                f"loss scale now {trainer.current_loss_scale:g}")
        skipped = now
        vtot, vcnt = 0.0, 0
        kept = [] if cindex or valid_auroc or valid_auprc or rows_loss else None          # every validation batch's (logits, targets), on the device
        if valid_bags_per_call > 1 and rows_loss and hasattr(valid_batches, "block"):
            _validate_block(trainer, valid_batches, valid_bags_per_call, kept)
        elif valid_bags_per_call > 1:
            vtot, vcnt = _validate_ragged(trainer, valid_batches, dev, class_weights, loss_fn, valid_bags_per_call, kept, not cindex and not rows_loss)
        for bags, coords, _sizes, targets in (valid_batches() if valid_bags_per_call == 1 else ()):
            lg = trainer.predict(bags.to(dev), None if coords is None else coords.to(dev))
            if kept is not None:
                kept.append((lg, targets.to(dev)))
            if cindex or rows_loss:
                continue
            vtot += float(task_loss(lg, targets, dev, class_weights, loss_fn)) * bags.shape[0]
            vcnt += bags.shape[0]
        if rows_loss and kept:
            vtot, vcnt = _rows_loss_sum(kept, dev, class_weights, loss_fn)
        vloss = vtot / max(vcnt, 1)
        if valid_auroc or valid_auprc:
            lg_all, y_all = torch.cat([lg.float() for lg, _ in kept]), torch.cat([t.float() for _, t in kept])
            probs_all, cls_all = torch.softmax(lg_all, dim=1), y_all.argmax(dim=1)
            if valid_auroc:
                hist["validation_auroc"].append(float(metrics.multiclass_auroc(probs_all, cls_all)[1]))
            if valid_auprc:
                hist["validation_auprc"].append(float(metrics.multiclass_auprc(probs_all, cls_all)[1]))
        score = vloss
        if cindex:
            y = torch.cat([t.float().reshape(-1, 2) for _, t in kept]) if kept else torch.zeros(0, 2, device=dev)
            if not bool((y[:, 1] == 1).any()):
                raise RuntimeError(f"epoch {epoch}: the validation set holds no event, so there is no val_cindex to monitor")
            s_all = torch.cat([lg.float().reshape(-1) for lg, _ in kept])
            vloss, score = torch.stack([losses.cox_breslow_loss(s_all, y[:, 0], y[:, 1]).double(),
                                        metrics.concordance_index(s_all, y[:, 0], y[:, 1]).double()]).tolist()
            hist["val_cox_loss"].append(vloss)
            hist["val_cindex"].append(score)
        hist["validation_loss"].append(vloss)
        if log:
            log(f"epoch {epoch}: train {hist['train_loss'][-1]:.5f} validation {vloss:.5f}" + (f" val_cindex {score:.4f}" if cindex else ""))
        if cindex and not math.isfinite(score):          # EarlyStopping(check_finite=True): the monitored value left the numbers
            hist["stopped_epoch"] = epoch
            break
        if (score > best["loss"]) if cindex else (score < best["loss"]):
            best.update(loss=score, epoch=epoch, P=trainer.P.clone())
            wait = 0
        else:
            wait += 1
            if wait >= patience:
                hist["stopped_epoch"] = epoch
                break
    if best["P"] is not None:
        trainer.P.copy_(best["P"])
        trainer._refresh()
    trainer.sync_to_model()
    hist["best_epoch"] = best["epoch"]
    return hist


def reference_flops_per_bag(T: int = 1024, F: int = 1024, D: int = 512, FF: int = 512, L: int = 2) -> float:
    return mil_core.flops_per_bag(T, F, D, FF, L)
