"""Training the barspoon head (`EncDecTransformer`) on the HIP path.

`HipBarspoonTrainer` is the reference's `LitMilClassificationMixin` (src/stamp/modeling/models/barspoon.py:211-348) without Lightning: one
`step` = `EncDecTransformer.forward_train` (ONE library call forward, ONE backward; csrc/barspoon_train.hip), the reference's loss
(:285-292: the sum over the targets of `F.cross_entropy(logits, float one-hot, weight=)`, in torch like the other heads' losses), and
`torch.optim.Adam(lr)` (:346-348) over the module's own parameters.  `predict` is the deploy forward (`EncDecTransformer.forward` in eval mode),
`predict_ragged` the same over bags of different lengths in one call (`forward_ragged`).
`fit` is the epoch loop of the reference's `train_model_` (src/stamp/modeling/train.py:504-564): validation loss after every epoch, early stopping
on it (mode min), the best epoch's weights restored.  There is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import copy

import torch
import torch.nn.functional as F

from .barspoon import EncDecTransformer


def multi_target_loss(logits: dict[str, torch.Tensor], targets: dict[str, torch.Tensor], weights: dict[str, torch.Tensor] | None = None) -> torch.Tensor:
    """barspoon.py:285-292: sum over the targets of the weighted cross entropy against float one-hot (or soft) labels."""
    total = None
    for t, lg in logits.items():
        w = None if weights is None or weights.get(t) is None else weights[t].to(lg.device, torch.float32)
        term = F.cross_entropy(lg, targets[t].to(lg.device, torch.float32), weight=w)
        total = term if total is None else total + term
    return total


class HipBarspoonTrainer:
    def __init__(self, model: EncDecTransformer, *, device="cuda", learning_rate: float = 1e-4, dropout: float | bool | None = None, seed: int = 0) -> None:
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("HipBarspoonTrainer runs on the GPU only (no CPU fallback)")
        self.model = model.to(self.dev)
        self.dropout = dropout
        self.optimizer = torch.optim.Adam(self.model.parameters(), lr=learning_rate)            # barspoon.py:346-348
        self._gen = torch.Generator().manual_seed(seed)                                          # the steps' mask seeds: reproducible per trainer
        self.steps = 0

    def _check(self, feats: torch.Tensor) -> None:
        if not feats.is_cuda:
            raise RuntimeError("HipBarspoonTrainer needs bags on the GPU (no CPU fallback)")

    def step(self, feats: torch.Tensor, positions: torch.Tensor, targets: dict[str, torch.Tensor], weights: dict[str, torch.Tensor] | None = None, *,
             update: bool = True, seed: int | None = None):
        """One training step -> (loss, {target: logits}).  `update=False` computes loss and gradients (left in `.grad`) without the optimiser step."""
        self._check(feats)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=self._gen).item())
        self.optimizer.zero_grad(set_to_none=True)
        logits = self.model.forward_train(feats, positions, seed=seed, dropout=self.dropout)
        loss = multi_target_loss(logits, targets, weights)
        loss.backward()
        if update:
            self.optimizer.step()
            self.steps += 1
        return loss.detach(), {t: v.detach() for t, v in logits.items()}

    @torch.no_grad()
    def predict(self, feats: torch.Tensor, positions: torch.Tensor) -> dict[str, torch.Tensor]:
        """The eval forward on the current weights (`EncDecTransformer.forward`, one library call)."""
        self._check(feats)
        was = self.model.training
        self.model.eval()
        try:
            return self.model(feats, positions)
        finally:
            self.model.train(was)

    @torch.no_grad()
    def predict_ragged(self, bags, positions, *, bags_per_call: int | None = None, max_rows_per_call: int = 1 << 62) -> dict[str, torch.Tensor]:
        """The eval forward on the current weights over bags of DIFFERENT lengths (`EncDecTransformer.forward_ragged`): lists of [T_i, d_features] and
        [T_i, 2] tensors -> `{target: logits [N, n_out]}`, bag i's rows bit-identical to `predict(bags[i][None], positions[i][None])`."""
        bags = list(bags)
        for b in bags:
            self._check(b)
        was = self.model.training
        self.model.eval()
        try:
            return self.model.forward_ragged(bags, positions, bags_per_call=bags_per_call, max_rows_per_call=max_rows_per_call)
        finally:
            self.model.train(was)

    def _validation_sum(self, valid_batches, weights, bags_per_call: int, max_rows_per_call: int) -> tuple[float, int]:
        """Sum over the validation batches of loss * batch size, and the bag count.  bags_per_call > 1: consecutive one-bag batches share ragged calls;
        each bag's loss is formed from its own logits row and the host reads once per group -- the same values added in the same order as the loop's."""
        dev = self.dev
        vtot, vcnt = 0.0, 0
        pend: list = []

        def flush():
            nonlocal vtot, vcnt
            if not pend:
                return
            pos = None if pend[0][1] is None else [p for _, p, _ in pend]
            lg = self.predict_ragged([b for b, _, _ in pend], pos, bags_per_call=bags_per_call, max_rows_per_call=max_rows_per_call)
            losses = torch.stack([multi_target_loss({t: v[i:i + 1] for t, v in lg.items()}, pend[i][2], weights) for i in range(len(pend))])
            for v in losses.tolist():           # one device-to-host read
                vtot += v
            vcnt += len(pend)
            pend.clear()

        for feats, positions, targets in valid_batches():
            if bags_per_call > 1 and feats.shape[0] == 1:
                if pend and (pend[0][1] is None) != (positions is None):
                    flush()
                pend.append((feats[0].to(dev), None if positions is None else positions[0].to(dev), targets))
                if len(pend) >= bags_per_call:
                    flush()
                continue
            flush()
            lg = self.predict(feats.to(dev), None if positions is None else positions.to(dev))
            vtot += float(multi_target_loss(lg, targets, weights)) * feats.shape[0]
            vcnt += feats.shape[0]
        flush()
        return vtot, vcnt

    def fit(self, train_batches, valid_batches, *, max_epochs: int, patience: int = 16, weights=None, log=None, valid_bags_per_call: int = 1,
            valid_max_rows_per_call: int = 262144) -> dict:
        """train_batches / valid_batches: callables returning an iterable of (feats, positions, targets) per epoch.  Validation loss (eval forward,
        Lightning's mean over batches weighted by batch size) after every epoch; stops when it has not improved for `patience` epochs; the best epoch's
        weights are restored.  valid_bags_per_call > 1: one-bag validation batches share ragged calls of at most that many bags and
        `valid_max_rows_per_call` tile rows (`predict_ragged`), with the losses of the one-bag loop.  Returns the history."""
        if valid_bags_per_call < 1 or valid_max_rows_per_call < 1:
            raise ValueError("valid_bags_per_call and valid_max_rows_per_call must be >= 1")
        dev = self.dev
        best = {"loss": float("inf"), "epoch": -1, "state": None}
        hist = {"train_loss": [], "validation_loss": [], "best_epoch": -1, "stopped_epoch": None}
        wait = 0
        for epoch in range(max_epochs):
            tot, cnt = 0.0, 0
            for feats, positions, targets in train_batches():
                loss, _ = self.step(feats.to(dev), None if positions is None else positions.to(dev), targets, weights)
                tot += float(loss) * feats.shape[0]
                cnt += feats.shape[0]
            hist["train_loss"].append(tot / max(cnt, 1))
            vtot, vcnt = self._validation_sum(valid_batches, weights, valid_bags_per_call, valid_max_rows_per_call)
            vloss = vtot / max(vcnt, 1)
            hist["validation_loss"].append(vloss)
            if log:
                log(f"epoch {epoch}: train {hist['train_loss'][-1]:.5f} validation {vloss:.5f}")
            if vloss < best["loss"]:
                best.update(loss=vloss, epoch=epoch, state=copy.deepcopy(self.model.state_dict()))
                wait = 0
            else:
                wait += 1
                if wait >= patience:
                    hist["stopped_epoch"] = epoch
                    break
        if best["state"] is not None:
            self.model.load_state_dict(best["state"])
        hist["best_epoch"] = best["epoch"]
        return hist
