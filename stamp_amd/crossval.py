"""`stamp crossval` on the HIP path: k-fold training and test-fold predictions from ONE resident cohort.

Restates the reference's `categorical_crossval_` (src/stamp/modeling/crossval.py:48-370) for tile-level features and a single target:
  * the folds: `get_splits` = `_get_splits` (:373-426) with the splitter `categorical_crossval_` picks (:92-96) -- `StratifiedKFold` on the label
    (classification) or on the event status with a missing status counted as 0 (survival), `KFold` for regression; `shuffle=True, random_state=0`, patients
    in the mapping's order.  `splits.json` has the reference's schema (`_Splits`, :39-45); an existing file is used instead of drawing new folds (:84-112);
    a file naming a patient without data raises (:120-124); patients with data but in no fold are logged and left out (:126-130).
  * categories are those of the whole cohort (:137-151); the class weights come from the train fold (train.py:594-600).
  * per fold the "pure 2-way k-fold split" (:197-287): the test fold IS the validation set of the fit; then the test fold is predicted (:295-318) and shaped by
    `deploy.to_prediction_df` / `to_regression_prediction_df` / `to_survival_prediction_df` (:320-370), the survival cut-off being the trainer's
    `train_pred_median` (:337).  A fold whose `patient-preds.csv` exists is skipped (:183-188).

What differs, on purpose: the reference builds two DataLoaders per fold and re-reads every patient's `.h5` files in every epoch of every fold.  Here every
file is read ONCE into a `cohort.ResidentCohort` whose patients are ordered by test fold -- so every test fold is a consecutive row range of the store -- and
the folds are `CohortView`s of it: nothing is copied or read again.  With `sampler="device"` (the default here) an epoch's bags are drawn by one
`amds_bag_plan` launch; `sampler="torch"` keeps the host draws, and then a fold's batches are bit-identical to those of a separate cohort of its patients.
`split-{i}/model.pt` is a plain `torch.save` file (`load_fold_model` reads it), NOT a Lightning checkpoint: `deploy.model_from_checkpoint` does not take it.

Slide- / patient-level feature files (one vector per entry; the whole cohort must be of ONE feature type) take the same flow on a
`cohort.ResidentFeatureTable` ordered by test fold, with `mlp_train.HipMlpTrainer` over `mil.MLP` / `mil.Linear`: the reference's `feature_type in {"slide",
"patient"}` feed (src/stamp/modeling/data.py:355-419).  `bag_size` and `sampler` do not apply there; `vary_precision_bits` is refused.

Out of scope, each refused with a ValueError: multi-target ground truths and the barspoon trainer (it has its own `fit`), cohorts of mixed feature types,
and the CLI / config layer.  `sklearn` is needed by `get_splits` alone: `crossval(splits=...)` runs without it."""
from __future__ import annotations

import json
import logging
from collections.abc import Callable, Mapping, Sequence
from dataclasses import dataclass
from pathlib import Path
from typing import Any

import torch

from . import bags as B
from . import deploy, losses
from . import h5io
from .cohort import ResidentCohort, ResidentFeatureTable

_log = logging.getLogger("stamp_amd")
TASKS = ("classification", "regression", "survival")
Split = dict          # {"train_patients": [...], "test_patients": [...]}, lists sorted


# ---- folds -------------------------------------------------------------------------------------------------------------------------------------
def get_splits(patient_ids: Sequence[str], ground_truths: Sequence[Any], *, n_splits: int, task: str) -> list[Split]:
    """The reference's `_get_splits` (crossval.py:373-426): -> one {"train_patients", "test_patients"} dict of sorted id lists per fold."""
    import numpy as np
    from sklearn.model_selection import KFold, StratifiedKFold          # (the only use of sklearn in this module)

    if task not in TASKS:
        raise ValueError(f"task must be one of {TASKS}, got {task!r}")
    if len(patient_ids) != len(ground_truths):
        raise ValueError("as many ground truths as patients")
    if any(isinstance(g, dict) for g in ground_truths):
        raise ValueError("multi-target ground truths are out of scope here")
    patients = np.array(list(patient_ids))
    if task == "survival":
        statuses = []
        for g in ground_truths:
            status = g[1] if isinstance(g, (tuple, list)) and len(g) == 2 else g
            statuses.append(int(status) if status is not None else 0)
        y, splitter = np.array(statuses), StratifiedKFold
    elif task == "classification":
        y, splitter = np.array(list(ground_truths)), StratifiedKFold
    else:
        y, splitter = None, KFold
    skf = splitter(n_splits=n_splits, shuffle=True, random_state=0)
    folds = skf.split(patients) if y is None else skf.split(patients, y)
    return [{"train_patients": sorted(str(p) for p in patients[tr]), "test_patients": sorted(str(p) for p in patients[te])} for tr, te in folds]


def write_splits(path, splits: Sequence[Split]) -> None:
    """`splits.json` in the reference's schema: {"splits": [{"train_patients": [...], "test_patients": [...]}]}, lists sorted."""
    doc = {"splits": [{"train_patients": sorted(str(p) for p in s["train_patients"]), "test_patients": sorted(str(p) for p in s["test_patients"])} for s in splits]}
    Path(path).write_text(json.dumps(doc, indent=4) + "\n")


def read_splits(path) -> list[Split]:
    doc = json.loads(Path(path).read_text())
    if not isinstance(doc, dict) or not isinstance(doc.get("splits"), list):
        raise ValueError(f'{path}: not a splits file ({{"splits": [...]}} expected)')
    out = []
    for s in doc["splits"]:
        if not isinstance(s, dict) or "train_patients" not in s or "test_patients" not in s:
            raise ValueError(f"{path}: every split needs train_patients and test_patients")
        out.append({"train_patients": sorted(str(p) for p in s["train_patients"]), "test_patients": sorted(str(p) for p in s["test_patients"])})
    return out


def check_splits(splits: Sequence[Split], patient_ids) -> set:
    """The two mismatch rules of crossval.py:114-130: a split naming a patient without data raises RuntimeError; patients with data but in no split are
    logged and returned (they are left out)."""
    in_splits = {p for s in splits for p in (*s["train_patients"], *s["test_patients"])}
    have = set(patient_ids)
    if missing := in_splits - have:
        raise RuntimeError(f"The splits file contains some patients we don't have information for in the clini / slide table: {sorted(missing)}")
    if left_out := have - in_splits:
        _log.warning(f"Some of the entries in the clini / slide table are not in the crossval split: {sorted(left_out)}")
    return left_out


# ---- per-fold files ----------------------------------------------------------------------------------------------------------------------------------
def head_constructor_args(model: torch.nn.Module) -> dict:
    """The keyword arguments that rebuild a MIL head `fit` can train."""
    from . import mlp_core
    from .abmil import GatedAttentionMIL
    from .mil import MLP, Linear, TransMIL, VisionTransformer
    if isinstance(model, MLP):
        fi, hid, out, layers = mlp_core.model_dims(model)
        return dict(dim_input=fi, dim_hidden=hid, dim_output=out, num_layers=layers, dropout=model.dropout_p)
    if isinstance(model, Linear):
        return dict(dim_input=model.fc.in_features, dim_output=model.fc.out_features)
    if isinstance(model, VisionTransformer):
        d = model.dims
        return dict(dim_output=d.C, dim_input=d.F, dim_model=d.D, n_layers=d.L, n_heads=d.H, dim_feedforward=d.FF, dropout=model.dropout, use_alibi=model.use_alibi)
    if isinstance(model, TransMIL):
        return dict(dim_output=model.n_classes, dim_input=model._fc1[0].in_features, dim_hidden=model.dim_hidden)
    if isinstance(model, GatedAttentionMIL):
        fi, hid, att, out = model.dims
        return dict(dim_input=fi, dim_hidden=hid, dim_attention=att, dim_output=out, dropout=model.dropout)
    raise ValueError(f"{type(model).__name__} is not a head `mil_train.fit` trains (VisionTransformer, TransMIL, GatedAttentionMIL, MLP, Linear)")


def save_fold_model(path, trainer, *, task: str, categories: Sequence) -> None:
    """`split-{i}/model.pt`: a `torch.save` dict {format, head, head_kwargs, state_dict, task, categories, train_pred_median} -- not a Lightning checkpoint."""
    model = trainer.model
    torch.save({"format": "stamp_amd.crossval/1", "head": type(model).__name__, "head_kwargs": head_constructor_args(model),
                "state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "task": task, "categories": list(categories),
                "train_pred_median": getattr(trainer, "train_pred_median", None)}, path)


def load_fold_model(path) -> tuple[torch.nn.Module, dict]:
    """-> (the head of a `split-{i}/model.pt` in eval mode, the file's dict)."""
    from .abmil import GatedAttentionMIL
    from .mil import MLP, Linear, TransMIL, VisionTransformer
    doc = torch.load(path, map_location="cpu", weights_only=True)
    heads = {c.__name__: c for c in (VisionTransformer, TransMIL, GatedAttentionMIL, MLP, Linear)}
    if doc.get("format") != "stamp_amd.crossval/1" or doc.get("head") not in heads:
        raise ValueError(f"{path}: not a model file of stamp_amd.crossval")
    model = heads[doc["head"]](**doc["head_kwargs"])
    model.load_state_dict(doc["state_dict"])
    return model.eval(), doc


# ---- the run ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class CrossvalResult:
    splits: list          # the folds used, `splits.json`'s content
    cohort: Any           # the ONE ResidentCohort / ResidentFeatureTable (None when every fold was already done)
    histories: list       # per fold: `fit`'s history (a skipped fold: its history.json, or None)
    predictions: list     # per fold: patient id -> prediction on the CPU (a skipped fold: None)
    frames: list          # per fold: the `patient-preds.csv` table


def _frame(task, predictions, gts, categories, patient_label, ground_truth_label, cut_off):
    if task == "classification":
        return deploy.to_prediction_df(categories=categories, patient_to_ground_truth=gts, predictions=predictions, patient_label=patient_label,
                                       ground_truth_label=ground_truth_label)
    if task == "regression":
        return deploy.to_regression_prediction_df(patient_to_ground_truth=gts, predictions=predictions, patient_label=patient_label,
                                                  ground_truth_label=ground_truth_label)
    return deploy.to_survival_prediction_df(patient_to_ground_truth=gts, predictions=predictions, patient_label=patient_label, cut_off=cut_off)


def cohort_feature_type(patient_data) -> str:
    """"tile", "slide" or "patient": the feature type of every file of the cohort (`h5io.feature_type`); a cohort of mixed types is a ValueError."""
    kinds: dict = {}
    for p in patient_data:
        for f in p.feature_files:
            kinds.setdefault(h5io.file_feature_type(f), f)
    if not kinds:
        return "tile"
    if len(kinds) != 1:
        raise ValueError("the cohort's feature files must be of one feature type, got " + ", ".join(f"{k} ({v})" for k, v in sorted(kinds.items(), key=lambda kv: str(kv[0]))))
    return next(iter(kinds))


def crossval(patient_to_data: Mapping[str, B.PatientData], *, task: str, make_trainer: Callable, n_splits: int = 5, splits: Sequence[Split] | None = None,
             output_dir=None, categories: Sequence[str] | None = None, bag_size: int = 512, batch_size: int = 64, max_epochs: int = 64, patience: int = 16,
             sampler: str = "device", seed: int = 0, generator: torch.Generator | None = None, vary_precision_bits: int | None = None,
             valid_bags_per_call: int = 1, predict_bags_per_call: int = 1, patient_label: str = "PATIENT", ground_truth_label: str | None = None,
             device="cuda", out_dtype: torch.dtype = torch.float32, **fit_kwargs) -> CrossvalResult:
    """patient_to_data: patient id -> `bags.PatientData` (tile-level feature files, one ground truth).  make_trainer(fold=, dim_feats=, categories=,
    class_weights=) -> any trainer `mil_train.fit` drives (HipMilVitTrainer, HipTransMilTrainer, HipAbmilTrainer).  splits: the folds to use (else
    `output_dir/splits.json` if it exists, else `get_splits`).  fit_kwargs go to `fit`: survival runs pass monitor="val_cindex"; `loss_fn` defaults to the
    task's (cross-entropy / `losses.l1_loss` / `losses.cox_survival_loss`).  The device sampler of fold i is keyed with `seed + i`, so a patient does not
    meet the same bags in two folds.  Slide- / patient-level files (one feature type for the whole cohort, else ValueError): ONE `ResidentFeatureTable`
    instead, `make_trainer` returning a `HipMlpTrainer`; `bag_size`, `sampler`, `seed` and `out_dtype` do not apply, `vary_precision_bits` is refused.  Module
    docstring for the flow and what it writes under `output_dir`."""
    from .mil_train import fit
    if task not in TASKS:
        raise ValueError(f"task must be one of {TASKS}, got {task!r}")
    if any(isinstance(p.ground_truth, dict) for p in patient_to_data.values()):
        raise ValueError("multi-target ground truths are out of scope: crossval trains one target (the barspoon trainer has its own fit)")
    if task != "survival" and ground_truth_label is None:
        raise ValueError(f"ground_truth_label is required for {task}")
    data = {str(p): d for p, d in patient_to_data.items()}
    ids = list(data)
    gts = {p: d.ground_truth for p, d in data.items()}
    out = None if output_dir is None else Path(output_dir)
    if out is not None:
        out.mkdir(parents=True, exist_ok=True)
    if splits is not None:
        splits = [{"train_patients": sorted(str(p) for p in s["train_patients"]), "test_patients": sorted(str(p) for p in s["test_patients"])} for s in splits]
    elif out is not None and (out / "splits.json").exists():
        splits = read_splits(out / "splits.json")
    else:
        splits = get_splits(ids, [gts[p] for p in ids], n_splits=n_splits, task=task)
    left_out = check_splits(splits, ids)
    feature_type = cohort_feature_type(d for p, d in data.items() if p not in left_out)          # (file attributes only: no dataset is read)
    vectors = feature_type in ("slide", "patient")
    if vectors and vary_precision_bits is not None:
        raise ValueError(f"vary_precision_bits does not apply to {feature_type}-level features (the reference's transform is part of the tile feed)")
    if out is not None and not (out / "splits.json").exists():
        write_splits(out / "splits.json", splits)
    if task == "classification":
        categories = list(categories) if categories else sorted({g for g in gts.values() if g is not None})
    else:
        categories = []

    n = len(splits)
    res = CrossvalResult(splits=list(splits), cohort=None, histories=[None] * n, predictions=[None] * n, frames=[None] * n)
    todo = []
    for i in range(n):
        d = None if out is None else out / f"split-{i}"
        if d is not None and (d / "patient-preds.csv").exists():
            import pandas as pd
            _log.info(f"skipping training for split {i}, as its predictions are already present")
            res.frames[i] = pd.read_csv(d / "patient-preds.csv", float_precision="round_trip")          # (the default parser is an ulp off)
            if (d / "history.json").exists():
                res.histories[i] = json.loads((d / "history.json").read_text())
        else:
            todo.append(i)
    if not todo:
        return res

    # ---- read once: the patients ordered by test fold, so that every test fold is a consecutive range of the store
    position: dict = {}
    for s in splits:
        members = set(s["test_patients"])
        for p in ids:
            if p in members and p not in position:
                position[p] = len(position)
    for s in splits:          # (patients that are only ever trained on)
        members = set(s["train_patients"])
        for p in ids:
            if p in members and p not in position:
                position[p] = len(position)
    store_ids = sorted(position, key=position.__getitem__)
    if vectors:
        cohort = ResidentFeatureTable([data[p] for p in store_ids], task=task, categories=categories or None, device=device)
    else:
        cohort = ResidentCohort([data[p] for p in store_ids], task=task, categories=categories or None, device=device)
        if cohort.multi_target:
            raise ValueError("multi-target ground truths are out of scope")
    res.cohort = cohort
    default_loss = {"classification": None, "regression": losses.l1_loss, "survival": losses.cox_survival_loss}[task]
    fit_kwargs.setdefault("loss_fn", default_loss)

    for i in todo:
        s = splits[i]
        train_set, test_set = set(s["train_patients"]), set(s["test_patients"])
        train_ids, test_ids = [p for p in ids if p in train_set], [p for p in ids if p in test_set]
        train_view, test_view = cohort.view([position[p] for p in train_ids]), cohort.view([position[p] for p in test_ids])
        weights = B.class_weights(cohort.targets[train_view.entries if vectors else train_view.patients], categories) if task == "classification" else None
        trainer = make_trainer(fold=i, dim_feats=cohort.n_feats, categories=list(categories), class_weights=weights)
        if type(trainer).__name__ == "HipBarspoonTrainer" or not all(hasattr(trainer, a) for a in ("step", "predict", "epoch_end", "P", "model")):
            raise ValueError(f"make_trainer returned {type(trainer).__name__}: crossval drives the trainers of `mil_train.fit` (the barspoon trainer has its own fit)")
        if vectors:
            feed = train_view.train_batches(batch_size, shuffle=True, generator=generator)
        else:
            feed = train_view.train_batches(batch_size, bag_size, shuffle=True, generator=generator, out_dtype=out_dtype, vary_precision_bits=vary_precision_bits,
                                            sampler=sampler, seed=int(seed) + i)
        hist = fit(trainer, feed, test_view.valid_batches(), max_epochs=max_epochs, patience=patience, class_weights=weights,
                   valid_bags_per_call=valid_bags_per_call, **fit_kwargs)
        preds = deploy.predict_(trainer.model, test_view.valid_batches()(), test_ids, task=task, device=device, bags_per_call=predict_bags_per_call)
        frame = _frame(task, preds, gts, categories, patient_label, ground_truth_label, getattr(trainer, "train_pred_median", None))
        res.histories[i], res.predictions[i], res.frames[i] = hist, preds, frame
        if out is not None:
            d = out / f"split-{i}"
            d.mkdir(parents=True, exist_ok=True)
            save_fold_model(d / "model.pt", trainer, task=task, categories=categories)
            (d / "history.json").write_text(json.dumps(hist, indent=1) + "\n")
            frame.to_csv(d / "patient-preds.csv", index=False)          # last: its presence marks the fold as done
    return res


__all__ = ["cohort_feature_type", "get_splits", "write_splits", "read_splits", "check_splits", "crossval", "CrossvalResult", "save_fold_model", "load_fold_model", "head_constructor_args",
           "TASKS"]
