"""`stamp_amd.crossval.crossval` on the GPU: 18 patients with 1-2 feature files each (8-40 tiles x 48 features), 3 folds, 2 epochs, bags of 16, batches
of 4.  Every patient is predicted once, by the fold that did not train on it; every file is read once for the whole run; with the host sampler the folds --
views of one cohort -- train and predict bit for bit like separate cohorts built per fold; a finished output directory is not trained again; given folds
need no sklearn; and the device sampler feeds TransMIL, for which the order inside a bag matters."""
import json
import sys

import numpy as np
import pytest
import torch

from stamp_amd import bags as B
from stamp_amd import crossval as X
from stamp_amd import deploy, h5io
from stamp_amd.cohort import ResidentCohort

pytestmark = pytest.mark.gpu

N, FD, BAG, BATCH, FOLDS, EPOCHS = 18, 48, 16, 4, 3, 2
LABELS = ["pos" if i % 3 else "neg" for i in range(N)]
SURV = [(10.0 + 3.5 * i + (40.0 if i % 2 else 0.0), int(i % 3 != 0)) for i in range(N)]
REGR = [0.25 * i - 2.0 for i in range(N)]
# folds given by hand (no sklearn): patient i is tested by fold (i + i // 3) % 3 -- six patients per fold, two of them "neg"
GIVEN = [{"train_patients": [f"pat{i:02d}" for i in range(N) if (i + i // 3) % FOLDS != k],
          "test_patients": [f"pat{i:02d}" for i in range(N) if (i + i // 3) % FOLDS == k]} for k in range(FOLDS)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("crossval_files")
    rng = np.random.default_rng(1)
    out = []
    for i in range(N):
        fs = []
        for k in range(1 + i % 2):
            n = int(rng.integers(8, 21))          # 1-2 files of 8-20 tiles: 8-40 tiles per patient
            x = (rng.standard_normal((n, FD)) + (1.0 if LABELS[i] == "pos" else -1.0)).astype(np.float16)
            p = d / f"pat{i:02d}_{k}.h5"
            h5io.write_tile_features(p, x, rng.integers(0, 40, (n, 2)).astype(np.float32) * 256.0, extractor="test", tile_size_um=256.0, tile_size_px=224,
                                     code_hash="0", stamp_version="2.4.0")
            fs.append(p)
        out.append(fs)
    return out


def _data(files, gts):
    return {f"pat{i:02d}": B.PatientData(ground_truth=g, feature_files=fs) for i, (g, fs) in enumerate(zip(gts, files))}


def _abmil(gpu, dim_output, log=None):
    from stamp_amd.abmil import GatedAttentionMIL, HipAbmilTrainer

    def make(*, fold, dim_feats, categories, class_weights):
        if log is not None:
            log.append((fold, dim_feats, list(categories), class_weights))
        torch.manual_seed(100 + fold)
        return HipAbmilTrainer(GatedAttentionMIL(dim_feats, 64, 32, dim_output), device=gpu, max_lr=5e-3, total_steps=32, sched_interval="step", dropout=False)
    return make


def _vit(gpu, log=None):
    from stamp_amd.mil import VisionTransformer
    from stamp_amd.mil_train import HipMilVitTrainer

    def make(*, fold, dim_feats, categories, class_weights):
        if log is not None:
            log.append((fold, dim_feats, list(categories), class_weights))
        torch.manual_seed(200 + fold)
        model = VisionTransformer(dim_output=len(categories), dim_input=dim_feats, dim_model=64, n_layers=1, n_heads=2, dim_feedforward=64, dropout=0.0, use_alibi=False)
        return HipMilVitTrainer(model, device=gpu, max_lr=3e-3, total_steps=32, sched_interval="step", dropout=False)
    return make


def _count_reads(monkeypatch):
    """Counts `h5io.read_file` calls that fetch data (the header pass `feature_shape` may go through read_file on the pure-Python backend: not counted)."""
    calls = {"n": 0, "header": 0}
    real_read, real_shape = h5io.read_file, h5io.feature_shape

    def read(path):
        calls["n"] += 0 if calls["header"] else 1
        return real_read(path)

    def shape(path):
        calls["header"] += 1
        try:
            return real_shape(path)
        finally:
            calls["header"] -= 1

    monkeypatch.setattr(h5io, "read_file", read)
    monkeypatch.setattr(h5io, "feature_shape", shape)
    return calls


def _check_every_patient_predicted_by_the_fold_that_did_not_train_on_it(res, ids):
    assert len(res.splits) == len(res.predictions) == len(res.frames) == len(res.histories) == FOLDS
    seen = []
    for s, preds in zip(res.splits, res.predictions):
        assert set(preds) == set(s["test_patients"]) and not set(preds) & set(s["train_patients"])
        assert set(s["train_patients"]) | set(s["test_patients"]) == set(ids)
        seen += list(preds)
    assert sorted(seen) == sorted(ids)
    # the store is ordered by test fold: every test fold is a consecutive range
    assert res.cohort is not None and len(res.cohort) == len(ids)


def test_classification_vit_device_sampler_reads_every_file_once(gpu, files, tmp_path, monkeypatch):
    calls = _count_reads(monkeypatch)
    data, log = _data(files, LABELS), []
    out = tmp_path / "cv"
    res = X.crossval(data, task="classification", make_trainer=_vit(gpu, log), n_splits=FOLDS, output_dir=out, bag_size=BAG, batch_size=BATCH, max_epochs=EPOCHS,
                     ground_truth_label="KRAS", device=gpu, seed=5, generator=torch.Generator().manual_seed(0))
    assert calls["n"] == sum(len(f) for f in files) == 27          # each file once for 3 folds x 2 epochs + validation + prediction
    ids = list(data)
    _check_every_patient_predicted_by_the_fold_that_did_not_train_on_it(res, ids)
    assert [entry[0] for entry in log] == [0, 1, 2] and all(entry[1] == FD and entry[2] == ["neg", "pos"] for entry in log)
    for i, (s, hist, frame, preds) in enumerate(zip(res.splits, res.histories, res.frames, res.predictions)):
        assert list(frame.columns) == ["PATIENT", "KRAS", "pred", "KRAS_neg", "KRAS_pos", "loss"] and len(frame) == len(s["test_patients"])
        assert len(hist["train_loss"]) == EPOCHS and all(np.isfinite(hist["train_loss"])) and all(np.isfinite(hist["validation_loss"]))
        assert all(p.shape == (2,) and abs(float(p.sum()) - 1) < 1e-5 for p in preds.values())
        # class weights of the TRAIN fold
        train = [LABELS[ids.index(p)] for p in s["train_patients"]]
        w = torch.tensor([len(train) / train.count("neg"), len(train) / train.count("pos")])
        assert torch.allclose(log[i][3], w / w.sum())
        # the test fold is a consecutive range of the store (a ragged group of the view exists)
        test_view = res.cohort.view([j for j in range(len(ids)) if j // (len(ids) // FOLDS) == i])
        assert test_view.ragged_group(0, len(test_view)).n_bags == len(s["test_patients"])
    # what the run left behind
    assert json.loads((out / "splits.json").read_text())["splits"] == res.splits and X.read_splits(out / "splits.json") == res.splits
    assert res.splits == X.get_splits(ids, LABELS, n_splits=FOLDS, task="classification")
    for i in range(FOLDS):
        assert json.loads((out / f"split-{i}" / "history.json").read_text()) == res.histories[i]
        model, doc = X.load_fold_model(out / f"split-{i}" / "model.pt")
        assert doc["head"] == "VisionTransformer" and doc["categories"] == ["neg", "pos"] and doc["task"] == "classification" and doc["head_kwargs"]["dim_input"] == FD
    order = {p: j for j, p in enumerate(p for s in res.splits for p in ids if p in set(s["test_patients"]))}
    again = deploy.predict_(model, res.cohort.view([order[p] for p in res.predictions[2]]).valid_batches()(), list(res.predictions[2]), task="classification", device=gpu)
    assert all(torch.equal(again[p], res.predictions[2][p]) for p in again)
    # a second run on the same directory trains nothing, reads nothing and returns the same frames
    before = calls["n"]
    boom = lambda **kw: (_ for _ in ()).throw(AssertionError("a finished fold was trained again"))  # noqa: E731
    res2 = X.crossval(data, task="classification", make_trainer=boom, n_splits=FOLDS, output_dir=out, bag_size=BAG, batch_size=BATCH, max_epochs=EPOCHS,
                      ground_truth_label="KRAS", device=gpu)
    assert calls["n"] == before and res2.splits == res.splits and res2.histories == res.histories
    for a, b in zip(res.frames, res2.frames):
        assert a.to_csv(index=False) == b.to_csv(index=False)
    # one fold removed: only that fold runs again
    (out / "split-1" / "patient-preds.csv").unlink()
    log.clear()
    res3 = X.crossval(data, task="classification", make_trainer=_vit(gpu, log), n_splits=FOLDS, output_dir=out, bag_size=BAG, batch_size=BATCH, max_epochs=EPOCHS,
                      ground_truth_label="KRAS", device=gpu, seed=5, generator=torch.Generator().manual_seed(0))
    assert [entry[0] for entry in log] == [1] and res3.predictions[0] is None and set(res3.predictions[1]) == set(res.splits[1]["test_patients"])


def test_survival_and_regression_on_the_abmil_trainer(gpu, files):
    data = _data(files, SURV)
    res = X.crossval(data, task="survival", make_trainer=_abmil(gpu, 1), n_splits=FOLDS, bag_size=BAG, batch_size=BATCH, max_epochs=EPOCHS, device=gpu,
                     monitor="val_cindex", out_dtype=torch.float16)
    _check_every_patient_predicted_by_the_fold_that_did_not_train_on_it(res, list(data))
    assert res.splits == X.get_splits(list(data), SURV, n_splits=FOLDS, task="survival")
    for hist, frame in zip(res.histories, res.frames):
        assert len(hist["val_cindex"]) == EPOCHS and all(np.isfinite(hist["val_cindex"])) and len(hist["train_pred_median"]) == EPOCHS
        assert list(frame.columns) == ["PATIENT", "pred_score", "time", "event", f"cut_off={hist['train_pred_median'][-1]}"]
        assert all(np.isfinite(frame["pred_score"]))
    data = _data(files, REGR)
    res = X.crossval(data, task="regression", make_trainer=_abmil(gpu, 1), n_splits=FOLDS, bag_size=BAG, batch_size=BATCH, max_epochs=EPOCHS, device=gpu,
                     ground_truth_label="age", patient_label="P")
    _check_every_patient_predicted_by_the_fold_that_did_not_train_on_it(res, list(data))
    for hist, frame in zip(res.histories, res.frames):
        assert list(frame.columns) == ["P", "age", "pred", "loss"] and all(np.isfinite(frame["loss"])) and all(np.isfinite(hist["validation_loss"]))
        assert list(frame["loss"]) == sorted(frame["loss"])


def test_fold_views_equal_separate_cohorts_bit_for_bit(gpu, files):
    """sampler="torch", one generator seed, HipAbmilTrainer without dropout (its step is reproducible bit for bit): every fold's history and predictions equal
    a run that builds a fresh train and test ResidentCohort per fold and calls `fit` and `deploy.predict_` by hand."""
    from stamp_amd.mil_train import fit
    data = _data(files, LABELS)
    ids = list(data)
    res = X.crossval(data, task="classification", make_trainer=_abmil(gpu, 2), splits=GIVEN, bag_size=BAG, batch_size=BATCH, max_epochs=EPOCHS, sampler="torch",
                     generator=torch.Generator().manual_seed(4), ground_truth_label="KRAS", device=gpu, out_dtype=torch.float16, vary_precision_bits=6)
    g = torch.Generator().manual_seed(4)
    make = _abmil(gpu, 2)
    for i, s in enumerate(GIVEN):
        train_ids, test_ids = [p for p in ids if p in s["train_patients"]], [p for p in ids if p in s["test_patients"]]
        train = ResidentCohort([data[p] for p in train_ids], task="classification", categories=["neg", "pos"], device=gpu)
        test = ResidentCohort([data[p] for p in test_ids], task="classification", categories=["neg", "pos"], device=gpu)
        weights = B.class_weights(train.targets, ["neg", "pos"])
        trainer = make(fold=i, dim_feats=FD, categories=["neg", "pos"], class_weights=weights)
        hist = fit(trainer, train.train_batches(BATCH, BAG, shuffle=True, generator=g, out_dtype=torch.float16, vary_precision_bits=6), test.valid_batches(),
                   max_epochs=EPOCHS, patience=16, class_weights=weights)
        preds = deploy.predict_(trainer.model, test.valid_batches()(), test_ids, task="classification", device=gpu)
        print(f"fold {i}: views {res.histories[i]['train_loss']} separate cohorts {hist['train_loss']}")
        assert res.histories[i] == hist
        assert list(res.predictions[i]) == test_ids and all(torch.equal(res.predictions[i][p], preds[p]) for p in test_ids)
        assert all(np.isfinite(hist["train_loss"]))
    assert res.histories[0] != res.histories[1]


def test_given_splits_run_without_sklearn_and_transmil_takes_the_device_sampler(gpu, files, monkeypatch):
    from stamp_amd.mil import TransMIL
    from stamp_amd.transmil_train import HipTransMilTrainer
    for name in [m for m in sys.modules if m == "sklearn" or m.startswith("sklearn.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "sklearn", None)          # `import sklearn...` now raises ImportError
    with pytest.raises(ImportError):
        X.get_splits(["a", "b"], [1.0, 2.0], n_splits=2, task="regression")

    def make(*, fold, dim_feats, categories, class_weights):
        torch.manual_seed(300 + fold)
        return HipTransMilTrainer(TransMIL(dim_output=len(categories), dim_input=dim_feats, dim_hidden=128), device=gpu, max_lr=2e-3, total_steps=32,
                                  sched_interval="step", dropout=False)

    data = _data(files, LABELS)
    res = X.crossval(data, task="classification", make_trainer=make, splits=GIVEN, bag_size=BAG, batch_size=BATCH, max_epochs=EPOCHS, sampler="device", seed=2,
                     generator=torch.Generator().manual_seed(1), ground_truth_label="KRAS", device=gpu)
    _check_every_patient_predicted_by_the_fold_that_did_not_train_on_it(res, list(data))
    assert res.splits == [{k: sorted(v) for k, v in s.items()} for s in GIVEN]
    for hist in res.histories:
        assert len(hist["train_loss"]) == EPOCHS and all(np.isfinite(hist["train_loss"])) and all(np.isfinite(hist["validation_loss"]))
    # patients with data that no fold names are left out (and never read into the store); a barspoon-style trainer is refused
    extra = dict(data, zz=B.PatientData(ground_truth="pos", feature_files=[files[0][0].parent / "missing.h5"]))
    with pytest.raises(ValueError, match="crossval drives the trainers"):
        X.crossval(extra, task="classification", make_trainer=lambda **kw: object(), splits=GIVEN, bag_size=BAG, batch_size=BATCH, max_epochs=1,
                   ground_truth_label="KRAS", device=gpu)
