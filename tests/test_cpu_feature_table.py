"""`cohort.ResidentFeatureTable` on host tensors (everything of the table that does not launch), over real files written with `h5io.write_slide_features`;
the labels against the reference's own slide / patient branch of `create_dataloader` (tests/golden/feature_table_labels.json, tools/make_golden.py);
`crossval`'s refusals and the fold-model round trip of the MLP / Linear heads."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from stamp_amd import cohort as C
from stamp_amd import crossval as X
from stamp_amd import h5io
from stamp_amd.bags import PatientData

GOLD = json.loads((Path(__file__).parent / "golden" / "feature_table_labels.json").read_text())
META = dict(encoder="test", precision="fp16", code_hash="0" * 8, stamp_version="2.5.0")


def _write(path, arr, feat_type="slide"):
    h5io.write_slide_features(path, arr, feat_type=feat_type, **META)
    return path


def _tile_file(path, n=5, F=8):
    h5io.write_tile_features(path, np.zeros((n, F), np.float16), np.zeros((n, 2), np.float32), extractor="test", tile_size_um=256.0, tile_size_px=224, code_hash="0" * 8,
                             stamp_version="2.5.0")
    return path


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    d = tmp_path_factory.mktemp("vec")
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((7, 8)).astype(np.float16)
    files = [_write(d / f"v{i}.h5", rows[i] if i % 2 else rows[i][None], "slide" if i < 4 else "patient") for i in range(7)]      # [F] and [1, F]
    return d, rows, files


def _pd(files, gts):
    return [PatientData(ground_truth=g, feature_files=[f]) for f, g in zip(files, gts)]


def test_vectors_of_both_shapes_are_read_and_the_store_keeps_the_files_precision(vectors):
    d, rows, files = vectors
    t = C.ResidentFeatureTable(_pd(files, list("abababa")), task="classification", device="cpu")
    assert len(t) == 7 and t.n_feats == 8 and t.dtype == torch.float16 and t.feats.dtype == torch.float16
    assert torch.equal(t.feats, torch.from_numpy(rows)) and t.nbytes == 7 * 8 * 2
    mixed = files[:3] + [_write(d / "f32.h5", rows[3].astype(np.float32))]
    t32 = C.ResidentFeatureTable(_pd(mixed, list("abab")), task="classification", device="cpu")
    assert t32.dtype == torch.float32 and torch.equal(t32.feats, torch.from_numpy(rows[:4]).float())          # one fp32 file: an fp32 store, fp16 widened exactly
    with pytest.raises(ValueError, match="max_bytes"):
        C.ResidentFeatureTable(_pd(files, list("abababa")), task="classification", device="cpu", max_bytes=7 * 8 * 2 - 1)


def test_refusals(vectors, tmp_path):
    d, rows, files = vectors
    two = _write(tmp_path / "two.h5", np.zeros((2, 8), np.float16))
    with pytest.raises(RuntimeError, match=r"Expected single feature vector \(shape \[F\] or \[1, F\]\), got \(2, 8\)"):
        C.ResidentFeatureTable(_pd([files[0], two], "ab"), task="classification", device="cpu")
    with pytest.raises(ValueError, match="tile-level"):
        C.ResidentFeatureTable(_pd([files[0], _tile_file(tmp_path / "tile.h5")], "ab"), task="classification", device="cpu")
    wide = _write(tmp_path / "wide.h5", np.zeros(9, np.float16))
    with pytest.raises(ValueError, match=r"one feature width, got \[8, 9\]"):
        C.ResidentFeatureTable(_pd([files[0], wide], "ab"), task="classification", device="cpu")
    with pytest.raises(ValueError, match="multi-target"):
        C.ResidentFeatureTable([PatientData(ground_truth={"x": "a"}, feature_files=[files[0]])], task="classification", device="cpu")


def test_an_entrys_first_file_is_taken(vectors):
    d, rows, files = vectors
    pdata = [PatientData(ground_truth="a", feature_files=[files[2], files[0]]), PatientData(ground_truth="b", feature_files=iter([files[5], files[1], files[3]]))]
    t = C.ResidentFeatureTable(pdata, task="classification", device="cpu")
    assert t.files == [files[2], files[5]] and torch.equal(t.feats, torch.from_numpy(rows[[2, 5]]))


@pytest.mark.parametrize("case", sorted(GOLD["cases"]))
def test_labels_equal_the_references(case):
    g = GOLD["cases"][case]
    gts = [tuple(x) if isinstance(x, list) else x for x in g["gts"]]
    pdata = [PatientData(ground_truth=gt, feature_files=[f"/feat/{n}.h5" for n in fs]) for gt, fs in zip(gts, g["files"])]
    labels, cats = C.feature_table_labels(pdata, g["task"], g["categories_in"])
    want = torch.tensor([[math.nan if v is None else v for v in r] for r in g["labels"]], dtype=torch.float32)
    assert str(labels.dtype) == g["labels_dtype"] and labels.shape == want.shape
    assert torch.equal(torch.nan_to_num(labels, nan=-7.0), torch.nan_to_num(want, nan=-7.0)) and torch.equal(labels.isnan(), want.isnan())
    assert [str(c) for c in cats] == g["categories"]
    assert [Path(next(iter(p.feature_files))).stem for p in pdata] == g["picked"]


def test_unknown_survival_status_raises_like_the_reference():
    assert GOLD["unknown_status_raises"] == "ValueError"
    with pytest.raises(ValueError, match="Unrecognized survival status"):
        C.parse_survival_status("unknown")


def test_epoch_order_is_one_randperm_with_a_tail_batch_and_views_share_storage(vectors):
    d, rows, files = vectors
    t = C.ResidentFeatureTable(_pd(files, list("abababa")), task="classification", device="cpu")
    view = t.view([6, 1, 4, 0, 2])
    assert view.table is t and len(view) == 5
    plan = view.epoch_plan(2, shuffle=True, generator=torch.Generator().manual_seed(9))
    g = torch.Generator().manual_seed(9)
    order = torch.randperm(5, generator=g)
    assert [b.tolist() for b in plan] == [torch.tensor([6, 1, 4, 0, 2])[order][a:a + 2].tolist() for a in (0, 2, 4)] and plan[-1].numel() == 1      # the tail batch
    g2 = torch.Generator().manual_seed(9)
    view.epoch_plan(2, shuffle=True, generator=g2)
    assert torch.equal(g2.get_state(), g.get_state())                                    # exactly ONE randperm(len(view)) was drawn
    assert [b.tolist() for b in view.epoch_plan(2, shuffle=True, generator=torch.Generator().manual_seed(9), drop_last=True)] == [b.tolist() for b in plan[:2]]
    assert [b.tolist() for b in view.epoch_plan(4, shuffle=False)] == [[6, 1, 4, 0], [2]]
    # validation: [1, F] views of the store in entry order, no copy
    items = list(view.valid_batches()())
    assert [tuple(x[0].shape) for x in items] == [(1, 8)] * 5 and all(x[1] is None and x[2] is None for x in items)
    for e, (feats, _c, _s, target) in zip(view.entries, items):
        assert feats.data_ptr() == t.feats[e].data_ptr() and torch.equal(target, t.targets[e:e + 1])
        assert feats.untyped_storage().data_ptr() == t.feats.untyped_storage().data_ptr()
    with pytest.raises(ValueError, match="outside"):
        t.view([7])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(view.train_batches(2)()))


def test_crossval_refuses_mixed_feature_types_and_vary_precision_before_any_work(vectors, tmp_path):
    d, rows, files = vectors
    boom = lambda **kw: (_ for _ in ()).throw(AssertionError("a trainer was built"))  # noqa: E731
    splits = [{"train_patients": ["p0", "p1"], "test_patients": ["p2", "p3"]}, {"train_patients": ["p2", "p3"], "test_patients": ["p0", "p1"]}]
    data = {f"p{i}": PatientData(ground_truth="ab"[i % 2], feature_files=[files[i]]) for i in range(3)}
    data["p3"] = PatientData(ground_truth="b", feature_files=[_tile_file(tmp_path / "tile.h5")])
    with pytest.raises(ValueError, match="one feature type"):
        X.crossval(data, task="classification", make_trainer=boom, splits=splits, ground_truth_label="y", device="cpu")
    data["p3"] = PatientData(ground_truth="b", feature_files=[files[3]])
    assert X.cohort_feature_type(data.values()) == "slide"
    with pytest.raises(ValueError, match="vary_precision_bits"):
        X.crossval(data, task="classification", make_trainer=boom, splits=splits, ground_truth_label="y", vary_precision_bits=4, device="cpu")
    with pytest.raises(ValueError, match="one feature type"):          # slide and patient files do not mix either
        X.cohort_feature_type([PatientData(ground_truth="a", feature_files=[files[0], files[5]])])


def test_fold_models_of_the_mlp_and_linear_heads_round_trip(tmp_path):
    from stamp_amd.mil import MLP, Linear

    class T:
        train_pred_median = 0.25

    torch.manual_seed(4)
    for model, kwargs in ((MLP(dim_input=12, dim_hidden=7, dim_output=3, num_layers=3, dropout=0.25), dict(dim_input=12, dim_hidden=7, dim_output=3, num_layers=3, dropout=0.25)),
                          (Linear(dim_input=12, dim_output=2), dict(dim_input=12, dim_output=2))):
        T.model = model
        assert X.head_constructor_args(model) == kwargs
        X.save_fold_model(tmp_path / "model.pt", T, task="classification", categories=["a", "b", "c"])
        back, doc = X.load_fold_model(tmp_path / "model.pt")
        assert type(back) is type(model) and not back.training and doc["head"] == type(model).__name__ and doc["train_pred_median"] == 0.25
        sd, sb = model.state_dict(), back.state_dict()
        assert list(sd) == list(sb) and all(torch.equal(sd[k], sb[k]) for k in sd)


def test_trainer_refuses_more_layers_than_the_library_takes():
    from stamp_amd import mlp_core
    from stamp_amd.mil import MLP
    with pytest.raises(ValueError, match="1 to 8 layers"):
        mlp_core.model_dims(MLP(dim_input=4, dim_hidden=4, dim_output=2, num_layers=9, dropout=0.0))
    assert mlp_core.model_dims(MLP(dim_input=5, dim_hidden=4, dim_output=2, num_layers=8, dropout=0.0)) == (5, 4, 2, 8)
