"""The host side of stamp_amd/crossval.py and of the cohort's fold views -- no GPU: the folds against the reference's own `_get_splits`
(tests/golden/crossval_splits.json, written by tools/make_golden.py::golden_crossval_splits), the splits file and its two mismatch rules, and the
bookkeeping of `CohortView` on a store of host tensors."""
import json
import logging
from pathlib import Path

import pytest
import torch

from stamp_amd import cohort as C
from stamp_amd import crossval as X

GOLD = json.loads((Path(__file__).parent / "golden" / "crossval_splits.json").read_text())


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: f"{c['task']}-{c['n_splits']}")
def test_get_splits_equals_the_references_folds(case):
    """Classification with 3 unbalanced classes (13 / 6 / 4), survival with missing statuses, regression; 23 patients, 3 and 5 folds.  Folds compared as sets,
    in fold order."""
    gts = [tuple(g) if isinstance(g, list) else g for g in GOLD["ground_truths"][case["task"]]]
    assert len(GOLD["patients"]) == 23 == len(gts)
    if case["task"] == "classification":
        assert sorted(gts.count(c) for c in set(gts)) == [4, 6, 13]
    if case["task"] == "survival":
        assert sum(g[1] is None for g in gts) >= 2
    got = X.get_splits(GOLD["patients"], gts, n_splits=case["n_splits"], task=case["task"])
    assert len(got) == case["n_splits"] == len(case["splits"])
    for g, w in zip(got, case["splits"]):
        assert set(g["train_patients"]) == set(w["train_patients"]) and set(g["test_patients"]) == set(w["test_patients"])
        assert g["train_patients"] == sorted(g["train_patients"]) and g["test_patients"] == sorted(g["test_patients"])
        assert not set(g["train_patients"]) & set(g["test_patients"]) and len(g["train_patients"]) + len(g["test_patients"]) == 23
    assert sorted(p for g in got for p in g["test_patients"]) == sorted(GOLD["patients"])          # every patient is tested exactly once


def test_get_splits_refuses_what_is_out_of_scope():
    with pytest.raises(ValueError, match="task"):
        X.get_splits(["a", "b"], [1, 2], n_splits=2, task="ranking")
    with pytest.raises(ValueError, match="multi-target"):
        X.get_splits(["a", "b"], [{"x": 1}, {"x": 2}], n_splits=2, task="classification")
    with pytest.raises(ValueError, match="as many"):
        X.get_splits(["a", "b"], [1], n_splits=2, task="regression")


def test_splits_file_round_trip_and_the_two_mismatch_rules(tmp_path, caplog):
    splits = [{"train_patients": ["c", "a"], "test_patients": ["b"]}, {"train_patients": {"b"}, "test_patients": ("c", "a")}]
    X.write_splits(tmp_path / "splits.json", splits)
    doc = json.loads((tmp_path / "splits.json").read_text())
    assert doc == {"splits": [{"train_patients": ["a", "c"], "test_patients": ["b"]}, {"train_patients": ["b"], "test_patients": ["a", "c"]}]}
    back = X.read_splits(tmp_path / "splits.json")
    assert back == doc["splits"]
    (tmp_path / "bad.json").write_text(json.dumps({"folds": []}))
    with pytest.raises(ValueError, match="not a splits file"):
        X.read_splits(tmp_path / "bad.json")
    # a split naming a patient without data raises; a patient with data but in no split is logged and left out
    with pytest.raises(RuntimeError, match=r"don't have information.*\['c'\]"):
        X.check_splits(back, ["a", "b"])
    with caplog.at_level(logging.WARNING, logger="stamp_amd"):
        assert X.check_splits(back, ["a", "b", "c", "zz"]) == {"zz"}
    assert "not in the crossval split" in caplog.text and "zz" in caplog.text
    assert X.check_splits(back, ["a", "b", "c"]) == set()


def test_crossval_refusals_come_before_any_work():
    from stamp_amd.bags import PatientData
    boom = lambda **kw: (_ for _ in ()).throw(AssertionError("a trainer was built"))  # noqa: E731
    multi = {"a": PatientData(ground_truth={"x": "1"}, feature_files=[]), "b": PatientData(ground_truth={"x": "2"}, feature_files=[])}
    with pytest.raises(ValueError, match="multi-target"):
        X.crossval(multi, task="classification", make_trainer=boom, ground_truth_label="x")
    one = {"a": PatientData(ground_truth="1", feature_files=[]), "b": PatientData(ground_truth="2", feature_files=[])}
    with pytest.raises(ValueError, match="task"):
        X.crossval(one, task="ranking", make_trainer=boom)
    with pytest.raises(ValueError, match="ground_truth_label"):
        X.crossval(one, task="classification", make_trainer=boom)
    with pytest.raises(RuntimeError, match="don't have information"):
        X.crossval(one, task="classification", make_trainer=boom, ground_truth_label="x", splits=[{"train_patients": ["a", "q"], "test_patients": ["b"]}])


def _stub_store(lengths, Fd=4):
    """A ResidentCohort over host tensors, without files or a device: row r of the store holds the value r."""
    c = C.ResidentCohort.__new__(C.ResidentCohort)
    c.lengths = list(lengths)
    c.offsets = [0]
    for n in c.lengths:
        c.offsets.append(c.offsets[-1] + n)
    R = c.offsets[-1]
    c.device = torch.device("cpu")
    c.feats = torch.arange(R, dtype=torch.float32)[:, None].expand(R, Fd).contiguous()
    c.coords = torch.arange(2 * R, dtype=torch.float32).reshape(R, 2)
    c._offsets_dev = torch.tensor(c.offsets, dtype=torch.int32)
    c._lengths_dev = torch.tensor(c.lengths, dtype=torch.int64)
    c.multi_target = False
    c.targets = c._targets_dev = torch.arange(len(c.lengths), dtype=torch.float32)[:, None]
    c.n_feats = Fd
    return c


def test_view_bookkeeping_on_a_stub_store():
    c = _stub_store([3, 1, 4, 2, 5])
    v = c.view([3, 0, 1, 2])
    assert isinstance(v, C.CohortView) and len(v) == 4 and v.patients == [3, 0, 1, 2] and len(c) == 5
    # validation batches: the view's patients in the view's order, every tensor a view of the store (no copy)
    got = list(v.valid_batches()())
    assert [int(t[3].item()) for t in got] == [3, 0, 1, 2] and [int(t[2].item()) for t in got] == [2, 3, 1, 4]
    assert [t[0][0, 0, 0].item() for t in got] == [8.0, 0.0, 3.0, 4.0] and all(t[0].shape == (1, n, 4) for t, n in zip(got, (2, 3, 1, 4)))
    assert all(t[0].untyped_storage().data_ptr() == c.feats.untyped_storage().data_ptr() for t in got)
    assert all(t[1].untyped_storage().data_ptr() == c.coords.untyped_storage().data_ptr() for t in got)
    assert [len(t) for t in v.barspoon_valid_batches()()] == [3] * 4
    # the cohort's own methods are the view over range(len)
    assert [int(t[3].item()) for t in c.valid_batches()()] == [0, 1, 2, 3, 4]
    # ragged groups: consecutive store patients only
    rb = v.ragged_group(1, 4)
    assert rb.lengths == (3, 1, 4) and rb.offsets.tolist() == [0, 3, 4, 8] and rb.feats.shape == (8, 4) and rb.feats[0, 0] == 0
    assert rb.feats.untyped_storage().data_ptr() == c.feats.untyped_storage().data_ptr()
    assert v.ragged_group(0, 1).lengths == (2,) and v.ragged_group(0, 1).feats[0, 0] == 8 and v.ragged_group(2, 2).lengths == ()
    with pytest.raises(ValueError, match="not consecutive"):
        v.ragged_group(0, 2)
    with pytest.raises(ValueError, match="not consecutive"):
        c.view([0, 2]).ragged_group(0, 2)
    with pytest.raises(ValueError, match="outside"):
        v.ragged_group(2, 5)
    with pytest.raises(ValueError, match="outside"):
        c.view([0, 5])
    assert c.view([]).ragged_group(0, 0).lengths == () and list(c.view([]).valid_batches()()) == []
    # argument checks of the feeds, before anything runs
    for feed in (v.train_batches, v.barspoon_batches, c.train_batches, c.barspoon_batches):
        with pytest.raises(ValueError, match="shuffle=False"):
            feed(2, 2, shuffle=False, sampler="device")
        with pytest.raises(ValueError, match="sampler"):
            feed(2, 2, sampler="numpy")
        with pytest.raises(ValueError, match=">= 1"):
            feed(0, 2)
        assert callable(feed(2, 2, shuffle=False)) and callable(feed(2, 2, sampler="device", seed=3))


def test_view_draws_what_a_separate_cohort_draws(monkeypatch):
    """sampler="torch": a view over S consumes the generator exactly like a cohort built from S alone -- the same patient order and, per patient, the same
    local rows (the gather is replaced by a host stand-in that records the index plan)."""
    from stamp_amd import ops
    S = [4, 1, 2]
    big, small = _stub_store([3, 9, 4, 2, 7]), _stub_store([7, 9, 4])
    seen = []

    def record(store, coords, idx, out_dtype, **kw):
        seen.append((idx.clone(), kw))
        return store[idx.clamp(min=0)], coords[idx.clamp(min=0)]

    monkeypatch.setattr(ops, "bag_batch_gather", record)
    a = list(big.view(S).train_batches(2, 5, generator=torch.Generator().manual_seed(7), vary_precision_bits=3)())
    plan_a, seen[:] = list(seen), []
    b = list(small.train_batches(2, 5, generator=torch.Generator().manual_seed(7), vary_precision_bits=3)())
    assert len(a) == len(b) == 2 and len(plan_a) == len(seen) == 2
    local = lambda store, members, idx, targets: [[(int(r) - store.offsets[members[int(t)]]) if r >= 0 else -1 for r in row]  # noqa: E731
                                                  for row, t in zip(idx.tolist(), targets.reshape(-1).tolist())]
    for (ba, (ia, kwa)), (bb, (ib, kwb)) in zip(zip(a, plan_a), zip(b, seen)):
        assert kwa == kwb and kwa["vary_precision_bits"] == 3
        assert torch.equal(ba[2], bb[2])                                                          # bag sizes
        assert [S[int(t)] for t in bb[3].reshape(-1)] == [int(t) for t in ba[3].reshape(-1)]      # the same patients in the same order
        assert local(big, list(range(5)), ia, ba[3]) == local(small, list(range(3)), ib, bb[3])  # the same rows of each patient
