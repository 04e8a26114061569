"""The concordance statistic's definition (tests/rank_oracle.py) against an independent restatement of lifelines' time-ordered sweep, its hand-worked
cases, the AUROC mapping against sklearn, the order keys of csrc/rank_metrics.hip restated in numpy, and the host-side refusals of the new entry points."""
import numpy as np
import pytest
import torch

import rank_oracle as R


@pytest.mark.parametrize("seed", range(6))
def test_definition_equals_the_time_ordered_sweep_under_heavy_ties(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 220))
    score, time, event = R.heavy_ties(n, 100 + seed, p_event=(0.15, 0.5, 0.9)[seed % 3])
    if seed == 5:                                   # untied, continuous data as well
        score, time = rng.standard_normal(n).astype(np.float32), rng.random(n).astype(np.float32)
    conc, tied, perm, valid = R.pair_counts(score, time, event)
    assert valid == n and (conc, tied, perm) == R.sweep_counts(score, time, event)
    assert perm > 0 and tied > 0 or seed == 5


def test_hand_worked_cases():
    t, e = [1, 2, 3], [1, 1, 1]
    assert R.pair_counts([3, 2, 1], t, e) == (3, 0, 3, 3) and R.c_of(R.pair_counts([3, 2, 1], t, e)) == 1.0
    assert R.pair_counts([1, 2, 3], t, e) == (0, 0, 3, 3) and R.c_of(R.pair_counts([1, 2, 3], t, e)) == 0.0
    assert R.pair_counts([5, 5, 5], t, e) == (0, 3, 3, 3) and R.c_of(R.pair_counts([5, 5, 5], t, e)) == 0.5
    # an earliest censored item starts no pair and ends none: the counts of the other two items alone
    assert R.pair_counts([9, 2, 1], [0, 2, 3], [0, 1, 1])[:3] == R.pair_counts([2, 1], [2, 3], [1, 1])[:3] == (1, 0, 1)
    # a death and a censoring at one time are a pair (the censored subject outlived the death) ...
    assert R.pair_counts([2, 1], [4, 4], [1, 0])[:3] == (1, 0, 1)
    # ... two deaths at one time are not
    assert R.pair_counts([2, 1], [4, 4], [1, 1])[:3] == (0, 0, 0) and np.isnan(R.c_of(R.pair_counts([2, 1], [4, 4], [1, 1])))
    for case in (([3, 2, 1], t, e), ([5, 5, 5], t, e), ([9, 2, 1], [0, 2, 3], [0, 1, 1]), ([2, 1], [4, 4], [1, 0]), ([2, 1], [4, 4], [1, 1])):
        assert R.pair_counts(*case)[:3] == R.sweep_counts(*case)
    # invalid items take part in no pair
    nan = float("nan")
    assert R.pair_counts([3, nan, 2, 1, 7, 7], [1, 1.5, 2, 3, nan, 2], [1, 1, 1, 1, 1, 2]) == (3, 0, 3, 3)


def test_auroc_is_the_same_statistic_as_sklearns_roc_auc_score():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(7)
    for n, levels in ((40, 4), (300, 8), (301, 1000)):
        y = rng.integers(0, 3, n)
        p = rng.integers(0, levels, (n, 3)).astype(np.float32) / levels          # tied scores
        for c in range(3):
            got = R.c_of(R.pair_counts(p[:, c], (y != c).astype(np.float32), (y == c).astype(np.uint8)))
            assert abs(got - sk.roc_auc_score(y == c, p[:, c])) < 1e-12, (n, levels, c)


def _key(x):
    """rk_key of csrc/rank_metrics.hip: fp32 -> uint32 in fp32's order, -0 and +0 on one key."""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = np.where((b << np.uint64(1)) & np.uint64(0xFFFFFFFF) == 0, np.uint64(0), b)
    return np.where(b & np.uint64(0x80000000) != 0, ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def test_order_keys_of_the_kernel_restate_the_fp32_compares():
    """The kernel tests permissibility with ONE unsigned compare ki < kj (ki = key(time_i) for an event, 2^32 - 1 otherwise; kj = key(time_j) + (event_j == 0),
    0 for an invalid item) and compares score keys: over signed zeros, denormals, infinities and ties this equals the definition's fp32 compares."""
    tiny = np.float32(1e-45)
    vals = np.array([-np.inf, -3.5, -1.0, -tiny, -0.0, 0.0, tiny, np.float32(1.17549435e-38), 1.0, np.nextafter(np.float32(1), np.float32(2)), 3.5, np.inf], np.float32)
    k = _key(vals)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(k[:, None] < k[None, :], vals[:, None] < vals[None, :]) and np.array_equal(k[:, None] == k[None, :], vals[:, None] == vals[None, :])
    assert int(k.max()) + 1 < 0xFFFFFFFF and int(k.min()) > 0
    rng = np.random.default_rng(3)
    n = 400
    score, time, event = rng.choice(vals, n), rng.choice(vals, n), rng.integers(0, 2, n).astype(np.uint8)
    score[::17], time[::19], event[::23] = np.nan, np.nan, 7
    ok = R.valid_mask(score, time, event)
    ki = np.where(ok & (event == 1), _key(time), np.uint64(0xFFFFFFFF))
    kj = np.where(ok, _key(time) + (event == 0), np.uint64(0))
    ks = _key(score)
    perm = ki[:, None] < kj[None, :]
    got = (int((perm & (ks[:, None] > ks[None, :])).sum()), int((perm & (ks[:, None] == ks[None, :])).sum()), int(perm.sum()), int(ok.sum()))
    assert got == R.pair_counts(score, time, event) and got[2] > 0


def test_metrics_and_fit_refuse_what_they_do_not_serve():
    from stamp_amd import metrics, mil_train

    with pytest.raises(RuntimeError, match="GPU"):
        metrics.concordance_index(torch.zeros(3), torch.arange(3.0), torch.ones(3))
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.multiclass_auroc(torch.full((4, 2), 0.5), torch.tensor([0, 1, 0, 1]))
    with pytest.raises(ValueError, match="monitor"):
        mil_train.fit(object(), lambda: (), lambda: (), max_epochs=1, monitor="val_auc")
    with pytest.raises(ValueError, match="valid_auroc"):
        mil_train.fit(object(), lambda: (), lambda: (), max_epochs=1, loss_fn=lambda a, b: a.sum(), valid_auroc=True)
