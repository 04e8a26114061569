"""The definition of the curve statistics (tests/curve_oracle.py = include/amdstamp.h, amds_binary_curves) on the CPU: hand-worked cases, the measured
distance to sklearn + np.interp with its knife edges, and the host-side refusals of the library (no kernel runs here).

Bars.  AP and the PR area are sums of at most 400 float64 terms <= 1 formed in another order than sklearn's: 1e-12.  A grid value is one interpolation of
float64 ratios: 1e-9 leaves six orders of room above its rounding, so a larger difference is never rounding -- it is a grid point that coincides with a
curve point as a rational (k * N == FP_t * (G - 1) or k * P == TP_t * (G - 1)), where numpy's k * (1 / (G - 1)) and sklearn's fps / fps[-1] may or may not
compare equal and np.interp lands on either side of a step.  Only such points may differ, and at most 1e-3 of all compared points."""

import numpy as np
import pytest

import curve_oracle as O

G = 1000


def test_hand_worked_cases():
    # perfect ranking: every positive above every negative
    r = O.curves([4, 3, 2, 1], [1, 1, 0, 0], grid=3)
    assert r["counts"] == (2, 2) and r["ap"] == 1.0 and r["pr_area"] == 1.0
    assert r["roc"].tolist() == [1.0, 1.0, 1.0]                       # np.interp takes the top of the vertical step at x = 0
    assert r["pr"].tolist() == [1.0, 1.0, 0.5] and r["pr_area_grid"] == 0.25 * 2.0 + 0.25 * 1.5          # the last point: most false positives
    # reversed ranking: thresholds 4, 3 take the negatives first -> TP = 0, 0, 1, 2; FP = 1, 2, 2, 2
    r = O.curves([4, 3, 2, 1], [0, 0, 1, 1], grid=3)
    assert r["ap"] == 0.5 * (1 / 3) + 0.5 * (2 / 4)
    assert r["pr_area"] == 0.5 * (1 / 3 + 0.0) / 2 + 0.5 * (1 / 3 + 0.5) / 2
    assert r["roc"].tolist() == [0.0, 0.0, 1.0]
    assert r["pr"].tolist() == [0.0, 1 / 3, 0.5]                      # top-scoring negatives: the PR grid starts at 0, not 1
    # all scores tied: one threshold, one curve point (P, N)
    r = O.curves([0.5] * 5, [1, 0, 0, 1, 0], grid=5)
    assert r["ap"] == 2 / 5 and r["roc"].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert r["pr"].tolist() == [1.0, 1.0 + 0.25 * (0.4 - 1.0), 1.0 + 0.5 * (0.4 - 1.0), 1.0 + 0.75 * (0.4 - 1.0), 0.4]
    assert r["pr_area"] == (1.0 + 0.4) / 2
    # ties inside a ranking, weights, invalid items, signed zeros
    a = O.curves([0.9, 0.5, 0.5, 0.1], [1, 1, 0, 0], grid=0)
    assert a["ap"] == 0.5 * 1.0 + 0.5 * (2 / 3) and np.isnan(a["pr_area_grid"]) and a["roc"].size == 0
    b = O.curves([0.9, 0.5, 0.5, 0.1, np.nan, 0.7, 0.2], [1, 1, 0, 0, 1, 2, 255], grid=0)
    assert b["ap"] == a["ap"] and b["counts"] == (2, 2)
    w = O.curves([0.9, 0.5, 0.1], [1, 0, 1], grid=7, weight=[2, 0, 1])          # a score without weight is no threshold
    assert w["counts"] == (3, 0) and np.isnan(w["ap"])
    z = O.curves(np.array([0.0, -0.0, 1.0], np.float32), [1, 0, 0], grid=0)      # -0 == +0: one tie group
    assert z["ap"] == 1 / 3
    # undefined problems: NaN everywhere, the counts stay
    for lab, counts in (([0, 0, 0], (0, 3)), ([1, 1, 1], (3, 0)), ([2, 2, 2], (0, 0))):
        r = O.curves([1, 2, 3], lab, grid=4)
        assert r["counts"] == counts and np.isnan([r["ap"], r["pr_area"], r["pr_area_grid"]]).all() and np.isnan(r["roc"]).all() and np.isnan(r["pr"]).all()


def probe_problems():
    """The recipe the header's knife-edge counts were measured on: seeded, n 5..399, 3..199 score levels in sixteenths, every second problem a bootstrap
    multiset of itself; a problem left with one class is dropped (298 of 300 remain)."""
    rng = np.random.default_rng(0)
    out = []
    for trial in range(300):
        n = int(rng.integers(5, 400))
        s = (rng.integers(0, rng.integers(3, 200), n) / 16).astype(np.float32)
        y = (rng.random(n) < rng.uniform(0.1, 0.9)).astype(np.int64)
        idx = rng.integers(0, n, n)
        w = np.bincount(idx, minlength=n).astype(np.int64) if trial % 2 else np.ones(n, np.int64)
        ys, ss = (y[idx], s[idx]) if trial % 2 else (y, s)
        if len(np.unique(ys)) == 2:
            out.append((s, y, w, ss, ys))
    return out


def test_distance_to_sklearn_and_np_interp_on_the_probe_problems():
    sk = pytest.importorskip("sklearn.metrics")
    problems = probe_problems()
    assert len(problems) == 298
    grid = np.linspace(0, 1, G)
    worst = {"ap": 0.0, "pr_area": 0.0, "pr_area_grid": 0.0}
    far = {"roc": 0, "pr": 0}
    for s, y, w, ss, ys in problems:
        got = O.curves(s, y, grid=G, weight=w)
        again = O.curves(ss, ys, grid=G)                                            # the multiset, gathered: the same integers, the same values
        assert got["counts"] == again["counts"] == (int(ys.sum()), int((1 - ys).sum()))
        assert got["ap"] == again["ap"] and np.array_equal(got["roc"], again["roc"]) and np.array_equal(got["pr"], again["pr"])
        precision, recall, _ = sk.precision_recall_curve(ys, ss)
        fpr, tpr, _ = sk.roc_curve(ys, ss)
        ref = {"roc": np.interp(grid, fpr, tpr), "pr": np.interp(grid, recall[::-1], precision[::-1])}
        worst["ap"] = max(worst["ap"], abs(got["ap"] - sk.average_precision_score(ys, ss)))
        worst["pr_area"] = max(worst["pr_area"], abs(got["pr_area"] - sk.auc(recall, precision)))
        edge = dict(zip(("roc", "pr"), O.knife_edges(s, y, G, weight=w)))
        ok_area = True
        for kind in ("roc", "pr"):
            d = np.abs(got[kind] - ref[kind]) > 1e-9
            assert not (d & ~edge[kind]).any(), (kind, np.flatnonzero(d & ~edge[kind]))          # away from a knife edge: rounding only
            far[kind] += int(d.sum())
            ok_area &= kind == "roc" or not d.any()
        if ok_area:                                                                  # (a grid without a flipped point: its trapezoid is rounding away too)
            worst["pr_area_grid"] = max(worst["pr_area_grid"], abs(got["pr_area_grid"] - sk.auc(grid, ref["pr"])))
    compared = len(problems) * G
    print(f"curve statistics against sklearn + np.interp on {len(problems)} problems, {compared} grid points per curve: max |dAP| {worst['ap']:.2e}, "
          f"max |dPR area| {worst['pr_area']:.2e}, max |d gridded PR area| {worst['pr_area_grid']:.2e}; grid points more than 1e-9 apart: "
          f"ROC {far['roc']}, PR {far['pr']} (all at knife edges)")
    assert worst["ap"] < 1e-12 and worst["pr_area"] < 1e-12 and worst["pr_area_grid"] < 1e-12
    assert far["roc"] <= 1e-3 * compared and far["pr"] <= 1e-3 * compared


# ---- the library's host side --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from stamp_amd import _lib
    return _lib.lib()


def _refused(lib, size, text):
    assert size == 0 and text in lib.amds_last_error(), (size, lib.amds_last_error())


def test_workspace_sizes_and_refused_shapes(lib):
    size = lib.amds_binary_curves_workspace_bytes
    # rank codes (4 bytes per base item, to 256) + the out-of-range counts (8 bytes per problem and one total, to 256); positions in LDS up to 12288
    assert size(0, 1, 1, 0) == 256 + 256
    assert size(0, 1000, 3, 1000) == 12032 + 256
    assert size(10000, 10000, 1000, 1000) == 40192 + 8192
    assert size(211, 300, 37, 1000) == 1024 + 512
    assert size(0, 12288, 2, 2) == 98304 + 256
    assert size(0, 12289, 2, 2) == 98560 + 196864 + 256          # above: the two count arrays of every problem live in the workspace
    assert size(0, 1 << 20, 1, 4096) > 0 and size(1 << 20, 1, 1, 4096) > 0
    _refused(lib, size(0, 0, 1, 1000), b"n_items=0 outside [1, 1048576]")
    _refused(lib, size(0, (1 << 20) + 1, 1, 1000), b"n_items=1048577 outside [1, 1048576]")
    _refused(lib, size(0, 10, 0, 1000), b"n_problems >= 1 and n_problems * n_items < 2^31")
    _refused(lib, size(0, 1 << 20, 2048, 1000), b"n_problems * n_items < 2^31")
    _refused(lib, size((1 << 20) + 1, 10, 1, 1000), b"n_base=1048577 outside [1, 1048576]")
    _refused(lib, size(-1, 10, 1, 1000), b"n_base=-1")
    _refused(lib, size(0, 10, 1, 1), b"grid=1: needs 0 or 2 <= grid <= 4096")
    _refused(lib, size(0, 10, 1, 4097), b"grid=4097: needs 0 or 2 <= grid <= 4096")
    _refused(lib, size(0, 10, 1, -3), b"grid=-3")


def test_call_refuses_null_misaligned_and_short_workspaces_before_any_launch(lib):
    """Made-up addresses: every refusal here comes before the first launch, so none is ever dereferenced."""
    call, err = lib.amds_binary_curves, lib.amds_last_error
    need = lib.amds_binary_curves_workspace_bytes(0, 100, 2, 1000)
    a = 0x10000                                                       # 256-byte aligned

    def args(**kw):
        d = dict(score=a, s_item=1, s_prob=100, label=a, l_prob=0, idx=None, n_base=0, n=100, P=2, grid=1000, counts=a, scalars=a, roc=a, pr=a, ws=a,
                 ws_bytes=need, stream=None)
        d.update(kw)
        return tuple(d.values())

    for name in ("score", "label", "counts", "scalars", "ws"):
        assert call(*args(**{name: None})) == -1 and b"null pointer" in err(), name
    assert call(*args(ws=a + 16)) == -1 and b"workspace not 256-byte aligned" in err()
    assert call(*args(ws_bytes=need - 1)) == -2 and b"workspace %d < required %d bytes" % (need - 1, need) in err()
    assert call(*args(ws_bytes=0)) == -2
    assert call(*args(grid=0)) == -1 and b"grid=0 with a grid output" in err()
    assert call(*args(grid=1)) == -1 and b"grid=1" in err()
    assert call(*args(n=0)) == -1 and b"n_items=0" in err()
    assert call(*args(s_item=0)) == -1 and b"bad strides" in err()
    assert call(*args(l_prob=-1)) == -1 and b"bad strides" in err()
    assert call(*args(idx=a, n_base=0)) == -1 and b"n_base=0 outside" in err()
