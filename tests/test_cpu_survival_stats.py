"""tests/survival_oracle.py on hand-worked cases and on the published Freireich 6-MP trial, the erfc form of the chi-square tail against scipy, the
regression oracle against sklearn and scipy, the device-free halves of stamp_amd.metrics (cut-off, chi2 / p, the numbers formed from the moments) against
the oracle, and the host-side refusals of the two new entry points."""
import math
from fractions import Fraction as F

import numpy as np
import pytest
import torch

import rank_oracle as R
import survival_oracle as O

HALF = 0.5          # the cut-off of the hand-worked cases: scores 0.9 are HIGH, 0.1 LOW
HI, LO = 0.9, 0.1


def test_one_death():
    """HIGH dies at 1, LOW is censored at 2.  t = 1: n = 2, n_H = 1, d = 1 -> E = 1/2, V = 1 * 1 / 1 * 1/2 * 1/2 = 1/4; O = 1; chi2 = (1/2)^2 / (1/4) = 1."""
    w = O.survival([HI, LO], [1, 2], [1, 0], HALF, grid=[0.5, 1, 2, np.nan])
    assert w["exact"] == (1, F(1, 2), F(1, 4)) and w["chi2"] == 1.0 and w["p"] == pytest.approx(math.erfc(math.sqrt(0.5)), rel=1e-15)
    assert w["counts"] == [(1, 0, 1), (1, 1, 0)] and w["pairs"] == 1 and w["median"] == [math.inf, 1.0]
    np.testing.assert_array_equal(w["km"], [[1, 1, 1, np.nan], [1, 0, 0, np.nan]])
    assert w["table"].tolist() == [[[1, 0, 0], [1, 0, 0], [1, 0, 1], [-1, -1, -1]], [[1, 0, 0], [1, 1, 0], [0, 1, 0], [-1, -1, -1]]]


def test_two_items_dying_together_have_no_variance():
    """One death in each group at the same time: n = d = 2 -> E = 2 * 1/2 = 1 = O and d (n - d) = 0 -> V = 0: chi2 0, p 1."""
    w = O.survival([HI, LO], [1, 1], [1, 1], HALF)
    assert w["exact"] == (1, 1, 0) and w["chi2"] == 0.0 and w["p"] == 1.0 and w["pairs"] == 0 and w["median"] == [1.0, 1.0]


def test_a_death_tied_with_a_censoring():
    """times 2 (HIGH, death), 2 (LOW, censored), 3 (LOW, death).  t = 2: n = 3, n_H = 1, d = 1 -> E = 1/3, V = 1 * 2 / 2 * 1/3 * 2/3 = 2/9; t = 3: n = 1 adds
    nothing; chi2 = (2/3)^2 / (2/9) = 2.  The item censored at 2 is at risk at 2 (S_LOW stays 1 there).  One comparable pair (the death at 2 against the
    item at 3), where the concordance statistic has two permissible pairs: it also counts (death, censored) at one time."""
    s, t, e = [HI, LO, LO], [2, 2, 3], [1, 0, 1]
    w = O.survival(s, t, e, HALF, grid=[2, 3])
    assert w["exact"] == (1, F(1, 3), F(2, 9)) and w["chi2"] == pytest.approx(2.0, rel=1e-15)
    np.testing.assert_array_equal(w["km"], [[1, 0], [0, 0]])
    assert w["pairs"] == 1 and R.pair_counts(s, t, e)[2] == 2 and w["median"] == [3.0, 2.0]
    assert w["table"].tolist() == [[[2, 0, 1], [1, 1, 1]], [[1, 1, 0], [0, 1, 0]]]


def test_a_group_that_dies_out():
    """HIGH dies at 1 and 2, LOW is censored at 3 and 4.  t = 1: n = 4, n_H = 2 -> E 1/2, V 1/4; t = 2: n = 3, n_H = 1 -> E 1/3, V 2/9.  S_HIGH = 1/2, then
    exactly 0; the median is the first time at which S <= 1/2, here t = 1 with S = 1/2 exactly."""
    w = O.survival([HI, HI, LO, LO], [1, 2, 3, 4], [1, 1, 0, 0], HALF, grid=[0, 1, 1.5, 2, 5])
    assert w["exact"] == (2, F(5, 6), F(17, 36)) and w["chi2"] == float(F(49, 36) / F(17, 36))
    np.testing.assert_array_equal(w["km"], [[1, 1, 1, 1, 1], [1, 0.5, 0.5, 0, 0]])
    assert w["median"] == [math.inf, 1.0] and w["pairs"] == 3 + 2


def test_no_death_no_variance_and_an_empty_group():
    w = O.survival([HI, HI, LO], [1, 2, 3], [0, 0, 0], HALF)
    assert w["exact"] == (0, 0, 0) and w["chi2"] == 0.0 and w["p"] == 1.0 and w["median"] == [math.inf, math.inf]
    w = O.survival([HI, HI], [1, 2], [1, 0], HALF, grid=[1])
    assert w["exact"] is None and all(math.isnan(w[k]) for k in ("O", "E", "V", "chi2", "p"))
    assert np.isnan(w["km"][0]).all() and w["km"][1].tolist() == [0.5] and math.isnan(w["median"][0]) and w["median"][1] == 1.0
    # a score equal to the cut-off is LOW; the default cut-off is the median, the midpoint for an even count
    assert O.survival([0.5, 0.7], [1, 2], [1, 1], 0.5)["counts"] == [(1, 1, 0), (1, 1, 0)]
    assert O.survival([1, 2, 3, 4], [1, 2, 3, 4], [1, 1, 1, 1])["cut_off"] == 2.5 and O.survival([1, 2, 3], [1, 2, 3], [1, 1, 1])["cut_off"] == 2.0


def test_freireich_6mp_trial():
    """Freireich et al. 1963, 21 against 21 (remission weeks; Kleinbaum & Klein, Survival Analysis, table 1.1): the log-rank chi2 is 16.79 in print."""
    mp6 = [(6, 1), (6, 1), (6, 1), (6, 0), (7, 1), (9, 0), (10, 1), (10, 0), (11, 0), (13, 1), (16, 1), (17, 0), (19, 0), (20, 0), (22, 1), (23, 1), (25, 0),
           (32, 0), (32, 0), (34, 0), (35, 0)]
    placebo = [1, 1, 2, 2, 3, 4, 4, 5, 5, 8, 8, 8, 8, 11, 11, 12, 12, 15, 17, 22, 23]
    time = [t for t, _ in mp6] + placebo
    event = [e for _, e in mp6] + [1] * 21
    w = O.survival([LO] * 21 + [HI] * 21, time, event, HALF)
    assert w["counts"] == [(21, 9, 12), (21, 21, 0)] and w["O"] == 21.0
    assert abs(w["chi2"] - 16.79) < 5e-3 and w["E"] == pytest.approx(10.75, abs=5e-3)
    assert w["median"] == [23.0, 8.0]


def test_chi_square_tail_is_the_erfc_form():
    st = pytest.importorskip("scipy.stats")
    for x in (0.0, 1e-12, 0.3, 1.0, 3.841458820694124, 16.79, 100.0, 700.0, 900.0):
        assert math.erfc(math.sqrt(x / 2)) == pytest.approx(float(st.chi2.sf(x, 1)), rel=1e-12)


def _reg_case(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.uniform(1, 3, n).astype(np.float32)
    return t, (0.8 * t + rng.normal(0, 0.3, n) + 0.5).astype(np.float32)


def test_regression_oracle_is_sklearn_and_scipy():
    sk = pytest.importorskip("sklearn.metrics")
    st = pytest.importorskip("scipy.stats")
    for n, seed in ((2, 1), (3, 2), (50, 3), (501, 4)):
        t, p = _reg_case(n, seed)
        if n > 3:
            t[5], p[7] = np.nan, np.nan
        ok = ~(np.isnan(t) | np.isnan(p))
        t64, p64 = t[ok].astype(np.float64), p[ok].astype(np.float64)
        w = O.regression(O.moments(t, p))
        assert w["count"] == ok.sum()
        assert w["r2_score"] == pytest.approx(sk.r2_score(t64, p64), rel=1e-12) and w["mae"] == pytest.approx(sk.mean_absolute_error(t64, p64), rel=1e-12)
        assert w["rmse"] == pytest.approx(math.sqrt(sk.mean_squared_error(t64, p64)), rel=1e-12)
        assert w["pearson_r"] == pytest.approx(float(st.pearsonr(t64, p64)[0]), rel=1e-12)
        line = st.linregress(t64, p64)
        assert w["slope"] == pytest.approx(line.slope, rel=1e-12) and w["intercept"] == pytest.approx(line.intercept, rel=1e-12, abs=1e-12)
        assert w["stderr"] == pytest.approx(line.stderr, rel=1e-12)          # (exactly 0 for two rows)
    const = O.regression(O.moments(np.full(5, 2.0), [1, 2, 3, 4, 5]))
    assert math.isnan(const["pearson_r"]) and const["r2_score"] == 0.0 and math.isnan(const["slope"])
    assert math.isnan(O.regression(O.moments([1, 2, 3], np.full(3, 7.0)))["pearson_r"])


def test_the_device_free_halves_of_metrics_equal_the_oracle():
    from stamp_amd import metrics
    for n, seed in ((1, 0), (2, 1), (7, 2), (8, 3), (60, 4)):
        s, t, e = R.heavy_ties(n, seed)
        s = s + np.float32(0.01) * np.arange(n, dtype=np.float32)
        if n > 3:
            s[1], t[2], e[3] = np.nan, np.nan, 255
        cut = metrics._median_cut_off(torch.from_numpy(s), torch.from_numpy(t), torch.from_numpy(e))
        want = O.median_cut_off(s, t, e)
        assert cut.dtype == torch.float64 and (cut.item() == want or (math.isnan(want) and cut.isnan().all()))
        w = O.survival(s, t, e)
        chi2, p = metrics._chi2_p(*[torch.tensor([w[k]], dtype=torch.float64) for k in "OEV"])
        np.testing.assert_allclose(chi2.numpy(), [w["chi2"]], rtol=1e-14, equal_nan=True)
        np.testing.assert_allclose(p.numpy(), [w["p"]], rtol=1e-12, equal_nan=True)
    for tp in (_reg_case(2, 5), _reg_case(300, 6), (np.full(5, 2.0, np.float32), np.arange(5, dtype=np.float32)), _reg_case(1, 7)):
        m = O.moments(*tp)
        got, want = metrics.regression_from_moments(torch.tensor([m], dtype=torch.float64)), O.regression(m)
        for k in metrics.REGRESSION_KEYS:
            np.testing.assert_allclose(float(got[k][0]), want[k], rtol=1e-13, equal_nan=True, err_msg=k)


def test_metrics_and_entry_points_refuse_what_they_do_not_serve():
    from stamp_amd import _lib, metrics
    s, t, e = torch.rand(6), torch.arange(6.0), torch.ones(6)
    for call in (lambda: metrics.survival_groups(s, t, e), lambda: metrics.logrank_test(s, t, e), lambda: metrics.kaplan_meier(s, t, e),
                 lambda: metrics.survival_stats(s, t, e), lambda: metrics.bootstrap_survival(s, t, e, n_resamples=2),
                 lambda: metrics.regression_stats(s, t), lambda: metrics.bootstrap_regression(s, t, n_resamples=2), lambda: metrics.regression_moments(s, t)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    lib = _lib.lib()
    size = lib.amds_survival_groups_workspace_bytes
    assert size(0, 100, 3, 256, 1) > 0 and size(0, 100, 3, 256, 1) % 256 == 0
    for bad in ((0, 0, 1, 0, 1), (0, (1 << 20) + 1, 1, 0, 1), (0, 5, 0, 0, 1), (-1, 5, 1, 0, 1), ((1 << 20) + 1, 5, 1, 0, 1), (0, 5, 1, 1, 1), (0, 5, 1, 4097, 1),
                (0, 1 << 20, 2048, 0, 1)):
        assert size(*bad) == 0, bad
    assert b"n_problems * n_items < 2^31" in lib.amds_last_error()
    # the count arrays of a problem move from LDS to the workspace above 5000 positions (include/amdstamp.h): 32 bytes per position and problem
    assert size(0, 5001, 2, 0, 1) - size(0, 5000, 2, 0, 1) >= 2 * 5000 * 32
    assert size(5000, 100, 7, 0, 1) == size(5000, 100, 1, 0, 1)          # (both round the bad-index counts up to 256 bytes)
    rsize = lib.amds_regression_moments_workspace_bytes
    assert rsize(0, 70001, 3) == 256 and rsize(0, 0, 1) == 0 and rsize(0, 5, 0) == 0 and rsize(-1, 5, 1) == 0 and rsize(0, 1 << 31, 1) == 0
    # a NULL pointer is refused before anything is launched
    assert lib.amds_survival_groups(None, 1, 0, None, 0, None, 0, None, 0, None, 0, 5, 1, None, 0, 0, None, None, None, None, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.amds_last_error()
    assert lib.amds_regression_moments(None, 1, 0, None, 1, 0, None, 0, 5, 1, None, None, 0, None) == -1 and b"null pointer" in lib.amds_last_error()
