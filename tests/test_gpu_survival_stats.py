"""amds_survival_groups, amds_regression_moments and the stamp_amd.metrics functions over them on the GPU, against tests/survival_oracle.py (exact
rationals for the log-rank sums and the Kaplan-Meier products, brute force for the tables, medians and pairs, exactly rounded float64 sums for the
regression moments; itself pinned by tests/test_cpu_survival_stats.py), and the C-ABI contract (reproducible, poisoned workspace, guard bands, NULL grids,
refusals).

Bars.  Counts, tables, pairs, medians and O are integers or times: equality.  E, V and every positive S are sums / products of at most n <= 2^20 float64
terms in a fixed order, each term a correctly rounded ratio of integers: the relative error is at most about n * 2^-53 <= 1.2e-10 at the limit and
5001 * 2^-53 = 5.6e-13 at the sizes here, so 1e-11 leaves an order of magnitude.  S is exactly 0 where the oracle's is 0.  p = erfc(sqrt(chi2 / 2)) has
the condition number chi2 * exp(-chi2 / 2) / (sqrt(2 pi chi2) * p) ~ chi2 / 2 + 1/2 <= 460 down to p = 1e-200, so 1e-9 holds there with chi2 at 1e-11
and an erfc good to 1e-12.  The regression moments are sums of n <= 70001 non-negative or well-conditioned terms against exactly rounded sums: 1e-12."""
import math

import numpy as np
import pytest
import torch

import guarded as G
import rank_oracle as R
import survival_oracle as O

pytestmark = pytest.mark.gpu

RTOL, P_RTOL, M_RTOL = 1e-11, 1e-9, 1e-12
LDS_ITEMS = 5000          # include/amdstamp.h: the arrays of a problem live in LDS up to 5000 positions


def _dev(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _distinct(n, seed):
    """Scores without ties, every time its own (a permutation plus a half), random events."""
    rng = np.random.default_rng(seed)
    return rng.random(n).astype(np.float32), (rng.permutation(n) + 0.5).astype(np.float32), (rng.random(n) < 0.6).astype(np.uint8)


def _grid_for(t, G_):
    """G_ times from below the first to beyond the last, the first half of them exact item times."""
    ok = t[~np.isnan(t)]
    if len(ok) == 0:
        ok = np.zeros(1, np.float32)
    lin = np.linspace(float(ok.min()) - 1.0, float(ok.max()) + 1.0, G_ - G_ // 2)
    return np.concatenate([np.sort(ok)[np.linspace(0, len(ok) - 1, G_ // 2).astype(int)], lin]).astype(np.float32)


def _check(res, wants, grid=None):
    """res: a SurvivalGroups of len(wants) problems; wants: the oracle's dicts."""
    from stamp_amd import metrics
    P = len(wants)
    assert res.counts.dtype == torch.int64 and res.counts.cpu().tolist() == [[list(c) for c in w["counts"]] for w in wants]
    for k, w in enumerate(wants):
        if w["pairs"] is not None:
            assert int(res.pairs[k]) == w["pairs"], ("pairs", k)
    for name, key, rtol in (("observed", "O", 0), ("expected", "E", RTOL), ("variance", "V", RTOL)):
        got = getattr(res, name)
        assert got.dtype == torch.float64 and got.device.type == "cuda" and tuple(got.shape) == (P,)
        np.testing.assert_allclose(got.cpu().numpy(), [w[key] for w in wants], rtol=rtol, atol=0, equal_nan=True, err_msg=name)
    chi2, p = metrics._chi2_p(res.observed, res.expected, res.variance)
    for k, w in enumerate(wants):
        print(f"problem {k}: O {float(res.observed[k])!r} E {float(res.expected[k])!r} / {w['E']!r} V {float(res.variance[k])!r} / {w['V']!r} "
              f"p {float(p[k])!r} / {w['p']!r}")
        if math.isnan(w["p"]):
            assert p[k].isnan() and chi2[k].isnan()
        elif w["p"] >= 1e-200:
            assert abs(float(p[k]) - w["p"]) <= P_RTOL * w["p"], (k, float(p[k]), w["p"])
    np.testing.assert_array_equal(res.median.cpu().numpy(), np.array([w["median"] for w in wants]), err_msg="median")
    if grid is None:
        assert res.km is None and res.at_risk is None
        return
    km, want_km = res.km.cpu().numpy(), np.stack([w["km"] for w in wants])
    assert res.km.dtype == torch.float64 and km.shape == want_km.shape == (P, 2, grid)
    assert np.array_equal(np.isnan(km), np.isnan(want_km)) and np.array_equal(km == 0.0, want_km == 0.0)          # exactly 0 where the oracle's is 0
    pos = want_km > 0
    np.testing.assert_allclose(km[pos], want_km[pos], rtol=RTOL, atol=0, err_msg="km")
    assert res.at_risk.dtype == torch.int64 and np.array_equal(res.at_risk.cpu().numpy(), np.stack([w["table"] for w in wants]))


@pytest.mark.parametrize("kind", ["ties", "distinct"])
@pytest.mark.parametrize("n", [1, 2, 3, 257, 4099])
def test_log_rank_curves_tables_and_medians_equal_the_oracle(gpu, n, kind):
    """Integer times 0..9 with scores on 8 levels (the median cut-off then EQUALS a score: those items are LOW), and distinct times; the default cut-off."""
    from stamp_amd import metrics
    s, t, e = R.heavy_ties(n, 7 * n) if kind == "ties" else _distinct(n, 7 * n + 1)
    grid = _grid_for(t, 34)
    res = metrics.survival_groups(_dev(gpu, s), _dev(gpu, t), _dev(gpu, e), grid_times=_dev(gpu, grid))
    want = O.survival(s, t, e, grid=grid)
    assert float(res.cut_off[0]) == want["cut_off"]
    _check(res, [want], 34)
    _check(metrics.survival_groups(_dev(gpu, s), _dev(gpu, t), _dev(gpu, e)), [want])
    if n == 1:
        assert res.observed.isnan().all() and res.km[0, 1].isnan().all() and not res.km[0, 0].isnan().any()          # one item: HIGH is empty


@pytest.mark.parametrize("n", [LDS_ITEMS, LDS_ITEMS + 1])
def test_the_threshold_between_lds_and_workspace_arrays(gpu, n):
    """Both sides of the header's threshold, two problems in one call (times on 50 levels, so the positions run up to the end of the arrays), then resampled."""
    from stamp_amd import metrics
    rng = np.random.default_rng(n)
    s = rng.random((2, n)).astype(np.float32)
    t = rng.integers(0, 50, (2, n)).astype(np.float32)
    e = (rng.random((2, n)) < 0.5).astype(np.uint8)
    grid = np.stack([_grid_for(t[p], 20) for p in range(2)])
    res = metrics.survival_groups(_dev(gpu, s), _dev(gpu, t), _dev(gpu, e), grid_times=_dev(gpu, grid))
    _check(res, [O.survival(s[p], t[p], e[p], grid=grid[p]) for p in range(2)], 20)
    idx = rng.integers(0, n, (3, 1200)).astype(np.int32)
    cut = float(np.median(s[1]))
    res = metrics.survival_groups(_dev(gpu, s[1]), _dev(gpu, t[1]), _dev(gpu, e[1]), cut_off=cut, grid_times=_dev(gpu, grid[1]), idx=_dev(gpu, idx))
    _check(res, [O.survival(s[1][r], t[1][r], e[1][r], cut, grid=grid[1]) for r in idx], 20)


def test_invalid_items_signed_zeros_denormals_and_infinite_times(gpu):
    from stamp_amd import metrics
    rng = np.random.default_rng(3)
    n = 300
    vals = np.array([-1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32)
    s, t, e = rng.random(n).astype(np.float32), rng.choice(vals, n), (rng.random(n) < 0.7).astype(np.uint8)
    s[[0, 17, 255, 256]] = np.nan
    t[[1, 18, 254, n - 1]] = np.nan
    e[[2, 257]] = 255
    e[[3, 19]] = 2
    grid = np.array([-2.0, -1e-45, -0.0, 0.0, 1e-45, np.nan, 0.5, 1.0, np.inf], np.float32)
    want = O.survival(s, t, e, grid=grid)
    assert sum(c[0] for c in want["counts"]) == n - 12 and len(np.unique(t[R.valid_mask(s, t, e)])) == 6          # -0 and +0 are one time
    res = metrics.survival_groups(_dev(gpu, s), _dev(gpu, t), _dev(gpu, e), grid_times=_dev(gpu, grid))
    _check(res, [want], len(grid))
    assert res.km[0, :, 5].isnan().all() and bool((res.at_risk[0, :, 5] == -1).all())                              # the NaN grid time
    nan_event = np.where(e > 1, np.nan, e.astype(np.float32)).astype(np.float32)          # numbers: 0 and 1 are valid, everything else (NaN too) is not
    _check(metrics.survival_groups(_dev(gpu, s), _dev(gpu, t), _dev(gpu, nan_event), grid_times=_dev(gpu, grid)), [want], len(grid))
    # denormal scores on both sides of a denormal cut-off
    s2 = np.array([-1e-45, 0.0, 1e-45, 3e-45, 1e-45, 3e-45], np.float32)
    t2, e2 = np.arange(6, dtype=np.float32), np.ones(6, np.uint8)
    _check(metrics.survival_groups(_dev(gpu, s2), _dev(gpu, t2), _dev(gpu, e2), cut_off=float(np.float32(1e-45))), [O.survival(s2, t2, e2, float(np.float32(1e-45)))])


def test_empty_group_no_death_cut_off_rules_and_the_report_row(gpu):
    from stamp_amd import metrics
    s, t, e = R.heavy_ties(200, 5)
    sd, td, ed = _dev(gpu, s), _dev(gpu, t), _dev(gpu, e)
    lr = metrics.logrank_test(sd, td, ed, cut_off=2.0)                                    # every score is below 2: HIGH is empty
    assert lr.chi2.isnan().all() and lr.p.isnan().all() and lr.observed.isnan().all() and lr.expected.isnan().all() and lr.variance.isnan().all()
    km = metrics.kaplan_meier(sd, td, ed, cut_off=2.0)
    assert km.km[0, 1].isnan().all() and not km.km[0, 0].isnan().any() and km.median[0, 1].isnan() and km.counts[0, 1].tolist() == [0, 0, 0]
    lr = metrics.logrank_test(sd, td, torch.zeros_like(ed))                               # no death: V = 0 with both groups present
    assert lr.chi2.tolist() == [0.0] and lr.p.tolist() == [1.0] and lr.variance.tolist() == [0.0]
    g = metrics.survival_groups(sd, td, ed, cut_off=0.5)                                  # a score EQUAL to the cut-off is LOW
    assert g.counts[0, :, 0].tolist() == [int((s <= 0.5).sum()), int((s > 0.5).sum())] and (s == 0.5).any()
    for n in (6, 7):                                                                      # the median: the midpoint for an even count, computed on the device
        sc = np.random.default_rng(n).permutation(n).astype(np.float32)
        sc_nan = np.concatenate([sc, [np.nan]]).astype(np.float32)
        g = metrics.survival_groups(_dev(gpu, sc_nan), _dev(gpu, np.arange(n + 1, dtype=np.float32)), torch.ones(n + 1, device=gpu))
        assert g.cut_off.dtype == torch.float64 and g.cut_off.tolist() == [float(np.nanmedian(sc_nan.astype(np.float64)))] == [(n - 1) / 2]
        assert g.counts[0, :, 0].tolist() == [(n + 1) // 2, n // 2]
    # the default grid: 256 times from 0 to the largest valid time; the curves against the oracle on that grid
    km = metrics.kaplan_meier(sd, td, ed)
    np.testing.assert_array_equal(km.x.cpu().numpy(), (np.arange(256) / 255 * 9.0).astype(np.float32))
    want = O.survival(s, t, e, grid=km.x.cpu().numpy())
    np.testing.assert_allclose(km.km[0].cpu().numpy(), want["km"], rtol=RTOL)
    assert np.array_equal(km.at_risk[0].cpu().numpy(), want["table"]) and km.median[0].tolist() == want["median"]
    row = metrics.survival_stats(sd, td, ed)
    assert {k: v.dim() for k, v in row.items()} == dict.fromkeys(("c_index", "logrank_p", "count", "events", "censored", "comparable_pairs", "threshold"), 0)
    assert row["c_index"].item() == metrics.concordance_index(sd, td, ed).item() and abs(row["logrank_p"].item() - want["p"]) <= P_RTOL * want["p"]
    assert (row["count"].item(), row["events"].item(), row["censored"].item()) == (200, int(e.sum()), int((e == 0).sum()))
    assert row["comparable_pairs"].item() == want["pairs"] != R.pair_counts(s, t, e)[2] and row["threshold"].item() == want["cut_off"]


def test_three_problems_through_the_strides_with_their_own_cut_offs_and_grids(gpu):
    from stamp_amd import metrics
    rng = np.random.default_rng(8)
    n = 333
    p = rng.integers(0, 16, (n, 4)).astype(np.float32) / 16
    t = rng.integers(0, 12, (3, n)).astype(np.float32)
    e = (rng.random(n) < 0.6).astype(np.uint8)
    cuts = np.array([0.25, 0.5, 0.40625])
    grids = np.stack([_grid_for(t[c], 9) for c in range(3)])
    pd = _dev(gpu, p)
    res = metrics.survival_groups(pd[:, :3].t(), _dev(gpu, t), _dev(gpu, e), cut_off=_dev(gpu, cuts), grid_times=_dev(gpu, grids))          # item stride 4, problem stride 1
    _check(res, [O.survival(p[:, c], t[c], e, cuts[c], grid=grids[c]) for c in range(3)], 9)
    assert res.cut_off.tolist() == cuts.tolist()
    res = metrics.survival_groups(pd[:, :3].t(), _dev(gpu, t[0]), _dev(gpu, e), grid_times=_dev(gpu, grids[0]))                             # shared time and grid, median cut-offs
    _check(res, [O.survival(p[:, c], t[0], e, grid=grids[0]) for c in range(3)], 9)


def _resample_case():
    rng = np.random.default_rng(5)
    n, R_, m = 211, 37, 300
    s, t, e = R.heavy_ties(n, 21)
    s = (s + rng.integers(0, 3, n) / 32).astype(np.float32)
    idx = rng.integers(0, n, (R_, m)).astype(np.int32)
    idx[11] = np.flatnonzero(s <= 0.25)[rng.integers(0, int((s <= 0.25).sum()), m)]          # one resample forced into one group
    return s, t, e, idx


def test_resamples_equal_the_oracle_on_the_gathered_arrays(gpu):
    from stamp_amd import metrics
    s, t, e, idx = _resample_case()
    cut = O.median_cut_off(s, t, e)
    grid = _grid_for(t, 16)
    wants = [O.survival(s[r], t[r], e[r], cut, grid=grid) for r in idx]
    assert math.isnan(wants[11]["O"]) and sum(math.isnan(w["O"]) for w in wants) == 1
    sd, td, ed = _dev(gpu, s), _dev(gpu, t), _dev(gpu, e)
    res = metrics.survival_groups(sd, td, ed, grid_times=_dev(gpu, grid), idx=_dev(gpu, idx))          # the default cut-off: the WHOLE sample's median
    assert res.cut_off.tolist() == [cut] * 37
    _check(res, wants, 16)
    cuts = np.linspace(0.2, 0.7, 37)
    res = metrics.survival_groups(sd, td, ed, cut_off=_dev(gpu, cuts), idx=_dev(gpu, idx[:, :129].astype(np.int64)))
    _check(res, [O.survival(s[r], t[r], e[r], c) for r, c in zip(idx[:, :129], cuts)])
    for bad in ([[0, 1, 211]], [[0, -1, 2]]):
        with pytest.raises(RuntimeError, match="outside"):
            metrics.survival_groups(sd, td, ed, idx=torch.tensor(bad, device=gpu))
    with pytest.raises(ValueError, match="ONE problem"):
        metrics.survival_groups(sd[None].expand(2, -1), td, ed, idx=_dev(gpu, idx))
    with pytest.raises(ValueError, match="grid=1"):
        metrics.survival_groups(sd, td, ed, grid_times=torch.zeros(1, device=gpu))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.survival_groups(torch.from_numpy(s), torch.from_numpy(t), torch.from_numpy(e))


def test_bootstrap_survival_bands_are_the_quantiles_of_the_oracles_rows(gpu):
    """60 items, distinct scores, so the median splits them 30 / 30.  Under generator seed 1 the oracle leaves out none of the 200 resamples (a resample
    misses a group with probability 2 * 2^-60)."""
    from stamp_amd import metrics
    s, t, e = _distinct(60, 12)
    t = np.floor(t / 3).astype(np.float32)                                                # ties in time
    n_res, seed = 200, 1
    idx = torch.randint(0, 60, (n_res, 60), generator=torch.Generator().manual_seed(seed), dtype=torch.int32).numpy()
    full = O.survival(s, t, e)
    assert full["counts"][0][0] == full["counts"][1][0] == 30
    grid = (np.arange(32) / 31 * float(t.max())).astype(np.float32)
    wants = [O.survival(s[r], t[r], e[r], full["cut_off"], grid=grid) for r in idx]
    assert sum(math.isnan(w["O"]) for w in wants) == 0
    b = metrics.bootstrap_survival(_dev(gpu, s), _dev(gpu, t), _dev(gpu, e), n_resamples=n_res, generator=torch.Generator().manual_seed(seed), points=32)
    assert b.used == n_res == 200 and b.dropped_share == 0.0
    np.testing.assert_array_equal(b.x.cpu().numpy(), grid)
    point = O.survival(s, t, e, grid=grid)
    np.testing.assert_allclose(b.km.cpu().numpy(), point["km"], rtol=RTOL)
    lo, hi = np.quantile(np.stack([w["km"] for w in wants]), [0.025, 0.975], axis=0)
    # (a quantile moves by no more than the largest change of a row value: the rows' bar holds for the bands)
    np.testing.assert_allclose(b.band_lower.cpu().numpy(), lo, rtol=RTOL, atol=0)
    np.testing.assert_allclose(b.band_upper.cpu().numpy(), hi, rtol=RTOL, atol=0)
    chi = [w["chi2"] for w in wants]
    np.testing.assert_allclose([b.chi2.item(), b.chi2_lower.item(), b.chi2_upper.item()], [point["chi2"], *np.quantile(chi, [0.025, 0.975])], rtol=10 * RTOL)
    meds = np.array([w["median"] for w in wants])
    assert b.median.tolist() == point["median"]
    assert b.median_lower.tolist() == np.quantile(meds, 0.025, axis=0, method="lower").tolist()
    assert b.median_upper.tolist() == np.quantile(meds, 0.975, axis=0, method="higher").tolist()
    for v in b[:10]:
        assert v.device.type == "cuda"
    none = metrics.bootstrap_survival(_dev(gpu, s), _dev(gpu, t), _dev(gpu, e), cut_off=5.0, n_resamples=3, points=5)          # HIGH is empty everywhere
    assert none.used == 0 and none.dropped_share == 1.0 and none.chi2.isnan() and none.band_upper.isnan().all() and none.median_lower.isnan().all()


def _abi_case():
    n, P, grid, m, R_ = 1500, 3, 64, 700, 4
    rng = np.random.default_rng(9)
    cols = [R.heavy_ties(n, 90 + p, p_event=0.8) for p in range(P)]
    score = np.stack([c[0] + rng.integers(0, 4, n).astype(np.float32) / 64 for c in cols], axis=1)          # [n][P]: item stride P, problem stride 1
    time, event = np.stack([c[1] for c in cols]), np.stack([c[2] for c in cols])                             # [P][n]
    cuts = np.array([0.3, 0.45, 0.5])
    grids = np.stack([_grid_for(time[p], grid) for p in range(P)])
    idx = rng.integers(0, n, (R_, m)).astype(np.int32)
    return n, P, grid, m, R_, score, time, event, cuts, grids, idx


def test_c_abi_reproducible_poisoned_workspace_guard_bands_null_grids_and_refusals(gpu):
    """amds_survival_groups on workspaces of exactly the stated size inside guard bands, poisoned with 0x00 and with 0xFF, guard bands around every output:
    the same bits under both poisons and from two calls, the oracle's values, bands intact; NULL grids with grid = 0 change nothing else; every refusal of
    the header."""
    from stamp_amd import _lib
    lib = _lib.lib()
    n, P, grid, m, R_, score, time, event, cuts, grids, idx = _abi_case()
    nb, nb0, nb_idx = (lib.amds_survival_groups_workspace_bytes(0, n, P, grid, 0), lib.amds_survival_groups_workspace_bytes(0, n, P, 0, 1),
                       lib.amds_survival_groups_workspace_bytes(n, m, R_, grid, 1))
    assert nb > 0 and nb % 256 == 0 and 0 < nb0 < nb and nb_idx > 0
    wants = [O.survival(score[:, p], time[p], event[p], cuts[p], grid=grids[p]) for p in range(P)]
    wants_idx = [O.survival(score[r, 0], time[0][r], event[0][r], cuts[0], grid=grids[0]) for r in idx]
    assert all(np.isfinite(w["median"]).all() for w in wants + wants_idx)                 # (run_contract wants finite outputs)
    names = ("counts", "logrank", "median", "pairs", "km", "table")

    def call(pattern):
        b = G.Bufs(gpu, pattern)
        s, t, e = b.inp(torch.from_numpy(score), name="score"), b.inp(torch.from_numpy(time), name="time"), b.inp(torch.from_numpy(event), name="event")
        c, g, ix = b.inp(torch.from_numpy(cuts), name="cutoff"), b.inp(torch.from_numpy(grids), name="grid"), b.inp(torch.from_numpy(idx), name="idx")
        outs = {}

        def run(tag, ws_bytes, rows, G_, ixp, base, items, cp, gp):
            ws = b.out((ws_bytes,), torch.uint8, name="ws" + tag)
            o = dict(counts=b.out((rows, 6), torch.int64, name="counts" + tag), logrank=b.out((rows, 3), torch.float64, name="logrank" + tag),
                     median=b.out((rows, 2), torch.float64, name="median" + tag), pairs=b.out((rows,), torch.int64, name="pairs" + tag))
            if G_:
                o.update(km=b.out((rows, 2 * G_), torch.float64, name="km" + tag), table=b.out((rows, 6 * G_), torch.int64, name="table" + tag))
            _lib.check(lib.amds_survival_groups(s.data_ptr(), P, 0 if ixp else 1, t.data_ptr(), n, e.data_ptr(), n, c.data_ptr(), cp, ixp, base, items, rows,
                                                g.data_ptr() if G_ else None, gp, G_, o["counts"].data_ptr(), o["logrank"].data_ptr(), o["median"].data_ptr(),
                                                o["pairs"].data_ptr(), G.ptr(o.get("km")), G.ptr(o.get("table")), ws.data_ptr(), ws_bytes, G.cur_stream()),
                       "survival_groups" + tag)
            outs.update({k + tag: v for k, v in o.items()})

        run("0", nb, P, grid, None, 0, n, 1, grid)
        run("1", nb, P, grid, None, 0, n, 1, grid)
        run("_no_grid", nb0, P, 0, None, 0, n, 1, 0)
        run("_idx", nb_idx, R_, grid, ix.data_ptr(), n, m, 0, 0)
        return b.result(**outs)

    o = G.run_contract(call)
    for k in names:
        assert torch.equal(o[k + "0"], o[k + "1"]), k                                     # two calls: the same bits
    for k in names[:4]:
        assert torch.equal(o[k + "_no_grid"], o[k + "0"]), k
    for tag, ws_ in (("0", wants), ("_idx", wants_idx)):
        assert o["counts" + tag].reshape(-1, 2, 3).tolist() == [[list(c) for c in w["counts"]] for w in ws_]
        assert o["pairs" + tag].tolist() == [w["pairs"] for w in ws_] and o["median" + tag].tolist() == [w["median"] for w in ws_]
        np.testing.assert_allclose(o["logrank" + tag].cpu().numpy(), [[w["O"], w["E"], w["V"]] for w in ws_], rtol=RTOL)
        np.testing.assert_allclose(o["km" + tag].cpu().numpy().reshape(-1, 2, grid), np.stack([w["km"] for w in ws_]), rtol=RTOL)
        assert np.array_equal(o["table" + tag].cpu().numpy().reshape(-1, 2, grid, 3), np.stack([w["table"] for w in ws_]))

    # refusals: nothing is launched, so the poisoned outputs stay poisoned
    b = G.Bufs(gpu, 0xFF)
    s, t, e, c, g = (b.inp(torch.from_numpy(a)) for a in (score, time, event, cuts, grids))
    ws, cnt, lr, med = b.out((nb,), torch.uint8, name="ws"), b.out((P, 6), torch.int64, name="counts"), b.out((P, 3), torch.float64, name="logrank"), \
        b.out((P, 2), torch.float64, name="median")
    km = b.out((P, 2 * grid), torch.float64, name="km")

    def rc(*, s_=s.data_ptr(), t_=t.data_ptr(), e_=e.data_ptr(), c_=c.data_ptr(), ix_=None, base=0, n_=n, P_=P, g_=g.data_ptr(), gp=grid, G_=grid,
           cnt_=cnt.data_ptr(), lr_=lr.data_ptr(), med_=med.data_ptr(), km_=km.data_ptr(), ws_=ws.data_ptr(), nb_=nb, si=P, sp=1, tp=n, ep=n, cp=1):
        return lib.amds_survival_groups(s_, si, sp, t_, tp, e_, ep, c_, cp, ix_, base, n_, P_, g_, gp, G_, cnt_, lr_, med_, None, km_, None, ws_, nb_, G.cur_stream())

    assert rc(nb_=nb - 1) == -2 and b"workspace" in lib.amds_last_error()
    assert rc(ws_=ws.data_ptr() + 8) == -1
    for bad in (dict(s_=None), dict(t_=None), dict(e_=None), dict(c_=None), dict(cnt_=None), dict(lr_=None), dict(med_=None), dict(ws_=None), dict(n_=0),
                dict(P_=0), dict(si=0), dict(sp=-1), dict(tp=-1), dict(ep=-1), dict(cp=2), dict(cp=-1), dict(gp=-1), dict(G_=1), dict(G_=4097),
                dict(G_=0), dict(G_=0, g_=None), dict(g_=None), dict(ix_=s.data_ptr(), base=0), dict(ix_=s.data_ptr(), base=(1 << 20) + 1),
                dict(n_=(1 << 20) + 1), dict(n_=1 << 20, P_=2048)):
        assert rc(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((cnt == -1).all()) and bool(lr.isnan().all()) and bool(med.isnan().all()) and bool(km.isnan().all())
    # an out-of-range index fails the call (and is never dereferenced: the base problem ends where the guard band begins)
    bad_idx = idx.copy()
    bad_idx[2, 333] = n
    bad_idx[0, 0] = -5
    ix = b.inp(torch.from_numpy(bad_idx), name="bad idx")
    ws2, cnt2, lr2, med2 = b.out((nb_idx,), torch.uint8, name="ws_idx"), b.out((R_, 6), torch.int64, name="counts_idx"), \
        b.out((R_, 3), torch.float64, name="lr_idx"), b.out((R_, 2), torch.float64, name="med_idx")
    got = lib.amds_survival_groups(s.data_ptr(), P, 0, t.data_ptr(), 0, e.data_ptr(), 0, c.data_ptr(), 0, ix.data_ptr(), n, m, R_, None, 0, 0, cnt2.data_ptr(),
                                   lr2.data_ptr(), med2.data_ptr(), None, None, None, ws2.data_ptr(), nb_idx, G.cur_stream())
    assert got == -1 and b"2 index value(s) lie outside" in lib.amds_last_error()
    torch.cuda.synchronize()
    for h in b.handles:
        h.assert_bands_intact()


def test_wrappers_run_on_a_guarded_workspace_of_the_stated_size(gpu, monkeypatch):
    from stamp_amd import metrics
    s, t, e, idx = _resample_case()
    grid = _grid_for(t, 16)
    cut = O.median_cut_off(s, t, e)
    wants = [O.survival(s[r], t[r], e[r], cut, grid=grid) for r in idx]
    for pattern in G.PATTERNS:
        with G.scratch_hook(monkeypatch, pattern) as log:
            res = metrics.survival_groups(_dev(gpu, s), _dev(gpu, t), _dev(gpu, e), grid_times=_dev(gpu, grid), idx=_dev(gpu, idx))
            m = metrics.regression_moments(_dev(gpu, s), _dev(gpu, t), idx=_dev(gpu, idx))
            torch.cuda.synchronize()
            log.assert_bands_intact()
        assert log.bytes_for("survival_stats") == [1024 + 1024 + 256 + 512] and log.bytes_for("regression_stats") == [512]
        _check(res, wants, 16)
        np.testing.assert_allclose(m.cpu().numpy(), [O.moments(t[r], s[r]) for r in idx], rtol=M_RTOL)          # (pred = the scores, truth = the times)
    with G.scratch_hook(monkeypatch, 0xFF, short_by=1):
        with pytest.raises(RuntimeError, match="workspace"):
            metrics.survival_groups(_dev(gpu, s), _dev(gpu, t), _dev(gpu, e))
        with pytest.raises(RuntimeError, match="workspace"):
            metrics.regression_moments(_dev(gpu, s), _dev(gpu, t))


# ---- regression --------------------------------------------------------------------------------------------------------------------------------------------
def _reg_case(n, seed):
    rng = np.random.default_rng(seed)
    t = rng.uniform(1, 3, n).astype(np.float32)
    return t, (0.8 * t + rng.normal(0, 0.3, n) + 0.5).astype(np.float32)


def _check_stats(got, want):
    """The report's numbers are a few float64 operations on moments good to 1e-12; the worst conditioned, 1 - r^2 in stderr with r about 0.85 on this data,
    amplifies by 2 r^2 / (1 - r^2) < 6: 1e-10 leaves an order of magnitude."""
    from stamp_amd import metrics
    for k in metrics.REGRESSION_KEYS:
        assert got[k].dim() == 0 and got[k].device.type == "cuda" and got[k].dtype == (torch.int64 if k == "count" else torch.float64)
        np.testing.assert_allclose(got[k].item(), want[k], rtol=1e-10, equal_nan=True, err_msg=k)


@pytest.mark.parametrize("n", [1, 2, 257, 70001])
def test_regression_moments_and_stats_equal_the_oracle(gpu, n):
    from stamp_amd import metrics
    t, p = _reg_case(n, n)
    if n > 2:
        t[[3, n - 1]], p[[5, n - 1]] = np.nan, np.nan
    m = metrics.regression_moments(_dev(gpu, p), _dev(gpu, t))
    want = O.moments(t, p)
    print("moments", m[0].tolist(), want)
    assert m.dtype == torch.float64 and tuple(m.shape) == (1, 8)
    np.testing.assert_allclose(m[0].cpu().numpy(), want, rtol=M_RTOL, atol=0, equal_nan=True)
    got = metrics.regression_stats(_dev(gpu, p), _dev(gpu, t))
    _check_stats(got, O.regression(want))
    if n < 3:
        return
    try:
        import scipy.stats as st
        import sklearn.metrics as sk
    except ImportError:
        return
    ok = ~(np.isnan(t) | np.isnan(p))
    t64, p64 = t[ok].astype(np.float64), p[ok].astype(np.float64)
    line = st.linregress(t64, p64)
    ref = dict(r2_score=sk.r2_score(t64, p64), mae=sk.mean_absolute_error(t64, p64), rmse=math.sqrt(sk.mean_squared_error(t64, p64)),
               pearson_r=st.pearsonr(t64, p64)[0], slope=line.slope, intercept=line.intercept, stderr=line.stderr, count=int(ok.sum()))
    _check_stats(got, ref)


def test_regression_constant_column_strides_resamples_and_refusals(gpu):
    from stamp_amd import _lib, metrics
    const = metrics.regression_moments(_dev(gpu, np.arange(257, dtype=np.float32)), torch.full((257,), 0.1, device=gpu))
    assert const[0, metrics.SXX].item() == 0.0 == const[0, metrics.SXY].item() and const[0, metrics.MEAN_T].item() == float(np.float32(0.1))
    st = metrics.regression_stats(_dev(gpu, np.arange(257, dtype=np.float32)), torch.full((257,), 0.1, device=gpu))
    assert st["pearson_r"].isnan() and st["r2_score"].item() == 0.0 and st["slope"].isnan() and st["count"].item() == 257
    assert metrics.regression_stats(torch.full((9,), 2.0, device=gpu), _dev(gpu, _reg_case(9, 1)[0]))["pearson_r"].isnan()          # a constant prediction
    # three problems as the columns of a row-major matrix (item stride 4, problem stride 1) against one shared truth
    n = 333
    t, _ = _reg_case(n, 2)
    p = np.stack([_reg_case(n, 2)[1], _reg_case(n, 3)[1], t, t], axis=1)
    p[7, 1] = np.nan
    m = metrics.regression_moments(_dev(gpu, p)[:, :3].t(), _dev(gpu, t))
    np.testing.assert_allclose(m.cpu().numpy(), [O.moments(t, p[:, c]) for c in range(3)], rtol=M_RTOL, equal_nan=True)
    assert m[2, metrics.SSE].item() == 0.0 and metrics.regression_from_moments(m)["r2_score"][2].item() == 1.0
    # resamples with duplicates against the oracle on the gathered arrays; bootstrap intervals
    rng = np.random.default_rng(4)
    idx = rng.integers(0, n, (21, 400)).astype(np.int32)
    td, pd = _dev(gpu, t), _dev(gpu, p[:, 1].copy())
    wants = [O.moments(t[r], p[r, 1]) for r in idx]
    np.testing.assert_allclose(metrics.regression_moments(pd, td, idx=_dev(gpu, idx.astype(np.int64))).cpu().numpy(), wants, rtol=M_RTOL)
    b = metrics.bootstrap_regression(pd, td, idx=_dev(gpu, idx))
    rows = [O.regression(w) for w in wants]
    for k, (value, lo, hi) in b.items():
        np.testing.assert_allclose([value.item(), lo.item(), hi.item()],
                                   [O.regression(O.moments(t, p[:, 1]))[k], *np.quantile([r[k] for r in rows], [0.025, 0.975])], rtol=1e-10, err_msg=k)
    assert set(b) == set(metrics.REGRESSION_KEYS) - {"count"}
    a1 = metrics.bootstrap_regression(pd, td, n_resamples=20, generator=torch.Generator().manual_seed(1))
    a2 = metrics.bootstrap_regression(pd, td, n_resamples=20, generator=torch.Generator().manual_seed(1))
    assert all(torch.equal(a1[k][1], a2[k][1]) and a1[k][1] <= a1[k][2] for k in a1)
    for bad in ([[0, 1, n]], [[0, -1, 2]]):
        with pytest.raises(RuntimeError, match="outside"):
            metrics.regression_moments(pd, td, idx=torch.tensor(bad, device=gpu))
    with pytest.raises(ValueError, match="ONE problem"):
        metrics.regression_moments(pd[None].expand(2, -1), td, idx=_dev(gpu, idx))

    # the C ABI: the same bits under both poisons and from two calls, guard bands intact, refusals
    lib = _lib.lib()
    nb = lib.amds_regression_moments_workspace_bytes(0, n, 3)

    def call(pattern):
        bufs = G.Bufs(gpu, pattern)
        pp, tt, ix = bufs.inp(torch.from_numpy(np.nan_to_num(p, nan=1.5)), name="pred"), bufs.inp(torch.from_numpy(t), name="truth"), \
            bufs.inp(torch.from_numpy(idx), name="idx")
        outs = {}
        for tag, rows, ixp, base, items in (("0", 3, None, 0, n), ("1", 3, None, 0, n), ("_idx", 21, ix.data_ptr(), n, 400)):
            ws, out = bufs.out((nb,), torch.uint8, name="ws" + tag), bufs.out((rows, 8), torch.float64, name="moments" + tag)
            _lib.check(lib.amds_regression_moments(tt.data_ptr(), 1, 0, pp.data_ptr(), 4, 1, ixp, base, items, rows, out.data_ptr(), ws.data_ptr(), nb,
                                                   G.cur_stream()), "regression_moments" + tag)
            outs["moments" + tag] = out
        return bufs.result(**outs)

    o = G.run_contract(call)
    assert torch.equal(o["moments0"], o["moments1"])
    pf = np.nan_to_num(p, nan=1.5)
    np.testing.assert_allclose(o["moments0"].cpu().numpy(), [O.moments(t, pf[:, c]) for c in range(3)], rtol=M_RTOL)
    np.testing.assert_allclose(o["moments_idx"].cpu().numpy(), [O.moments(t[r], pf[r, 0]) for r in idx], rtol=M_RTOL)
    bufs = G.Bufs(gpu, 0xFF)
    pp, tt = bufs.inp(torch.from_numpy(pf)), bufs.inp(torch.from_numpy(t))
    ws, out = bufs.out((nb,), torch.uint8, name="ws"), bufs.out((3, 8), torch.float64, name="moments")

    def rc(*, t_=tt.data_ptr(), p_=pp.data_ptr(), ix_=None, base=0, n_=n, P_=3, out_=out.data_ptr(), ws_=ws.data_ptr(), nb_=nb, ti=1, tp=0, pi=4, pp_=1):
        return lib.amds_regression_moments(t_, ti, tp, p_, pi, pp_, ix_, base, n_, P_, out_, ws_, nb_, G.cur_stream())

    assert rc(nb_=nb - 1) == -2 and b"workspace" in lib.amds_last_error()
    for bad in (dict(t_=None), dict(p_=None), dict(out_=None), dict(ws_=None), dict(ws_=ws.data_ptr() + 8), dict(n_=0), dict(n_=1 << 31), dict(P_=0), dict(ti=0),
                dict(pi=0), dict(tp=-1), dict(pp_=-1), dict(ix_=tt.data_ptr(), base=0)):
        assert rc(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool(out.isnan().all())
    for h in bufs.handles:
        h.assert_bands_intact()
