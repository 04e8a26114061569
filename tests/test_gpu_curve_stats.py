"""amds_binary_curves and the stamp_amd.metrics functions over it on the GPU, against tests/curve_oracle.py (the definition of include/amdstamp.h as
plain numpy, itself pinned against sklearn + np.interp by tests/test_cpu_curve_stats.py), the C-ABI contract (reproducible, poisoned workspace, guard
bands, NULL grids, refusals), and `mil_train.fit(valid_auprc=True)`.

Bars.  Counts are integers: equality.  The library and the oracle decide the order, the ties and the segment of every grid point on the same integers, so
a scalar or a grid value differs only by float64 rounding: a sum of at most 12289 terms <= 1 in another order (the oracle sums exactly), or one
interpolation of ratios; 1e-12 absolute covers both with three orders to spare and is far below any wrong decision (a neighbouring segment differs by
about 1 / n)."""
import numpy as np
import pytest
import torch

import curve_oracle as O
import guarded as G
import rank_oracle as R

pytestmark = pytest.mark.gpu

ATOL = 1e-12
# 256 threads per workgroup and scan tile, 64 lanes per wave, 1024 keys per LDS tile of the rank kernel
SIZES = [1, 2, 63, 64, 255, 256, 257, 1025]
GRIDS = [0, 2, 3, 1000]


def _case(n, levels, seed):
    """levels: 8 (sixteenths-like ties), 1 (everything tied), 0 (continuous scores).  Both classes present from n = 2 on."""
    rng = np.random.default_rng(seed)
    if levels == 0:
        s = rng.random(n).astype(np.float32)
    else:
        s = (rng.integers(0, levels, n) / 8).astype(np.float32)
    y = (rng.random(n) < 0.4).astype(np.uint8)
    if n >= 2:
        y[rng.integers(0, n)] = 1
        y[(np.flatnonzero(y == 1)[0] + 1) % n] = 0
    return s, y


def _dev(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _check(res, wants, grid, roc=True, pr=True):
    assert res.counts.dtype == torch.int64 and [tuple(r) for r in res.counts.cpu().tolist()] == [w["counts"] for w in wants]
    for name in ("ap", "pr_area", "pr_area_grid"):
        got = getattr(res, name)
        assert got.dtype == torch.float64 and got.device.type == "cuda"
        np.testing.assert_allclose(got.cpu().numpy(), [w[name] for w in wants], rtol=0, atol=ATOL, equal_nan=True, err_msg=name)
    for name, on in (("roc", roc), ("pr", pr)):
        got = getattr(res, name)
        if not on:
            assert got is None
            continue
        assert got.dtype == torch.float64 and tuple(got.shape) == (len(wants), grid)
        np.testing.assert_allclose(got.cpu().numpy(), np.stack([w[name] for w in wants]).reshape(len(wants), grid), rtol=0, atol=ATOL, equal_nan=True,
                                   err_msg=name)


@pytest.mark.parametrize("levels", [8, 1, 0])
@pytest.mark.parametrize("n", SIZES)
def test_counts_scalars_and_grids_equal_the_oracle(gpu, n, levels):
    from stamp_amd import metrics
    s, y = _case(n, levels, 1000 * levels + n)
    for grid in GRIDS:
        on = grid > 0
        res = metrics.binary_curves(_dev(gpu, s), _dev(gpu, y), grid=grid, roc=on, pr=on)
        _check(res, [O.curves(s, y, grid=grid)], grid, on, on)
    if n == 1:
        assert res.ap.isnan().all() and res.roc.isnan().all() and res.pr.isnan().all()          # one item: one class
    if levels == 1 and n >= 2:                                                                  # everything tied: AP = P / (P + N), the ROC grid = x
        assert abs(res.ap.item() - y.sum() / n) < ATOL
        np.testing.assert_allclose(res.roc[0].cpu().numpy(), np.arange(1000) / 999, rtol=0, atol=ATOL)


@pytest.mark.parametrize("n", [12288, 12289])
def test_the_threshold_between_lds_and_workspace_arrays(gpu, n):
    """Up to 12288 positions the two count arrays of a problem live in LDS, above in the workspace: both sides of the threshold, ties and none, resampled."""
    from stamp_amd import metrics
    rng = np.random.default_rng(n)
    s = np.stack([_case(n, 8, n)[0], _case(n, 0, n + 1)[0]])
    y = np.stack([_case(n, 8, n)[1], _case(n, 0, n + 1)[1]])
    _check(metrics.binary_curves(_dev(gpu, s), _dev(gpu, y), grid=1000), [O.curves(s[p], y[p], grid=1000) for p in range(2)], 1000)
    idx = rng.integers(0, n, (3, 5000)).astype(np.int32)
    _check(metrics.binary_curves(_dev(gpu, s[1]), _dev(gpu, y[1]), idx=_dev(gpu, idx), grid=257), [O.curves(s[1][r], y[1][r], grid=257) for r in idx], 257)


def test_invalid_items_signed_zeros_and_denormals(gpu):
    from stamp_amd import metrics
    rng = np.random.default_rng(3)
    n = 300
    s, y = _case(n, 8, 77)
    s[[0, 17, 255, 256, n - 1]] = np.nan
    y[[1, 18, 254]] = 2
    y[[2, 257]] = 255
    _check(metrics.binary_curves(_dev(gpu, s), _dev(gpu, y), grid=1000), [O.curves(s, y, grid=1000)], 1000)
    nan_label = np.where(y > 1, np.nan, y.astype(np.float32)).astype(np.float32)          # numbers: 0 and 1 are valid, everything else (NaN too) is not
    _check(metrics.binary_curves(_dev(gpu, s), _dev(gpu, nan_label), grid=3), [O.curves(s, y, grid=3)], 3)
    vals = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32)
    s2, y2 = rng.choice(vals, n), rng.integers(0, 2, n).astype(np.uint8)
    want = O.curves(s2, y2, grid=1000)
    assert len(O.curve_points(s2, y2)[0]) == 7                                             # -0 and +0 are one threshold, the denormals their own
    _check(metrics.binary_curves(_dev(gpu, s2), _dev(gpu, y2.astype(bool)), grid=1000), [want], 1000)
    ap = metrics.average_precision(_dev(gpu, s2), _dev(gpu, y2))
    assert ap.dim() == 0 and ap.dtype == torch.float64 and abs(ap.item() - want["ap"]) < ATOL
    assert metrics.average_precision(_dev(gpu, s2), torch.zeros(n, device=gpu)).isnan()
    with pytest.raises(ValueError, match="grid=1"):
        metrics.binary_curves(_dev(gpu, s2), _dev(gpu, y2), grid=1)
    with pytest.raises(ValueError, match="grid=0"):
        metrics.binary_curves(_dev(gpu, s2), _dev(gpu, y2), grid=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.binary_curves(torch.from_numpy(s2), torch.from_numpy(y2))


def test_three_problems_through_the_strides_multiclass_auprc_and_categorical_stats(gpu):
    from stamp_amd import metrics
    rng = np.random.default_rng(8)
    n, C = 333, 4
    y = rng.integers(0, C - 1, n)                                                          # the last class is absent
    p = rng.integers(0, 16, (n, C)).astype(np.float32) / 16
    pd, yd = _dev(gpu, p), _dev(gpu, y)
    pos = np.stack([(y == c) for c in range(C)])
    wants = [O.curves(p[:, c], pos[c].astype(np.uint8), grid=1000) for c in range(C)]
    _check(metrics.binary_curves(pd[:, :3].t(), _dev(gpu, pos[:3]), grid=1000), wants[:3], 1000)          # item stride 4, problem stride 1: no copy
    _check(metrics.binary_curves(pd.t(), _dev(gpu, pos), grid=2), [O.curves(p[:, c], pos[c].astype(np.uint8), grid=2) for c in range(C)], 2)
    per, mean = metrics.multiclass_auprc(pd, yd)
    assert per.dtype == torch.float64 and per[C - 1].isnan() and np.isnan(wants[C - 1]["ap"])
    np.testing.assert_allclose(per[:C - 1].cpu().numpy(), [w["ap"] for w in wants[:C - 1]], rtol=0, atol=ATOL)
    assert abs(mean.item() - np.mean([w["ap"] for w in wants[:C - 1]])) < ATOL
    nothing = metrics.multiclass_auprc(torch.full((4, 1), 0.5, device=gpu), torch.zeros(4, dtype=torch.long, device=gpu))
    assert nothing[0].isnan().all() and nothing[1].isnan()
    st = metrics.categorical_stats(pd, yd)
    assert st["count"].cpu().tolist() == [int((y == c).sum()) for c in range(C)]
    auroc = metrics.multiclass_auroc(pd, yd)[0]
    assert torch.equal(st["roc_auc_score"].nan_to_num(-1.0), auroc.nan_to_num(-1.0)) and torch.equal(st["average_precision_score"].nan_to_num(-1.0), per.nan_to_num(-1.0))
    pred = p.argmax(axis=1)
    f1 = [2 * ((pred == c) & (y == c)).sum() / max(2 * ((pred == c) & (y == c)).sum() + ((pred == c) ^ (y == c)).sum(), 1) for c in range(C)]
    np.testing.assert_allclose(st["f1_score"].cpu().numpy(), f1, rtol=0, atol=1e-15)
    try:
        from sklearn.metrics import average_precision_score, f1_score
    except ImportError:
        return
    for c in range(C - 1):
        assert abs(per[c].item() - average_precision_score(y == c, p[:, c])) < ATOL
        assert abs(st["f1_score"][c].item() - f1_score(y == c, pred == c)) < 1e-15


def _resample_case():
    rng = np.random.default_rng(5)
    n, R_, m = 211, 37, 300
    s, y = _case(n, 8, 21)
    idx = rng.integers(0, n, (R_, m)).astype(np.int32)
    idx[11] = np.flatnonzero(y == 0)[rng.integers(0, int((y == 0).sum()), m)]             # one resample forced to a single class
    return s, y, idx


def test_resamples_equal_the_oracle_on_the_gathered_arrays(gpu):
    from stamp_amd import metrics
    s, y, idx = _resample_case()
    wants = [O.curves(s[r], y[r], grid=1000) for r in idx]
    assert np.isnan(wants[11]["ap"]) and sum(np.isnan(w["ap"]) for w in wants) == 1
    sd, yd = _dev(gpu, s), _dev(gpu, y)
    res = metrics.binary_curves(sd, yd, idx=_dev(gpu, idx), grid=1000)
    _check(res, wants, 1000)
    assert res.roc[11].isnan().all() and res.pr[11].isnan().all() and res.counts[11].cpu().tolist() == [0, 300]
    _check(metrics.binary_curves(sd, yd, idx=_dev(gpu, idx[:, :129].astype(np.int64)), grid=3, roc=False), [O.curves(s[r], y[r], grid=3) for r in idx[:, :129]],
           3, roc=False)
    for bad in ([[0, 1, 211]], [[0, -1, 2]]):
        with pytest.raises(RuntimeError, match="outside"):
            metrics.binary_curves(sd, yd, idx=torch.tensor(bad, device=gpu), grid=2)
    with pytest.raises(ValueError, match="ONE problem"):
        metrics.binary_curves(sd[None].expand(2, -1), yd, idx=_dev(gpu, idx), grid=2)


@pytest.mark.parametrize("kind", ["roc", "pr"])
def test_bootstrap_curve_bands_are_the_quantiles_of_the_oracles_rows(gpu, kind):
    from stamp_amd import metrics
    s, y, idx = _resample_case()
    wants = [w for w in (O.curves(s[r], y[r], grid=1000) for r in idx) if not np.isnan(w["ap"])]
    sd, yd = _dev(gpu, s), _dev(gpu, y)
    b = metrics.bootstrap_curve(sd, yd, kind=kind, idx=_dev(gpu, idx), quantiles=(0.025, 0.975))
    assert b.used == 36 == len(wants)
    lo, hi = np.quantile(np.stack([w[kind] for w in wants]), [0.025, 0.975], axis=0)
    # (a quantile moves by no more than the largest change of a row value: the rows' bar holds for the bands)
    np.testing.assert_allclose(b.band_lower.cpu().numpy(), lo, rtol=0, atol=ATOL)
    np.testing.assert_allclose(b.band_upper.cpu().numpy(), hi, rtol=0, atol=ATOL)
    np.testing.assert_allclose(b.x.cpu().numpy(), np.linspace(0, 1, 1000), rtol=0, atol=1e-15)
    t, e = (y != 1).astype(np.float32), y
    if kind == "roc":
        vals = [R.c_of(R.pair_counts(s[r], t[r], e[r])) for k, r in enumerate(idx) if k != 11]
        assert b.value.item() == R.c_of(R.pair_counts(s, t, e))
    else:
        vals = [w["pr_area_grid"] for w in wants]
        assert abs(b.value.item() - O.curves(s, y, grid=0)["pr_area"]) < ATOL
    assert abs(b.lower.item() - np.quantile(vals, 0.025)) < ATOL and abs(b.upper.item() - np.quantile(vals, 0.975)) < ATOL
    for v in b[:6]:
        assert v.dtype == torch.float64 and v.device.type == "cuda"
    # drawn resamples: reproducible from the generator; nothing usable -> NaN bounds and bands
    a1 = metrics.bootstrap_curve(sd, yd, kind=kind, n_resamples=20, grid=50, generator=torch.Generator().manual_seed(1))
    a2 = metrics.bootstrap_curve(sd, yd, kind=kind, n_resamples=20, grid=50, generator=torch.Generator().manual_seed(1))
    assert a1.used == a2.used == 20 and torch.equal(a1.band_lower, a2.band_lower) and bool((a1.band_lower <= a1.band_upper).all()) and a1.x.shape == (50,)
    none = metrics.bootstrap_curve(sd, torch.zeros_like(yd), kind=kind, n_resamples=3, grid=5)
    assert none.used == 0 and none.value.isnan() and none.lower.isnan() and none.band_upper.isnan().all()


def test_c_abi_reproducible_poisoned_workspace_guard_bands_null_grids_and_refusals(gpu):
    """amds_binary_curves on workspaces of exactly the stated size inside guard bands, poisoned with 0x00 and with 0xFF, guard bands around every output:
    the same bits under both poisons and from two calls, the oracle's values, bands intact; a NULL grid is skipped and changes nothing else; an undersized
    or misaligned workspace, a NULL pointer, bad shapes and an out-of-range index are refused."""
    from stamp_amd import _lib
    lib = _lib.lib()
    n, P, grid, m, R_ = 1500, 3, 1000, 700, 4
    rng = np.random.default_rng(9)
    cols = [_case(n, 8 if p else 0, 90 + p) for p in range(P)]
    score = np.stack([c[0] for c in cols], axis=1)                                   # [n][P]: item stride P, problem stride 1
    label = np.stack([c[1] for c in cols])                                           # [P][n]
    idx = rng.integers(0, n, (R_, m)).astype(np.int32)
    nb, nb_idx = lib.amds_binary_curves_workspace_bytes(0, n, P, grid), lib.amds_binary_curves_workspace_bytes(n, m, R_, grid)
    assert nb > 0 and nb % 256 == 0 and nb_idx > 0

    def call(pattern):
        b = G.Bufs(gpu, pattern)
        s, y, ix = b.inp(torch.from_numpy(score), name="score"), b.inp(torch.from_numpy(label), name="label"), b.inp(torch.from_numpy(idx), name="idx")
        outs = {}

        def run(tag, ws_bytes, rows, want_roc, want_pr, ixp, base, items, lp):
            ws, cnt, sc = b.out((ws_bytes,), torch.uint8, name="ws" + tag), b.out((rows, 2), torch.int64, name="counts" + tag), \
                b.out((rows, 3), torch.float64, name="scalars" + tag)
            roc = b.out((rows, grid), torch.float64, name="roc" + tag) if want_roc else None
            pr = b.out((rows, grid), torch.float64, name="pr" + tag) if want_pr else None
            _lib.check(lib.amds_binary_curves(s.data_ptr(), P, 0 if ixp else 1, y.data_ptr(), lp, ixp, base, items, rows, grid, cnt.data_ptr(), sc.data_ptr(),
                                              G.ptr(roc), G.ptr(pr), ws.data_ptr(), ws_bytes, G.cur_stream()), "binary_curves" + tag)
            outs.update({"counts" + tag: cnt, "scalars" + tag: sc})
            if want_roc:
                outs["roc" + tag] = roc
            if want_pr:
                outs["pr" + tag] = pr

        run("0", nb, P, True, True, None, 0, n, n)
        run("1", nb, P, True, True, None, 0, n, n)
        run("_pr_only", nb, P, False, True, None, 0, n, n)
        run("_no_grid", nb, P, False, False, None, 0, n, n)
        run("_idx", nb_idx, R_, True, True, ix.data_ptr(), n, m, 0)
        return b.result(**outs)

    o = G.run_contract(call)
    for k in ("counts", "scalars", "roc", "pr"):
        assert torch.equal(o[k + "0"], o[k + "1"]), k                                # two calls: the same bits
    assert torch.equal(o["pr_pr_only"], o["pr0"]) and torch.equal(o["scalars_pr_only"], o["scalars0"]) and torch.equal(o["scalars_no_grid"], o["scalars0"])
    assert torch.equal(o["counts_no_grid"], o["counts0"])
    wants = [O.curves(*c, grid=grid) for c in cols]
    wants_idx = [O.curves(cols[0][0][r], cols[0][1][r], grid=grid) for r in idx]
    for tag, ws_ in (("0", wants), ("_idx", wants_idx)):
        assert [tuple(r) for r in o["counts" + tag].cpu().tolist()] == [w["counts"] for w in ws_]
        np.testing.assert_allclose(o["scalars" + tag].cpu().numpy(), [[w["ap"], w["pr_area"], w["pr_area_grid"]] for w in ws_], rtol=0, atol=ATOL)
        for kind in ("roc", "pr"):
            np.testing.assert_allclose(o[kind + tag].cpu().numpy(), np.stack([w[kind] for w in ws_]), rtol=0, atol=ATOL)

    # refusals: nothing is launched, so the poisoned outputs stay poisoned
    b = G.Bufs(gpu, 0xFF)
    s, y = b.inp(torch.from_numpy(score)), b.inp(torch.from_numpy(label))
    ws, cnt, sc = b.out((nb,), torch.uint8, name="ws"), b.out((P, 2), torch.int64, name="counts"), b.out((P, 3), torch.float64, name="scalars")
    roc = b.out((P, grid), torch.float64, name="roc")

    def rc(*, s_=s.data_ptr(), y_=y.data_ptr(), ix_=None, base=0, n_=n, P_=P, g_=grid, cnt_=cnt.data_ptr(), sc_=sc.data_ptr(), ws_=ws.data_ptr(), nb_=nb, si=P,
           sp=1):
        return lib.amds_binary_curves(s_, si, sp, y_, n, ix_, base, n_, P_, g_, cnt_, sc_, roc.data_ptr(), None, ws_, nb_, G.cur_stream())

    assert rc(nb_=nb - 1) == -2 and b"workspace" in lib.amds_last_error()
    assert rc(ws_=ws.data_ptr() + 8) == -1
    for bad in (dict(s_=None), dict(y_=None), dict(cnt_=None), dict(sc_=None), dict(ws_=None), dict(n_=0), dict(P_=0), dict(si=0), dict(sp=-1), dict(g_=0),
                dict(g_=1), dict(g_=4097), dict(ix_=s.data_ptr(), base=0), dict(n_=(1 << 20) + 1)):
        assert rc(**bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((cnt == -1).all()) and bool(sc.isnan().all()) and bool(roc.isnan().all())
    # an out-of-range index fails the call (and is never dereferenced: the base problem ends where the guard band begins)
    bad_idx = idx.copy()
    bad_idx[2, 333] = n
    bad_idx[0, 0] = -5
    ix = b.inp(torch.from_numpy(bad_idx), name="bad idx")
    ws2, cnt2, sc2 = b.out((nb_idx,), torch.uint8, name="ws_idx"), b.out((R_, 2), torch.int64, name="counts_idx"), b.out((R_, 3), torch.float64, name="sc_idx")
    got = lib.amds_binary_curves(s.data_ptr(), P, 0, y.data_ptr(), 0, ix.data_ptr(), n, m, R_, 0, cnt2.data_ptr(), sc2.data_ptr(), None, None, ws2.data_ptr(),
                                 nb_idx, G.cur_stream())
    assert got == -1 and b"2 index value(s) lie outside" in lib.amds_last_error()
    torch.cuda.synchronize()
    for h in b.handles:
        h.assert_bands_intact()


def test_wrappers_run_on_a_guarded_workspace_of_the_stated_size(gpu, monkeypatch):
    from stamp_amd import metrics
    s, y, idx = _resample_case()
    for pattern in G.PATTERNS:
        with G.scratch_hook(monkeypatch, pattern) as log:
            res = metrics.binary_curves(_dev(gpu, s), _dev(gpu, y), idx=_dev(gpu, idx), grid=64)
            torch.cuda.synchronize()
            log.assert_bands_intact()
        assert log.bytes_for("curve_stats") == [1024 + 512]
        _check(res, [O.curves(s[r], y[r], grid=64) for r in idx], 64)
    with G.scratch_hook(monkeypatch, 0xFF, short_by=1):
        with pytest.raises(RuntimeError, match="workspace"):
            metrics.binary_curves(_dev(gpu, s), _dev(gpu, y), grid=64)


def _toy_fit(gpu, **kw):
    """The three-class toy run of test_gpu_rank_metrics.py::test_fit_valid_auroc_on_a_three_class_toy_run."""
    from stamp_amd.mil import VisionTransformer
    from stamp_amd.mil_train import HipMilVitTrainer, fit

    Fd = 64
    g = torch.Generator().manual_seed(41)
    cls = torch.tensor([0, 1, 2] * 4)
    feats = [torch.randn(int(t), Fd, generator=g) + 0.5 * float(cls[k]) for k, t in enumerate(torch.randint(8, 40, (12,), generator=g))]
    onehot = torch.nn.functional.one_hot(cls, 3).float()
    train = [(torch.stack([f[:8] for f in feats]), None, None, onehot)]
    valid = [(feats[k][None], None, None, onehot[k:k + 1]) for k in range(12)]
    torch.manual_seed(0)
    model = VisionTransformer(dim_output=3, dim_input=Fd, dim_model=64, n_layers=1, n_heads=2, dim_feedforward=64, dropout=0.0, use_alibi=False)
    tr = HipMilVitTrainer(model, device=gpu, max_lr=3e-3, total_steps=2, sched_interval="step", dropout=False)
    preds, predict0 = [], tr.predict

    def predict(*a, **k):
        lg = predict0(*a, **k)
        preds.append(lg.detach().clone())
        return lg
    tr.predict = predict
    hist = fit(tr, lambda: train, lambda: valid, max_epochs=2, patience=8, **kw)
    return tr, hist, preds, cls


def test_fit_valid_auprc_on_the_three_class_toy_run(gpu):
    from stamp_amd import metrics, mil_train
    tr, hist, preds, cls = _toy_fit(gpu, valid_auprc=True, valid_auroc=True)
    assert len(hist["validation_auprc"]) == 2 == len(hist["validation_auroc"])
    for ep in range(2):
        probs = torch.softmax(torch.cat(preds[ep * 12:(ep + 1) * 12]).float(), dim=1)
        assert hist["validation_auprc"][ep] == metrics.multiclass_auprc(probs, cls.to(gpu))[1].item()
        assert hist["validation_auroc"][ep] == metrics.multiclass_auroc(probs, cls.to(gpu))[1].item()
        want = np.mean([O.curves(probs[:, c].cpu().numpy(), (cls == c).numpy().astype(np.uint8), grid=0)["ap"] for c in range(3)])
        assert abs(hist["validation_auprc"][ep] - want) < ATOL
    only, h_only, _, _ = _toy_fit(gpu, valid_auprc=True)
    off, h_off, _, _ = _toy_fit(gpu)
    assert "validation_auprc" not in h_off and "validation_auroc" not in h_off and "validation_auroc" not in h_only
    assert h_only["validation_auprc"] == hist["validation_auprc"]
    for h in (hist, h_only):                                                          # the flag changes neither a loss nor a weight
        assert {k: v for k, v in h.items() if not k.startswith("validation_au")} == h_off
    assert torch.equal(tr.P, off.P) and torch.equal(only.P, off.P)
    with pytest.raises(ValueError, match="valid_auprc"):
        mil_train.fit(object(), lambda: (), lambda: (), max_epochs=1, loss_fn=lambda a, b: a.sum(), valid_auprc=True)
