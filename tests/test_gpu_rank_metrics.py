"""stamp_amd.metrics and amds_concordance_counts on the GPU against the brute-force oracle (tests/rank_oracle.py), sklearn where it is installed, the C-ABI
contract (reproducible, poisoned workspace, guard bands, refusals), and `mil_train.fit(monitor="val_cindex")` / `fit(valid_auroc=True)`.

Counts are integers: every comparison of counts is an equality.  A C value is (concordant + tied / 2) / permissible evaluated in float64 from the same integers
on both sides, so those compare exactly too; against sklearn's trapezoid sum the bar is 1e-12 (a few hundred float64 roundings of values <= 1)."""
import numpy as np
import pytest
import torch

import guarded as G
import rank_oracle as R

pytestmark = pytest.mark.gpu

# the kernel's edges: 256 i items per workgroup, an inner loop in steps of 8, 1024 j items per LDS tile, 4096 j items per chunk (two chunks from 4097 on)
SIZES = [1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 513, 1000, 1023, 1024, 1025, 4095, 4096, 4097]


def _counts(gpu, score, time, event, idx=None):
    from stamp_amd import metrics
    out = metrics.concordance_counts(torch.from_numpy(np.asarray(score)).to(gpu), torch.from_numpy(np.asarray(time)).to(gpu),
                                     torch.from_numpy(np.asarray(event)).to(gpu), None if idx is None else torch.from_numpy(np.asarray(idx)).to(gpu))
    return [tuple(r) for r in out.cpu().tolist()]


@pytest.mark.parametrize("n", SIZES)
def test_counts_equal_the_oracle(gpu, n):
    score, time, event = R.heavy_ties(n, n)
    assert _counts(gpu, score, time, event) == [R.pair_counts(score, time, event)]


@pytest.mark.parametrize("n", [257, 1000])
def test_counts_all_censored_all_events_and_nan_items(gpu, n):
    from stamp_amd import metrics
    score, time, event = R.heavy_ties(n, 7 * n)
    for ev in (np.zeros(n, np.uint8), np.ones(n, np.uint8)):
        assert _counts(gpu, score, time, ev) == [R.pair_counts(score, time, ev)]
    assert _counts(gpu, score, time, np.zeros(n, np.uint8))[0][2] == 0
    s2, t2, e2 = score.copy(), time.copy(), event.astype(np.float32)
    s2[[0, n // 2, n - 1]], t2[[1, 255, 256]], e2[[2, 254, n - 2]] = np.nan, np.nan, np.nan
    for case in ((s2, time, event), (score, t2, event), (score, time, e2), (s2, t2, e2)):
        want = R.pair_counts(*case)
        assert _counts(gpu, *case) == [want]
        ci = metrics.concordance_index(*[torch.from_numpy(a).to(gpu) for a in case])
        assert ci.dim() == 0 and ci.device.type == "cuda" and ci.dtype == torch.float32 and ci.item() == np.float32(R.c_of(want))
    e3 = event.copy()
    e3[5] = 2                                       # an event byte that is neither 0 nor 1
    assert _counts(gpu, score, time, e3) == [R.pair_counts(score, time, e3)]
    # the reference's c_index: at most one valid row -> NaN; no permissible pair -> NaN
    one = torch.tensor([1.0, float("nan")], device=gpu)
    assert metrics.concordance_index(one, torch.tensor([1.0, 2.0], device=gpu), torch.ones(2, device=gpu)).isnan()
    assert metrics.concordance_index(torch.from_numpy(score).to(gpu), torch.from_numpy(time).to(gpu), torch.zeros(n, device=gpu)).isnan()
    assert metrics.concordance_index(torch.tensor([2.0, 1.0], device=gpu), torch.tensor([4.0, 4.0], device=gpu), torch.ones(2, device=gpu)).isnan()


def test_signed_zeros_denormals_and_infinities_compare_as_fp32(gpu):
    vals = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32)
    rng = np.random.default_rng(11)
    score, time, event = rng.choice(vals, 300), rng.choice(vals, 300), rng.integers(0, 2, 300).astype(np.uint8)
    assert _counts(gpu, score, time, event) == [R.pair_counts(score, time, event)]


@pytest.mark.parametrize("C", [3, 5])
def test_multiclass_auroc_through_the_strides(gpu, C):
    from stamp_amd import metrics
    rng = np.random.default_rng(C)
    n = 333
    y = rng.integers(0, C - 1, n)                   # the last class is absent
    p = rng.integers(0, 16, (n, C)).astype(np.float32) / 16
    per, mean = metrics.multiclass_auroc(torch.from_numpy(p).to(gpu), torch.from_numpy(y).to(gpu))
    want = [R.c_of(R.pair_counts(p[:, c], (y != c).astype(np.float32), (y == c).astype(np.uint8))) for c in range(C)]
    assert per.dtype == torch.float64 and per[:C - 1].cpu().tolist() == want[:C - 1]
    assert np.isnan(want[C - 1]) and per[C - 1].isnan()
    assert mean.item() == pytest.approx(np.mean(want[:C - 1]), abs=1e-15)          # a float64 mean of C - 1 values <= 1, summed in another order
    # per-problem times and events, a strided score matrix: the same counts as problem by problem
    pos = np.stack([(y == c) for c in range(C)])
    got = _counts(gpu, np.ascontiguousarray(p.T), (~pos).astype(np.float32), pos.astype(np.uint8))
    assert got == [R.pair_counts(p[:, c], (~pos[c]).astype(np.float32), pos[c].astype(np.uint8)) for c in range(C)]
    try:
        from sklearn.metrics import roc_auc_score
    except ImportError:
        return
    for c in range(C - 1):
        assert abs(per[c].item() - roc_auc_score(y == c, p[:, c])) < 1e-12
    everyone_positive = metrics.multiclass_auroc(torch.full((4, 1), 0.5, device=gpu), torch.zeros(4, dtype=torch.long, device=gpu))
    assert everyone_positive[0].isnan().all() and everyone_positive[1].isnan()


def test_resamples_equal_the_oracle_on_the_gathered_arrays(gpu):
    from stamp_amd import metrics
    rng = np.random.default_rng(5)
    n = 300
    score, time, event = R.heavy_ties(n, 55)
    idx = rng.integers(0, n, (7, n)).astype(np.int32)
    assert all(len(np.unique(r)) < n for r in idx)                                  # duplicates: a duplicated item is two items
    assert _counts(gpu, score, time, event, idx) == [R.pair_counts(score[r], time[r], event[r]) for r in idx]
    assert _counts(gpu, score, time, event, idx[:, :129].astype(np.int64)) == [R.pair_counts(score[r], time[r], event[r]) for r in idx[:, :129]]
    # the AUROC reading of the same call, per resample; one resample without a positive is skipped by bootstrap_ci
    y = rng.random(n) < 0.3
    idx[3] = np.flatnonzero(~y)[rng.integers(0, (~y).sum(), n)]
    t_auc, e_auc = (~y).astype(np.float32), y.astype(np.uint8)
    got = _counts(gpu, score, t_auc, e_auc, idx)
    assert got == [R.pair_counts(score[r], t_auc[r], e_auc[r]) for r in idx] and got[3][2] == 0
    vals = np.array([R.c_of(c) for k, c in enumerate(got) if k != 3])
    try:
        from sklearn.metrics import roc_auc_score
        for v, r in zip(vals, np.delete(idx, 3, axis=0)):
            assert abs(v - roc_auc_score(y[r], score[r])) < 1e-12
    except ImportError:
        pass
    dev = [torch.from_numpy(a).to(gpu) for a in (score, t_auc, e_auc)]
    point, lo, hi, used = metrics.bootstrap_ci(*dev, idx=torch.from_numpy(idx).to(gpu), quantiles=(0.025, 0.975))
    assert used == 6 and point.item() == R.c_of(R.pair_counts(score, t_auc, e_auc))
    # np.quantile's linear interpolation between two float64 values <= 1: two roundings, 2^-52 each
    assert lo.item() == pytest.approx(np.quantile(vals, 0.025), abs=1e-15) and hi.item() == pytest.approx(np.quantile(vals, 0.975), abs=1e-15)
    # drawn resamples: reproducible from the generator, bounds around the point value's neighbourhood
    a = metrics.bootstrap_ci(*dev, n_resamples=50, generator=torch.Generator().manual_seed(1))
    b = metrics.bootstrap_ci(*dev, n_resamples=50, generator=torch.Generator().manual_seed(1))
    assert a[3] == b[3] == 50 and a[1].item() == b[1].item() <= a[2].item() == b[2].item()
    with pytest.raises(RuntimeError, match="outside"):
        metrics.concordance_counts(*dev, idx=torch.tensor([[0, 1, n]], device=gpu))
    with pytest.raises(RuntimeError, match="outside"):
        metrics.concordance_counts(*dev, idx=torch.tensor([[0, -1, 2]], device=gpu))


def test_c_abi_reproducible_poisoned_workspace_guard_bands_and_refusals(gpu):
    """amds_concordance_counts on a workspace of exactly the stated size inside guard bands, poisoned with 0x00 and with 0xFF: same counts, the oracle's
    counts, bands intact, twice the same bits; an undersized workspace, a misaligned one, a NULL pointer, bad shapes and an out-of-range index are refused."""
    from stamp_amd import _lib
    lib = _lib.lib()
    n, P = 1500, 3
    rng = np.random.default_rng(9)
    cols = [R.heavy_ties(n, 90 + p) for p in range(P)]
    score = np.stack([c[0] for c in cols], axis=1)                                   # [n][P]: item stride P, problem stride 1
    time, event = np.stack([c[1] for c in cols]), np.stack([c[2] for c in cols])      # [P][n]
    idx = rng.integers(0, n, (4, 700)).astype(np.int32)
    nb, nb_idx = lib.amds_concordance_workspace_bytes(n, P), lib.amds_concordance_workspace_bytes(700, 4)
    assert nb > 0 and nb % 256 == 0 and nb_idx > 0
    assert lib.amds_concordance_workspace_bytes(0, 1) == 0 and lib.amds_concordance_workspace_bytes(1 << 31, 1) == 0 and lib.amds_concordance_workspace_bytes(5, 0) == 0

    def call(pattern):
        b = G.Bufs(gpu, pattern)
        s, t, e, ix = b.inp(torch.from_numpy(score), name="score"), b.inp(torch.from_numpy(time), name="time"), b.inp(torch.from_numpy(event), name="event"), \
            b.inp(torch.from_numpy(idx), name="idx")
        outs = {}
        for rep in range(2):
            ws, out = b.out((nb,), torch.uint8, name="ws"), b.out((P, 4), torch.int64, name="counts")
            _lib.check(lib.amds_concordance_counts(s.data_ptr(), P, 1, t.data_ptr(), n, e.data_ptr(), n, None, 0, n, P, out.data_ptr(), ws.data_ptr(), nb,
                                                   G.cur_stream()), "concordance_counts")
            outs[f"counts{rep}"] = out
        ws, out = b.out((nb_idx,), torch.uint8, name="ws_idx"), b.out((4, 4), torch.int64, name="counts_idx")
        _lib.check(lib.amds_concordance_counts(s.data_ptr(), P, 1, t.data_ptr(), 0, e.data_ptr(), 0, ix.data_ptr(), n, 700, 4, out.data_ptr(), ws.data_ptr(),
                                               nb_idx, G.cur_stream()), "concordance_counts idx")
        return b.result(resampled=out, **outs)

    o = G.run_contract(call)
    assert torch.equal(o["counts0"], o["counts1"])
    assert [tuple(r) for r in o["counts0"].cpu().tolist()] == [R.pair_counts(*c) for c in cols]
    assert [tuple(r) for r in o["resampled"].cpu().tolist()] == [R.pair_counts(cols[0][0][r], cols[0][1][r], cols[0][2][r]) for r in idx]

    # refusals: nothing is launched, so the poisoned output stays poisoned
    b = G.Bufs(gpu, 0xFF)
    s, t, e = b.inp(torch.from_numpy(score)), b.inp(torch.from_numpy(time)), b.inp(torch.from_numpy(event))
    ws, out = b.out((nb,), torch.uint8, name="ws"), b.out((P, 4), torch.int64, name="counts")

    def rc(*, s_=s.data_ptr(), t_=t.data_ptr(), e_=e.data_ptr(), ix_=None, base=0, n_=n, P_=P, out_=out.data_ptr(), ws_=ws.data_ptr(), nb_=nb, si=P, sp=1):
        return lib.amds_concordance_counts(s_, si, sp, t_, n, e_, n, ix_, base, n_, P_, out_, ws_, nb_, G.cur_stream())

    assert rc(nb_=nb - 1) == -2 and b"workspace" in lib.amds_last_error()           # AMDS_ERR_WORKSPACE
    assert rc(ws_=ws.data_ptr() + 8, nb_=nb) == -1                                  # not 256-byte aligned
    for bad in (dict(s_=None), dict(t_=None), dict(e_=None), dict(out_=None), dict(ws_=None), dict(n_=0), dict(P_=0), dict(si=0), dict(sp=-1),
                dict(ix_=s.data_ptr(), base=0)):
        assert rc(**bad) == -1, bad                                                 # AMDS_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == -1).all())
    # an out-of-range index fails the call (and is never dereferenced: the base problem ends where the guard band begins)
    bad_idx = idx.copy()
    bad_idx[2, 333] = n
    bad_idx[0, 0] = -5
    ix = b.inp(torch.from_numpy(bad_idx), name="bad idx")
    ws2, out2 = b.out((nb_idx,), torch.uint8, name="ws_idx"), b.out((4, 4), torch.int64, name="counts_idx")
    got = lib.amds_concordance_counts(s.data_ptr(), P, 1, t.data_ptr(), 0, e.data_ptr(), 0, ix.data_ptr(), n, 700, 4, out2.data_ptr(), ws2.data_ptr(), nb_idx,
                                      G.cur_stream())
    assert got == -1 and b"2 index value(s) lie outside" in lib.amds_last_error()
    torch.cuda.synchronize()
    for h in b.handles:
        h.assert_bands_intact()


# ---- fit(monitor="val_cindex") ------------------------------------------------------------------------------------------------------------------------
TIMES = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 6.0]
EVENTS = [1, 1, 1, 1, 1, 1, 0]
# validation scores per epoch (patient k's score in column k): epoch 1 ranks everyone right with tiny margins (C = 1, a Cox loss near the uninformed
# one), epoch 2 swaps the first two patients with wide margins (C < 1, the lowest Cox loss), epoch 3 ranks right again (C = 1: a tie with epoch 1)
SCRIPT = [[0.0, 0.3, 0.1, 0.5, 0.2, 0.4, 0.1],
          [0.07, 0.06, 0.05, 0.04, 0.03, 0.02, 0.01],
          [15.0, 18.0, 12.0, 9.0, 6.0, 3.0, 0.0],
          [0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1],
          [0.0, 0.3, 0.1, 0.5, 0.2, 0.4, 0.1],
          [0.0, 0.3, 0.1, 0.5, 0.2, 0.4, 0.1]]


class _Scripted:
    """The object `fit` drives: the score of a bag is SCRIPT[epoch][patient], the patient's number being the bag's first feature; all on the device."""

    def __init__(self, gpu, script):
        self.dev = gpu
        self.table = torch.tensor(script, dtype=torch.float32, device=gpu)
        self.ended = 0                              # epochs finished: the training steps of epoch e read row e, its validation (after epoch_end) too
        self.P = torch.zeros(1, device=gpu)
        self.synced = None
        self.ragged_calls = 0

    def _scores(self, row, first):
        return self.table[row][first.long()][:, None]

    def step(self, bags, targets, cw, coords=None, loss_fn=None):
        return torch.tensor(0.5, device=self.dev), self._scores(self.ended, bags[:, 0, 0]) + 100.0

    def epoch_end(self):
        self.ended += 1
        self.P = self.P + 1.0                       # "weights" after epoch e: e + 1

    def predict(self, bags, coords=None):
        return self._scores(self.ended - 1, bags[:, 0, 0])

    def predict_ragged(self, bags, coords=None):
        self.ragged_calls += 1
        return self._scores(self.ended - 1, torch.stack([b[0, 0] for b in bags]))

    def _refresh(self):
        pass

    def sync_to_model(self):
        self.synced = self.P.clone()


def _scripted_run(gpu, script, events=EVENTS, **kw):
    from stamp_amd import mil_train
    st = _Scripted(gpu, script)

    def bag(ks, tiles):
        return torch.tensor(ks, dtype=torch.float32)[:, None, None].expand(len(ks), tiles, 2).contiguous()

    def tgt(ks):
        return torch.tensor([[TIMES[k], float(events[k])] for k in ks])

    def train_batches():
        return [(bag(ks, 4), None, None, tgt(ks)) for ks in ([0, 1, 2], [3, 4, 5, 6])]

    def valid_batches():                            # one-bag batches of different lengths and one batch of two bags
        return [(bag(ks, tiles), None, None, tgt(ks)) for ks, tiles in (([0], 3), ([1], 5), ([2, 3], 2), ([4], 1), ([5], 4), ([6], 2))]

    hist = mil_train.fit(st, train_batches, valid_batches, max_epochs=len(script), loss_fn=lambda lg, t: lg.sum(), monitor="val_cindex", **kw)
    return st, hist


def _expected(script, events=EVENTS):
    from stamp_amd import losses
    ci = [float(np.float32(R.c_of(R.pair_counts(row, TIMES, events)))) for row in script]
    cox = [losses.cox_breslow_loss(torch.tensor(row), torch.tensor(TIMES), torch.tensor(events)).item() for row in script]
    return ci, cox


def test_fit_selects_the_first_epoch_of_maximal_cindex_not_of_minimal_cox_loss(gpu):
    ci, cox = _expected(SCRIPT)
    assert ci[1] == ci[3] == 1.0 and max(ci) == 1.0 and int(np.argmin(cox)) == 2 and ci[2] < 1.0          # the script does what its comment says
    st, hist = _scripted_run(gpu, SCRIPT, patience=3)
    assert hist["val_cindex"] == ci[:5]
    # (fp32 on the device against fp32 on the host: the log-sum-exp of epoch 2 is near 18, where fp32's spacing is 1.9e-6, and exp / log differ by a few ulp)
    assert hist["val_cox_loss"] == pytest.approx(cox[:5], abs=1e-5) and hist["validation_loss"] == hist["val_cox_loss"]
    assert hist["best_epoch"] == 1 and hist["stopped_epoch"] == 4                   # patience 3 counted from epoch 1: epochs 2, 3, 4 do not improve
    assert float(st.synced) == 2.0 and float(st.P) == 2.0                           # the weights after epoch 1 are back
    # train_pred_median: torch.median over all 7 training-step scores of the epoch (the stub's steps return the row + 100)
    assert hist["train_pred_median"] == [torch.tensor(row).add(100.0).median().item() for row in SCRIPT[:5]]
    assert st.train_pred_median == hist["train_pred_median"][-1]
    # patience 1: stops one epoch after the best one
    _, h1 = _scripted_run(gpu, SCRIPT, patience=1)
    assert h1["best_epoch"] == 1 and h1["stopped_epoch"] == 2 and len(h1["val_cindex"]) == 3


def test_fit_grouped_validation_gives_the_same_history(gpu):
    _, h1 = _scripted_run(gpu, SCRIPT, patience=3)
    st, h4 = _scripted_run(gpu, SCRIPT, patience=3, valid_bags_per_call=4)
    assert st.ragged_calls > 0 and h4 == h1


def test_fit_without_events_raises_and_a_nan_epoch_stops_the_loop(gpu):
    with pytest.raises(RuntimeError, match="val_cindex"):
        _scripted_run(gpu, SCRIPT, events=[0] * 7, patience=3)
    nan = float("nan")
    script = [SCRIPT[0], SCRIPT[2], [nan] * 7, SCRIPT[1]]
    st, hist = _scripted_run(gpu, script, patience=3)
    assert len(hist["val_cindex"]) == 3 and np.isnan(hist["val_cindex"][2]) and hist["stopped_epoch"] == 2
    assert hist["best_epoch"] == 1 and float(st.synced) == 2.0                      # the best finite epoch is restored
    st, hist = _scripted_run(gpu, [[nan] * 7, SCRIPT[1]], patience=3)
    assert hist["best_epoch"] == -1 and hist["stopped_epoch"] == 0 and float(st.synced) == 1.0          # no finite epoch: the last trained weights stay


def test_fit_val_cindex_on_a_real_survival_head(gpu):
    from stamp_amd import losses, metrics
    from stamp_amd.mil import VisionTransformer
    from stamp_amd.mil_train import HipMilVitTrainer, fit

    Fd = 64
    g = torch.Generator().manual_seed(31)
    n_pat = 12
    risk = torch.randn(n_pat, generator=g)
    times = torch.exp(-risk) * (0.5 + torch.rand(n_pat, generator=g))
    events = (torch.rand(n_pat, generator=g) < 0.7).float()
    events[0] = 1.0
    y = torch.stack([times, events], 1)
    feats = [torch.randn(int(t), Fd, generator=g) + risk[k] for k, t in enumerate(torch.randint(20, 61, (n_pat,), generator=g))]
    train = [(torch.stack([feats[k][:16] for k in ks]), None, None, y[ks]) for ks in ([0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11])]
    valid = [(feats[k][None], None, None, y[k:k + 1]) for k in range(n_pat)]
    torch.manual_seed(0)
    model = VisionTransformer(dim_output=1, dim_input=Fd, dim_model=64, n_layers=1, n_heads=2, dim_feedforward=64, dropout=0.0, use_alibi=False)
    tr = HipMilVitTrainer(model, device=gpu, max_lr=3e-3, total_steps=6, sched_interval="step", dropout=False)
    steps, preds = [], []
    step0, predict0 = tr.step, tr.predict

    def step(*a, **kw):
        loss, lg = step0(*a, **kw)
        steps.append(lg.detach().clone())
        return loss, lg

    def predict(*a, **kw):
        lg = predict0(*a, **kw)
        preds.append(lg.detach().clone())
        return lg
    tr.step, tr.predict = step, predict
    hist = fit(tr, lambda: train, lambda: valid, max_epochs=3, patience=8, loss_fn=losses.cox_survival_loss, monitor="val_cindex")
    tr.step, tr.predict = step0, predict0
    assert all(len(hist[k]) == 3 for k in ("val_cindex", "val_cox_loss", "train_pred_median", "validation_loss", "train_loss"))
    assert len(steps) == 6 and len(preds) == 3 * n_pat
    yd = y.to(gpu)
    for ep in range(3):
        s = torch.cat(preds[ep * n_pat:(ep + 1) * n_pat]).reshape(-1)
        assert hist["val_cindex"][ep] == metrics.concordance_index(s, yd[:, 0], yd[:, 1]).item()
        assert hist["val_cindex"][ep] == float(np.float32(R.c_of(R.pair_counts(s.cpu().numpy(), times.numpy(), events.numpy()))))
        assert hist["val_cox_loss"][ep] == losses.cox_breslow_loss(s, yd[:, 0], yd[:, 1]).item()
        assert hist["train_pred_median"][ep] == torch.cat(steps[2 * ep:2 * ep + 2]).reshape(-1).median().item()
    best = hist["best_epoch"]
    assert best == int(np.argmax(hist["val_cindex"])) and tr.train_pred_median == hist["train_pred_median"][-1]
    after = torch.cat([tr.predict(b.to(gpu)) for b, *_ in valid]).reshape(-1)
    assert torch.equal(after, torch.cat(preds[best * n_pat:(best + 1) * n_pat]).reshape(-1))


def test_fit_valid_auroc_on_a_three_class_toy_run(gpu):
    from stamp_amd import metrics
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

    def predict(*a, **kw):
        lg = predict0(*a, **kw)
        preds.append(lg.detach().clone())
        return lg
    tr.predict = predict
    hist = fit(tr, lambda: train, lambda: valid, max_epochs=2, patience=8, valid_auroc=True)
    assert len(hist["validation_auroc"]) == 2 and "val_cindex" not in hist and "train_pred_median" not in hist
    for ep in range(2):
        lg = torch.cat(preds[ep * 12:(ep + 1) * 12])
        assert hist["validation_auroc"][ep] == metrics.multiclass_auroc(torch.softmax(lg.float(), dim=1), cls.to(gpu))[1].item()
