"""amds_objective_step / amds_objective_rows (csrc/objective.hip) and what is built on them -- `train_ops.objective_step` / `objective_rows`,
`FlatTrainer.step(objective="library")`, `mil_train.fit(objective="library")`, `crossval(objective="library")` -- on the GPU.

Values: every loss and every dlogits tensor of the case list (tests/objective_cases.py) against the fp64 oracle (tests/objective_oracle.py).  The bar of a case
is 4 x the error of `stamp_amd.losses` evaluated in fp32 on the CPU on the same inputs against the same oracle (the margin the project gives its other fp32
kernels over torch's own arithmetic: operation orders differ), but not below a floor of a handful of fp32 roundings -- 8 * 2^-24 * max(|loss|, 1) for a loss,
2^-20 relative L2 for a gradient -- which alone applies where torch's error is 0 or NaN (the +-90 scores overflow its unshifted fp32 exp).  A gradient whose
oracle is all zeros (a single item; one event with nobody else at risk) has no norm to be relative to: the bar is then absolute, 2^-20 (its entries are
differences of O(1) terms).  Every case prints `OBJ name ...` with the kernel's and torch's errors; profiles/objective_kernel_errors.txt is that list.

Bits: a row's loss is the same alone, among N rows and as a one-row step; repeated calls agree; a power-of-two dlogits scale is exact; `epoch_acc` is the
Python-double sum; nothing is written outside the outputs (tests/guarded.py)."""
import functools
import math

import numpy as np
import pytest
import torch

import guarded as G
import objective_cases as OC
import objective_oracle as O

pytestmark = pytest.mark.gpu

CASES = OC.cases()
LOSS_FLOOR = 8 * 2.0 ** -24
GRAD_FLOOR = 2.0 ** -20


def loss_floor(loss: float) -> float:
    return LOSS_FLOOR * max(abs(loss), 1.0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (oracle loss, oracle grad, oracle has_grad, torch-fp32 loss error, torch-fp32 relative gradient error), computed once per case on the CPU."""
    kind, x, y, w = CASES[name]
    loss, grad, has_grad = O.step(kind, x.numpy(), y.numpy(), None if w is None else w.numpy())
    t_loss, t_grad = OC.torch_loss(kind, x, y, w, torch.float32)
    t_loss_err = abs(float(t_loss) - loss)
    t_grad_err = grad_error(np.zeros_like(grad) if t_grad is None else t_grad.double().numpy(), grad)
    return loss, grad, has_grad, t_loss_err, t_grad_err


def grad_error(got: np.ndarray, ref: np.ndarray) -> float:
    n = float(np.linalg.norm(ref))
    return float(np.linalg.norm(got.reshape(ref.shape) - ref)) / (n if n > 0 else 1.0)


def bar(torch_err: float, floor: float) -> float:
    return max(4.0 * torch_err, floor) if math.isfinite(torch_err) else floor


def run_step(gpu, name, **kw):
    from stamp_amd import train_ops as T
    kind, x, y, w = CASES[name]
    return T.objective_step(kind, x.to(gpu), y.to(gpu), None if w is None else w.to(gpu), **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_step_against_the_fp64_oracle(gpu, name):
    from stamp_amd import _lib
    assert _lib.lib().amds_objective_max_items() == OC.COX_LIMIT
    loss, grad, has_grad, t_loss_err, t_grad_err = reference(name)
    k_loss, k_grad, k_has = run_step(gpu, name)
    k_loss, k_grad_np, k_has = float(k_loss), k_grad.double().cpu().numpy(), int(k_has)
    loss_err, g_err = abs(k_loss - loss), grad_error(k_grad_np, grad)
    loss_bar, g_bar = bar(t_loss_err, loss_floor(loss)), bar(t_grad_err, GRAD_FLOOR)
    print(f"OBJ {name:34s} loss {loss:13.6e}  kernel err {loss_err:9.3e}  torch fp32 err {t_loss_err:9.3e}  bar {loss_bar:9.3e} | "
          f"dlogits rel-L2 kernel {g_err:9.3e}  torch fp32 {t_grad_err:9.3e}  bar {g_bar:9.3e}")
    assert math.isfinite(k_loss) and np.isfinite(k_grad_np).all()
    assert k_has == has_grad
    if has_grad == 0:
        assert k_loss == 0.0 and not k_grad_np.any()
    assert loss_err <= loss_bar, (loss_err, loss_bar)
    assert g_err <= g_bar, (g_err, g_bar)
    again = run_step(gpu, name)
    assert torch.equal(again[0], torch.as_tensor(k_loss, device=gpu)) and torch.equal(again[1], k_grad) and int(again[2]) == k_has


def test_cox_item_limit(gpu):
    from stamp_amd import _lib, train_ops as T
    n = T.objective_max_items() + 1
    for kind in (T.OBJ_COX_EFRON, T.OBJ_COX_BRESLOW):
        with pytest.raises(RuntimeError, match="at most 4096"):
            T.objective_step(kind, torch.zeros(n, 1, device=gpu), torch.ones(n, 2, device=gpu))
        assert b"at most 4096" in _lib.lib().amds_last_error()
        with pytest.raises(RuntimeError, match="CE and L1"):
            T.objective_rows(kind, torch.zeros(4, 1, device=gpu), torch.ones(4, 2, device=gpu))


def _rows_inputs(kind, N, gpu):
    g = torch.Generator().manual_seed(50 + N)
    if kind == O.CE:
        C = 5
        x = torch.randn(N, C, generator=g) * 3
        y = torch.softmax(torch.randn(N, C, generator=g), 1)
        w = torch.rand(C, generator=g) + 0.5
        return x.to(gpu), y.to(gpu), w.to(gpu)
    x, y = torch.randn(N, 1, generator=g), torch.randn(N, generator=g)
    y[::5] = x[::5, 0]
    return x.to(gpu), y.to(gpu), None


@pytest.mark.parametrize("kind", [O.CE, O.L1])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 4097])
def test_rows_have_the_bits_of_one_row_calls_and_of_one_row_steps(gpu, kind, N):
    from stamp_amd import train_ops as T
    x, y, w = _rows_inputs(kind, N, gpu)
    rows = T.objective_rows(kind, x, y, w)
    assert torch.equal(rows, T.objective_rows(kind, x, y, w))
    ref = O.rows(kind, x.cpu().numpy(), y.cpu().numpy(), None if w is None else w.cpu().numpy())
    assert np.abs(rows.double().cpu().numpy() - ref).max() <= LOSS_FLOOR * max(np.abs(ref).max(), 1.0)
    pick = range(N) if N <= 257 else list(range(0, N, 41)) + [N - 1]          # (4097: a hundred rows spread over every workgroup position, and the last)
    alone = torch.stack([T.objective_rows(kind, x[n:n + 1], y[n:n + 1], w)[0] for n in pick])
    steps = torch.stack([T.objective_step(kind, x[n:n + 1], y[n:n + 1], w)[0] for n in pick])
    want = rows[torch.as_tensor(list(pick), device=gpu)]
    assert torch.equal(alone.view(torch.int32), want.view(torch.int32)), "a row evaluated alone differs from the row among N"
    assert torch.equal(steps.view(torch.int32), want.view(torch.int32)), "the B = 1 step loss differs from the row's value"


@pytest.mark.parametrize("name", ["ce-65x5-soft-w-n3", "l1-65", "efron-65-ties-most", "breslow-65-ties-most"])
def test_power_of_two_scale_is_exact_from_host_and_device(gpu, name):
    base = run_step(gpu, name)[1]
    host = run_step(gpu, name, scale=1024.0)[1]
    dev = run_step(gpu, name, scale_dev=torch.tensor(1024.0, device=gpu))[1]
    want = (base * 1024.0).view(torch.int32)
    assert base.abs().max() > 0 and torch.equal(host.view(torch.int32), want) and torch.equal(dev.view(torch.int32), want)
    both = run_step(gpu, name, scale=4.0, scale_dev=torch.tensor(256.0, device=gpu))[1]
    assert torch.equal(both.view(torch.int32), want)


def test_epoch_acc_holds_the_python_double_sum(gpu):
    from stamp_amd import train_ops as T
    acc = torch.zeros(2, dtype=torch.float64, device=gpu)
    g = torch.Generator().manual_seed(9)
    tot, cnt = 0.0, 0
    for B in (64, 64, 7):
        x, y = (torch.randn(B, 3, generator=g) * 3).to(gpu), torch.softmax(torch.randn(B, 3, generator=g), 1).to(gpu)
        loss, _, _ = T.objective_step(T.OBJ_CE, x, y, epoch_acc=acc)
        tot += float(loss) * B
        cnt += B
    assert acc.tolist() == [tot, 135.0] and cnt == 135
    # a Cox batch without an event adds its zero loss and its size, as `fit` counts it
    T.objective_step(T.OBJ_COX_EFRON, torch.randn(5, 1, device=gpu), torch.tensor([[1.0, 0.0]] * 5, device=gpu), epoch_acc=acc)
    assert acc.tolist() == [tot, 140.0]


@pytest.mark.parametrize("name", ["ce-65x5-soft-w-n3", "ce-3x1024-onehot-now-pm80", "l1-65", "efron-300-ties-most", "breslow-300-censored_ties-most",
                                  "efron-7-ties-none"])
def test_nothing_is_written_outside_the_outputs(gpu, name):
    """Inputs inside guard bands, outputs poisoned on entry inside guard bands: bands intact, outputs independent of the poison, finite."""
    from stamp_amd import _lib
    kind, x, y, w = CASES[name]
    B, C = x.shape
    lib = _lib.lib()

    def call(pattern):
        b = G.Bufs(gpu, pattern)
        xg, yg = b.inp(x, name="logits"), b.inp(y.reshape(B, -1), name="targets")
        wg = None if w is None else b.inp(w, name="weight")
        acc = b.inp(torch.tensor([1.5, 2.0], dtype=torch.float64), name="epoch_acc")
        loss, has = b.out((1,), torch.float32, name="loss"), b.out((1,), torch.int32, name="has_grad")
        dl = b.out((B, C), torch.float32, name="dlogits")
        _lib.check(lib.amds_objective_step(kind, xg.data_ptr(), yg.data_ptr(), G.ptr(wg), B, C, 1.0, None, loss.data_ptr(), dl.data_ptr(), has.data_ptr(),
                                           acc.data_ptr(), G.cur_stream()), "objective_step")
        outs = dict(loss=loss, dlogits=dl, has_grad=has, epoch_acc=acc)
        if kind in (O.CE, O.L1):
            rows = b.out((B,), torch.float32, name="rows")
            _lib.check(lib.amds_objective_rows(kind, xg.data_ptr(), yg.data_ptr(), G.ptr(wg), B, C, rows.data_ptr(), G.cur_stream()), "objective_rows")
            outs["rows"] = rows
        return b.result(**outs)

    first = G.run_contract(call)
    loss, grad, has_grad, _, _ = reference(name)
    assert abs(float(first["loss"]) - loss) <= 4 * loss_floor(loss) and int(first["has_grad"]) == has_grad
    assert first["epoch_acc"].tolist() == [1.5 + float(first["loss"]) * B, 2.0 + B]


# ---- trainer level: the MLP head, F = 32, hidden 16, C = 3, batch 8, dropout off: exact fp32 and tiny ---------------------------------------------------
F_IN, HID, N_CLS, BATCH = 32, 16, 3, 8


def _mlp(gpu, dim_out=N_CLS, seed=11, **kw):
    from stamp_amd.mil import MLP
    from stamp_amd.mlp_train import HipMlpTrainer
    torch.manual_seed(seed)
    model = MLP(dim_input=F_IN, dim_hidden=HID, dim_output=dim_out, num_layers=2, dropout=0.0)
    return HipMlpTrainer(model, device=gpu, max_lr=1e-2, total_steps=64, sched_interval="step", dropout=False, **kw)


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm())


def _targets(task, g):
    from stamp_amd import losses
    if task == "ce":
        return None, torch.nn.functional.one_hot(torch.randint(0, N_CLS, (BATCH,), generator=g), N_CLS).float(), torch.tensor([0.5, 1.0, 2.0])
    if task == "l1":
        return losses.l1_loss, torch.randn(BATCH, generator=g), None
    t = torch.stack([torch.randint(1, 4, (BATCH,), generator=g).float(), (torch.rand(BATCH, generator=g) < 0.6).float()], 1)
    t[0, 1] = 1.0
    return (losses.cox_survival_loss if task == "efron" else losses.cox_slide_survival_loss), t, None


@pytest.mark.parametrize("task", ["ce", "l1", "efron", "breslow"])
def test_library_step_leaves_the_torch_steps_gradients(gpu, task):
    g = torch.Generator().manual_seed(21)
    loss_fn, targets, weights = _targets(task, g)
    tr = _mlp(gpu, dim_out=N_CLS if task == "ce" else 1)
    feats = torch.randn(BATCH, F_IN, generator=g).to(gpu)
    P0 = tr.P.clone()
    loss_t, logits_t = tr.step(feats, targets, weights, update=False, loss_fn=loss_fn)
    G_t = tr.G.clone()
    tr.G.zero_()
    loss_l, logits_l = tr.step(feats, targets, weights, update=False, loss_fn=loss_fn, objective="library")
    assert loss_l.is_cuda and loss_l.dim() == 0 and torch.equal(logits_t, logits_l) and torch.equal(tr.P, P0) and tr.step_count == 0
    print(f"{task}: loss torch {float(loss_t):.8f} library {float(loss_l):.8f}")
    assert abs(float(loss_l) - float(loss_t)) <= loss_floor(float(loss_t))
    # A Cox loss does not change when every score moves by one constant, so its dlogits add up to exactly 0 and the output bias's gradient -- their sum --
    # holds nothing but the rounding residue of either route: it has no norm of its own to be relative to, and is judged against the sum of the magnitudes
    # it is made of, |dlogits|_1.
    from stamp_amd import train_ops as T
    from stamp_amd.flat_trainer import objective_kind
    cancels = tr.prefixes[-1] + ".bias" if task in ("efron", "breslow") else None
    l1_norm = float(T.objective_step(objective_kind(loss_fn), logits_l, targets.to(gpu))[1].double().abs().sum())
    for k in tr.names:
        o, c = tr.offs[k]
        if k == cancels:
            r = float((tr.G[o:o + c].double() - G_t[o:o + c].double()).norm()) / l1_norm
            print(f"  {k}: |difference| / |dlogits|_1 {r:.3e} (exact value 0)")
        else:
            r = _rel(tr.G[o:o + c], G_t[o:o + c])
            print(f"  {k}: rel-L2 {r:.3e}")
        assert r <= GRAD_FLOOR, (k, r)
    # and a full step applies AdamW once and counts the batch into the epoch's sums
    tr.epoch_acc.zero_()
    loss_u, _ = tr.step(feats, targets, weights, loss_fn=loss_fn, objective="library")
    assert tr.step_count == 1 and not torch.equal(tr.P, P0) and tr.epoch_acc.tolist() == [float(loss_u) * BATCH, float(BATCH)]


@pytest.mark.parametrize("task", ["efron", "breslow"])
def test_cox_batch_without_events_takes_no_step_under_library(gpu, task):
    from stamp_amd import losses
    loss_fn = losses.cox_survival_loss if task == "efron" else losses.cox_slide_survival_loss
    tr = _mlp(gpu, dim_out=1)
    g = torch.Generator().manual_seed(22)
    feats = torch.randn(BATCH, F_IN, generator=g).to(gpu)
    live = torch.stack([torch.arange(BATCH).float(), torch.ones(BATCH)], 1)
    tr.step(feats, live, loss_fn=loss_fn, objective="library")          # one real step: m, v and the clock hold something
    state = [t.clone() for t in (tr.P, tr.m, tr.v)]
    count, pos = tr.step_count, tr.clock.pos
    loss, _ = tr.step(feats, torch.stack([torch.arange(BATCH).float(), torch.zeros(BATCH)], 1), loss_fn=loss_fn, objective="library")
    assert float(loss) == 0.0 and count == tr.step_count == 1 and pos == tr.clock.pos
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(state, (tr.P, tr.m, tr.v)))


def test_vit_head_folds_its_loss_scale_into_the_launch(gpu):
    """`HipMilVitTrainer` at "high": fp16 operands, dlogits x the device-resident 2^10 -- by `_scale_dlogits` after autograd or inside amds_objective_step."""
    from stamp_amd.mil import VisionTransformer
    from stamp_amd.mil_train import HipMilVitTrainer
    torch.manual_seed(31)
    model = VisionTransformer(dim_output=2, dim_input=64, dim_model=64, n_layers=1, n_heads=1, dim_feedforward=64, dropout=0.0, use_alibi=False)
    tr = HipMilVitTrainer(model, device=gpu, precision="high", dropout=False)
    assert tr._ls is not None and tr._dlogits_scale()[1] is tr._ls_scale and tr.current_loss_scale == 1024.0
    g = torch.Generator().manual_seed(32)
    bags = torch.randn(4, 64, 64, generator=g).half().to(gpu)
    targets = torch.nn.functional.one_hot(torch.arange(4) % 2, 2).float()
    loss_t, _ = tr.step(bags, targets, update=False, seed=1)
    G_t = tr.G.clone()
    tr.G.zero_()
    loss_l, _ = tr.step(bags, targets, update=False, seed=1, objective="library")
    assert abs(float(loss_l) - float(loss_t)) <= loss_floor(float(loss_t))
    for k in tr.names:
        o, c = tr.offs[k]
        if float(G_t[o:o + c].norm()) == 0.0:
            assert not tr.G[o:o + c].any()
            continue
        r = _rel(tr.G[o:o + c], G_t[o:o + c])
        print(f"  {k}: rel-L2 {r:.3e}")
        assert r <= GRAD_FLOOR, (k, r)
    sta = HipMilVitTrainer(model, device=gpu, precision="high", dropout=False, dynamic_loss_scale=False)
    assert sta._dlogits_scale() == (1024.0, None)


# ---- fit level: the same MLP, 40 resident entries, 3 epochs ----------------------------------------------------------------------------------------------
N_ENT = 40


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    from stamp_amd import h5io
    from stamp_amd.bags import PatientData
    from stamp_amd.cohort import ResidentFeatureTable
    d = tmp_path_factory.mktemp("objective_entries")
    rng = np.random.default_rng(5)
    labels = ["a", "b", "c"]
    data = {}
    for i in range(N_ENT):
        x = (rng.standard_normal(F_IN) + (i % 3)).astype(np.float16)
        p = d / f"e{i:02d}.h5"
        h5io.write_slide_features(p, x[None], encoder="test", precision="fp16", code_hash="0", stamp_version="2.5.0", feat_type="slide")
        data[f"e{i:02d}"] = PatientData(ground_truth=labels[i % 3], feature_files=[p])
    return data, lambda gpu: ResidentFeatureTable(list(data.values()), task="classification", device=gpu)


def _fit(gpu, tab, objective, per_call, block=True):
    from stamp_amd.mil_train import fit
    tr = _mlp(gpu, seed=12)
    view = tab._all()
    vb = view.valid_batches()
    if not block:
        inner = vb
        vb = lambda: inner()          # noqa: E731  (the same iteration without a `block` method)
    weights = torch.tensor([1.0, 0.5, 2.0])
    return fit(tr, view.train_batches(BATCH, generator=torch.Generator().manual_seed(3)), vb, max_epochs=3, patience=3, class_weights=weights,
               valid_bags_per_call=per_call, objective=objective)


def test_fit_histories_do_not_depend_on_the_validation_grouping(gpu, table):
    tab = table[1](gpu)
    h1 = _fit(gpu, tab, "library", 1)
    h40_iter = _fit(gpu, tab, "library", 40, block=False)
    h40_block = _fit(gpu, tab, "library", 40)
    h16_block = _fit(gpu, tab, "library", 16)
    print("library:", h1)
    assert h1 == h40_iter == h40_block == h16_block
    assert all(math.isfinite(v) for v in h1["train_loss"] + h1["validation_loss"]) and len(h1["validation_loss"]) == 3
    ht = _fit(gpu, tab, "torch", 1)
    print("torch:  ", ht)
    # epoch 0 only: its weights are still driven by near-identical gradients; later epochs may drift by rounding
    assert abs(h1["validation_loss"][0] - ht["validation_loss"][0]) <= loss_floor(ht["validation_loss"][0]) * N_ENT


def test_fit_library_regression_and_survival_run(gpu, table):
    from stamp_amd import losses
    from stamp_amd.mil_train import fit
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(N_ENT, F_IN, generator=g).to(gpu)

    def batches(targets, size):
        return lambda: ((feats[a:a + size], None, None, targets[a:a + size]) for a in range(0, N_ENT, size))

    y = torch.randn(N_ENT, generator=g)
    hists = [fit(_mlp(gpu, dim_out=1, seed=13), batches(y, BATCH), batches(y, k), max_epochs=2, loss_fn=losses.l1_loss, valid_bags_per_call=1, objective="library")
             for k in (1, 5)]
    assert hists[0] == hists[1] and all(math.isfinite(v) for v in hists[0]["validation_loss"])
    te = torch.stack([torch.randint(1, 9, (N_ENT,), generator=g).float(), (torch.arange(N_ENT) % 3 > 0).float()], 1)
    hs = fit(_mlp(gpu, dim_out=1, seed=14), batches(te, BATCH), batches(te, 1), max_epochs=2, loss_fn=losses.cox_survival_loss, monitor="val_cindex",
             objective="library")
    assert all(math.isfinite(v) for v in hs["train_loss"] + hs["val_cindex"]) and len(hs["train_pred_median"]) == 2


def test_crossval_runs_two_folds_under_library(gpu, table, tmp_path):
    from stamp_amd import crossval as X
    data = table[0]
    ids = list(data)
    splits = [{"train_patients": [p for j, p in enumerate(ids) if j % 2 != k], "test_patients": [p for j, p in enumerate(ids) if j % 2 == k]} for k in range(2)]

    def make(*, fold, dim_feats, categories, class_weights):
        assert dim_feats == F_IN and len(categories) == N_CLS
        return _mlp(gpu, seed=40 + fold)

    res = X.crossval(data, task="classification", make_trainer=make, splits=splits, output_dir=tmp_path / "cv", batch_size=BATCH, max_epochs=2,
                     ground_truth_label="KRAS", device=gpu, generator=torch.Generator().manual_seed(0), valid_bags_per_call=20, predict_bags_per_call=20,
                     objective="library")
    assert len(res.histories) == 2 and all(math.isfinite(v) for h in res.histories for v in h["train_loss"] + h["validation_loss"])
    assert sorted(p for preds in res.predictions for p in preds) == ids
    assert all(torch.isfinite(p).all() and p.shape == (N_CLS,) for preds in res.predictions for p in preds.values())
