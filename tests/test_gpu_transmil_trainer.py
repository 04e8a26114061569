"""`HipTransMilTrainer` on the GPU: the PPEG unpack kernel against torch slicing; one step against the `nn.Module` path (the same library calls on the same
values: bit for bit); AdamW + OneCycle against torch's; dropout seeds; `mil_train.fit` (classification, grouped ragged validation, C-index selection);
the HBM-resident cohort feeding it."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import guarded as gd
from stamp_amd import _lib, losses, metrics, ops
from stamp_amd import train_ops as T
from stamp_amd.mil import TransMIL
from stamp_amd.mil_train import fit
from stamp_amd.transmil_train import HipTransMilTrainer
from transmil_trainer_cases import PPEG_NAMES, feeds, patients, ppeg_windows

pytestmark = pytest.mark.gpu

# The bar tests/test_gpu_transmil_ragged.py applies to ragged against one-bag logits at "highest" (its BAR = 4 x E0, E0 = 7.463e-7 measured there).
RAGGED_BAR = 4 * 7.463e-7


@contextlib.contextmanager
def _precision(level):
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(level)
    try:
        yield
    finally:
        torch.set_float32_matmul_precision(old)


def _model(C_=2, dim_input=128, dim_hidden=64, seed=0):
    torch.manual_seed(seed)
    m = TransMIL(dim_output=C_, dim_input=dim_input, dim_hidden=dim_hidden)
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return m


def _batch(gpu, Bb=3, Tn=50, Fd=128, C_=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Bb, Tn, Fd, generator=g).to(gpu), torch.nn.functional.one_hot(torch.arange(Bb) % C_, C_).float().to(gpu)


# ---- 1. the unpack kernel ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cd", [64, 512])
def test_ppeg_grads_unpack_equals_torch_slicing_in_guarded_buffers(gpu, Cd):
    """All six outputs `torch.equal` the slicing of `transmil_core.backward` (restated in `ppeg_windows`, pinned on the CPU), under both poison bytes, with
    every byte outside the outputs untouched; 64 channels = one workgroup, 512 = eight."""
    table = torch.randn(50, Cd, generator=torch.Generator().manual_seed(Cd))
    want = ppeg_windows(table)

    def call(pattern):
        b = gd.Bufs(gpu, pattern)
        corr = b.inp(table, name="corr")
        outs = {k: b.out(tuple(want[k].shape), torch.float32, name=k) for k in PPEG_NAMES}
        T.ppeg_grads_unpack(corr, *[outs[k] for k in PPEG_NAMES])
        return b.result(**outs)

    got = gd.run_contract(call)
    for k in PPEG_NAMES:
        assert torch.equal(got[k].cpu(), want[k]), k


def test_ppeg_grads_unpack_refuses_null_and_misaligned_pointers(gpu):
    lib = _lib.lib()
    Cd = 64
    corr = torch.randn(50, Cd, device=gpu)
    outs = [torch.full((Cd * k + 4,), 3.0, device=gpu) for k in (49, 25, 9, 1, 1, 1)]
    ptrs = [o.data_ptr() for o in outs]
    for i in range(7):
        args = [corr.data_ptr()] + ptrs
        args[i] = None
        assert lib.amds_ppeg_grads_unpack(args[0], Cd, *args[1:], ops._stream()) == -1 and b"null" in lib.amds_last_error(), i
    assert lib.amds_ppeg_grads_unpack(corr.data_ptr(), Cd, ptrs[0] + 4, *ptrs[1:], ops._stream()) == -1 and b"aligned" in lib.amds_last_error()
    assert lib.amds_ppeg_grads_unpack(corr.data_ptr(), 6, *ptrs, ops._stream()) == -1 and b"multiple of 4" in lib.amds_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 3.0).all()) for o in outs)          # a refused call launched nothing


# ---- 2. + 6. one step equals the module path, at both precisions -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("Tn", [50, 300])
def test_step_equals_the_module_path_bit_for_bit(gpu, Tn, precision):
    """Tn = 50: 8 x 8 grid, 65 token rows, fewer than 256 landmarks' worth; Tn = 300: 18 x 18, 325 rows, front padding.  Logits and every gradient
    `torch.equal` those of `loss.backward()` through the module: the same library calls on the same fp32 values (the module's own tensors there, views of
    the flat buffer here)."""
    model = _model().to(gpu).eval()                        # eval: no dropout; the parameters need gradients, so the training kernels run
    bags, targets = _batch(gpu, Tn=Tn)
    tr = HipTransMilTrainer(copy.deepcopy(model), device=gpu, dropout=False)
    with _precision(precision):
        logits = model(bags)
        loss = torch.nn.functional.cross_entropy(logits, targets)
        loss.backward()
        loss_t, logits_t = tr.step(bags, targets, update=False)
    assert logits_t.shape == (3, 2) and torch.isfinite(logits_t).all()
    assert torch.equal(logits_t, logits.detach()) and torch.equal(loss_t, loss.detach())
    for n, p in model.named_parameters():
        assert p.grad is not None and tr.g(n).shape == p.grad.shape, n
        d = (tr.g(n) - p.grad).abs().max().item()
        assert torch.equal(tr.g(n), p.grad), (n, d)
    assert float(tr.G.abs().max()) > 0


# ---- 3. update=False ---------------------------------------------------------------------------------------------------------------------------------------
def test_update_false_leaves_the_state_alone(gpu):
    bags, targets = _batch(gpu)
    tr = HipTransMilTrainer(_model(), device=gpu, dropout=False, sched_interval="step", total_steps=6, max_lr=2e-3)
    tr.step(bags, targets)                                 # one real step first: m, v, step_count and the clock are off their initial values
    assert tr.step_count == 1 and tr.clock.pos == 1 and float(tr.m.abs().max()) > 0
    before = [t.clone() for t in (tr.P, tr.m, tr.v)]
    G0 = tr.G.clone()
    other, _ = _batch(gpu, seed=2)
    loss, logits = tr.step(other, targets, update=False)
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.P, tr.m, tr.v))) and tr.step_count == 1 and tr.clock.pos == 1
    assert not torch.equal(tr.G, G0) and torch.isfinite(loss)          # the gradients ARE this batch's
    # a loss without a gradient (a Cox batch without events) takes no step either way
    tr1 = HipTransMilTrainer(_model(C_=1), device=gpu, dropout=False)
    P0 = tr1.P.clone()
    no_event = torch.stack([torch.arange(3.0), torch.zeros(3)], 1)
    l0, lg0 = tr1.step(bags, no_event, loss_fn=losses.cox_survival_loss)
    assert tr1.step_count == 0 and torch.equal(tr1.P, P0) and lg0.shape == (3, 1) and float(l0) == 0.0


# ---- 4. twelve steps against torch AdamW + OneCycleLR ----------------------------------------------------------------------------------------------------
def test_twelve_steps_match_torch_adamw_and_onecycle(gpu):
    """The reference's `configure_optimizers` (models/__init__.py:133-141) driving the module, stepped per batch, against the trainer's fused AdamW fed torch's
    own lr and beta1 table.  Bars: those of tests/test_gpu_mil_seam.py for the same comparison on the `vit` head (5e-3 relative on the loss curve,
    2e-3 max(1, |q|max) on every parameter); the loss falls by at least 10 %."""
    steps = 12
    model = _model().to(gpu).eval()
    twin = copy.deepcopy(model)
    bags, targets = _batch(gpu, Bb=4)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, total_steps=steps, max_lr=2e-3, div_factor=25.0)
    tr = HipTransMilTrainer(twin, device=gpu, max_lr=2e-3, div_factor=25.0, total_steps=steps, sched_interval="step", dropout=False)
    la, lb = [], []
    for i in range(steps):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(bags), targets)
        loss.backward()
        opt.step()
        if i + 1 < steps:
            sched.step()
        la.append(loss.item())
        lb.append(tr.step(bags, targets)[0].item())
    print("torch AdamW on the module:", [round(v, 5) for v in la])
    print("fused trainer:            ", [round(v, 5) for v in lb])
    assert tr.step_count == steps and tr.clock.pos == steps
    assert lb[-1] < lb[0] * 0.9 and la[-1] < la[0] * 0.9
    assert max(abs(a - b) / max(abs(b), 1e-3) for a, b in zip(la, lb)) < 5e-3
    tr.sync_to_model()
    worst = max(((p - q).abs().max().item() / max(1.0, q.abs().max().item()), n) for (n, p), (_, q) in zip(model.state_dict().items(), twin.state_dict().items()))
    print("largest parameter difference / max(1, |q|max):", worst)
    for (n, p), (_, q) in zip(model.state_dict().items(), twin.state_dict().items()):
        assert (p - q).abs().max().item() < 2e-3 * max(1.0, q.abs().max().item()), n


# ---- 5. dropout ---------------------------------------------------------------------------------------------------------------------------------------------
def test_dropout_seeds(gpu):
    bags, targets = _batch(gpu, Tn=300)
    model = _model()
    tr = HipTransMilTrainer(copy.deepcopy(model), device=gpu)          # dropout=None: the reference's train mode
    _, a = tr.step(bags, targets, update=False, seed=5)
    Ga = tr.G.clone()
    _, b = tr.step(bags, targets, update=False, seed=5)
    assert torch.equal(a, b) and torch.equal(Ga, tr.G)
    _, c = tr.step(bags, targets, update=False, seed=6)
    assert not torch.equal(a, c)
    off = HipTransMilTrainer(copy.deepcopy(model), device=gpu, dropout=False)
    _, d = off.step(bags, targets, update=False, seed=5)
    Gd = off.G.clone()
    _, e = off.step(bags, targets, update=False, seed=6)
    assert torch.equal(d, e) and torch.equal(Gd, off.G) and not torch.equal(a, d)
    # the module's masks: without a seed both draw the step's seed from torch's CPU generator
    module = copy.deepcopy(model).to(gpu).train()
    torch.manual_seed(123)
    want = module(bags)
    torch.nn.functional.cross_entropy(want, targets).backward()
    torch.manual_seed(123)
    _, got = tr.step(bags, targets, update=False)
    assert torch.equal(got, want.detach()) and all(torch.equal(tr.g(n), p.grad) for n, p in module.named_parameters())


# ---- 7. - 9. fit -----------------------------------------------------------------------------------------------------------------------------------------------
N_TRAIN, BATCH, BAG = 24, 8, 32


def _fit_case(gpu, C_=2):
    bags, labels = patients()
    return bags, labels, _model(C_=C_, dim_input=64, seed=3)


def _run_fit(gpu, model, train, valid, **kw):
    tr = HipTransMilTrainer(copy.deepcopy(model), device=gpu, max_lr=2e-3, total_steps=24, sched_interval="step", dropout=kw.pop("dropout", False))
    snaps = []

    def log(msg):
        if msg.startswith("epoch"):
            snaps.append(tr.P.clone())

    torch.manual_seed(17)
    hist = fit(tr, train, valid, max_epochs=8, patience=3, log=log, **kw)
    return tr, hist, snaps


def test_fit_classification(gpu):
    bags, labels, model = _fit_case(gpu)
    assert 0 < int(labels[N_TRAIN:].sum()) < 8
    train, valid = feeds(bags, torch.nn.functional.one_hot(labels, 2).float(), N_TRAIN, BATCH, BAG, gpu)
    tr, hist, snaps = _run_fit(gpu, model, train, valid, valid_auroc=True)
    print("train", hist["train_loss"], "\nvalidation", hist["validation_loss"], "\nauroc", hist["validation_auroc"], "best", hist["best_epoch"])
    vl = hist["validation_loss"]
    assert len(vl) == len(hist["train_loss"]) == len(snaps) == len(hist["validation_auroc"]) and all(np.isfinite(vl))
    assert hist["train_loss"][-1] < hist["train_loss"][0]
    assert hist["best_epoch"] == min(range(len(vl)), key=vl.__getitem__)
    assert hist["skipped_steps"] == [0] * len(vl) and tr.step_count == 3 * len(vl)
    assert torch.equal(tr.P, snaps[hist["best_epoch"]])
    bag = valid()[0][0]
    with torch.no_grad():
        assert torch.equal(tr.model.to(gpu).eval()(bag), tr.predict(bag))


def test_fit_with_grouped_ragged_validation(gpu):
    """`valid_bags_per_call=4` goes through the trainer's `group_valid_bags` hook and `predict_ragged`: rows within the ragged bar of the one-bag logits, so on
    a fixture whose validation loss moves by more than 100 bars an epoch the same epoch is selected."""
    bags, labels, model = _fit_case(gpu)
    train, valid = feeds(bags, torch.nn.functional.one_hot(labels, 2).float(), N_TRAIN, BATCH, BAG, gpu)
    with _precision("highest"):
        tr_a, hist_a, snaps_a = _run_fit(gpu, model, train, valid)
        va = hist_a["validation_loss"]
        steps = [abs(a - b) for a, b in zip(va, va[1:])]
        print("validation", va, "\nsmallest change between epochs", min(steps), "bar", RAGGED_BAR)
        assert min(steps) > 100 * RAGGED_BAR
        tr_b, hist_b, snaps_b = _run_fit(gpu, model, train, valid, valid_bags_per_call=4)
        vb = hist_b["validation_loss"]
        assert len(snaps_a) == len(snaps_b) and all(torch.equal(a, b) for a, b in zip(snaps_a, snaps_b))          # validation does not touch the training
        assert hist_b["best_epoch"] == hist_a["best_epoch"] and torch.equal(tr_a.P, tr_b.P)
        vbags = [b[0] for b, *_ in valid()]
        one = torch.cat([tr_b.predict(b[None]) for b in vbags])
        rows = torch.cat([tr_b.predict_ragged(vbags[a:e]) for a, e in tr_b.group_valid_bags([b.shape[0] for b in vbags], 4)])
        err = (rows - one).abs().max(1).values
        print("ragged rows against one-bag logits:", err.tolist(), "validation loss difference", max(abs(a - b) for a, b in zip(va, vb)))
        assert rows.shape == one.shape and float(err.max()) <= RAGGED_BAR
        # cross-entropy moves by at most 2 max|d logit| (its gradient's L1 norm is at most 2), and so does the mean over the bags
        assert max(abs(a - b) for a, b in zip(va, vb)) <= 2 * RAGGED_BAR + 2 ** -23      # (+ one fp32 ulp of a per-bag loss below 2: each run rounds its own)


def test_fit_monitoring_the_validation_c_index(gpu):
    """Survival: dim_output 1, the Cox loss, targets [time, event]; selection by `val_cindex`.  `fit` restores the BEST epoch, so its `val_cindex` is the
    concordance of `predict` on the restored weights; the LAST epoch's value is checked on that epoch's weights (the same statement when the last epoch is
    the best one).  Dropout live: the loop draws the seeds."""
    bags, labels, model = _fit_case(gpu, C_=1)
    g = torch.Generator().manual_seed(5)
    score = torch.stack([b[:, 0].mean() for b in bags])
    time = (10.0 * torch.exp(-score) + torch.rand(len(bags), generator=g)).round(decimals=3)
    event = (torch.arange(len(bags)) % 3 != 0).float()
    assert int(event[N_TRAIN:].sum()) >= 1
    targets = torch.stack([time, event], 1)
    train, valid = feeds(bags, targets, N_TRAIN, BATCH, BAG, gpu)
    tr, hist, snaps = _run_fit(gpu, model, train, valid, loss_fn=losses.cox_survival_loss, monitor="val_cindex", dropout=None)
    print("val_cindex", hist["val_cindex"], "val_cox_loss", hist["val_cox_loss"], "median", hist["train_pred_median"], "best", hist["best_epoch"])
    n = len(hist["val_cindex"])
    assert n == len(hist["val_cox_loss"]) == len(hist["train_pred_median"]) == len(snaps) and hist["validation_loss"] == hist["val_cox_loss"]
    assert tr.train_pred_median == hist["train_pred_median"][-1] and np.isfinite(tr.train_pred_median)
    ci = hist["val_cindex"]
    assert hist["best_epoch"] == max(range(n), key=lambda i: (ci[i], -i)) and torch.equal(tr.P, snaps[hist["best_epoch"]])
    y = targets[N_TRAIN:].to(gpu)

    def cindex_now():
        s = torch.cat([tr.predict(b) for b, *_ in valid()]).reshape(-1)
        return float(metrics.concordance_index(s, y[:, 0], y[:, 1]).double())

    assert ci[hist["best_epoch"]] == cindex_now()          # the restored weights
    tr.P.copy_(snaps[-1])
    assert ci[-1] == cindex_now()                          # the last epoch's weights


# ---- 10. the resident cohort ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cohort(gpu, tmp_path_factory):
    from stamp_amd import bags as B
    from stamp_amd import h5io
    from stamp_amd.cohort import ResidentCohort
    d = tmp_path_factory.mktemp("transmil_cohort")
    rng = np.random.default_rng(0)
    data = []
    for i, n in enumerate([5, 90, 32, 33, 61, 20, 47, 80, 12, 64, 31, 70]):
        feats = (rng.standard_normal((n, 64)) + (0.5 if i % 2 else -0.5)).astype(np.float16)
        coords = np.stack([rng.integers(0, 40, n), rng.integers(0, 40, n)], 1).astype(np.float32) * 256.0
        p = d / f"p{i}.h5"
        h5io.write_tile_features(p, feats, coords, extractor="test", tile_size_um=256.0, tile_size_px=224, code_hash="0", stamp_version="2.4.0")
        data.append(B.PatientData(ground_truth="pos" if i % 2 else "neg", feature_files=[p]))
    return ResidentCohort(data, task="classification", device=gpu)


def test_resident_cohort_feeds_the_trainer(gpu, cohort):
    """One epoch of `train_batches(8, 32)` -- fp16 rows gathered on the device, taken by the training forward as they are -- equals, bit for bit, the same
    batches materialised first (under the same generator) and fed by hand with the same dropout seeds, as fp16 and as fp32."""
    model = _model(dim_input=64, seed=4)
    make = lambda: HipTransMilTrainer(copy.deepcopy(model), device=gpu, max_lr=2e-3, total_steps=4, sched_interval="step")  # noqa: E731
    feed = cohort.train_batches(batch_size=8, bag_size=32, out_dtype=torch.float16)
    tr_a, tr_b, tr_c = make(), make(), make()
    torch.manual_seed(4)
    out_a = []
    for k, (bags, coords, sizes, targets) in enumerate(feed()):
        assert bags.dtype == torch.float16 and bags.shape[1:] == (32, 64)
        out_a.append(tr_a.step(bags, targets, coords=coords, seed=100 + k))
    torch.manual_seed(4)
    held = [(b.clone(), t.clone()) for b, _c, _s, t in feed()]
    assert len(held) == len(out_a) == 2 and held[1][0].shape[0] == 4
    for k, (b, t) in enumerate(held):
        lb, gb = tr_b.step(b, t, seed=100 + k)
        lc, gc_ = tr_c.step(b.float(), t, seed=100 + k)
        assert torch.equal(lb, out_a[k][0]) and torch.equal(gb, out_a[k][1]) and torch.equal(lc, lb) and torch.equal(gc_, gb), k
    assert tr_a.step_count == 2 and torch.equal(tr_a.P, tr_b.P) and torch.equal(tr_a.P, tr_c.P) and torch.isfinite(tr_a.P).all()
    assert not torch.equal(tr_a.P, make().P)
    # validation: a ragged group is a view of the store and goes to the library as it is
    rb = cohort.ragged_group(1, 8)
    assert rb.feats.untyped_storage().data_ptr() == cohort.feats.untyped_storage().data_ptr()
    listed = [cohort.feats[cohort.offsets[p]:cohort.offsets[p + 1]].clone() for p in range(1, 8)]
    got, want = tr_a.predict_infer_ragged(rb), tr_a.predict_ragged(listed)
    assert got.shape == (7, 2) and torch.isfinite(got).all() and torch.equal(got, want)
    tr_a.sync_to_model()
    with torch.no_grad():
        assert torch.equal(tr_a.model.to(gpu).eval().forward_infer_ragged(rb), got)
    # and `fit` runs from the cohort's two feeds, grouped validation included
    hist = fit(tr_a, feed, cohort.valid_batches(), max_epochs=1, valid_bags_per_call=4)
    assert np.isfinite(hist["train_loss"][0]) and np.isfinite(hist["validation_loss"][0]) and hist["best_epoch"] == 0
