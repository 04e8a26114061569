"""The one-call MLP / Linear heads on the GPU (csrc/mlp.hip, stamp_amd/mlp_core.py, mlp_train.py, cohort.ResidentFeatureTable, crossval, deploy) against
tests/mlp_oracle.py in fp64.

Bars: the ones tests/test_gpu_mil.py holds this head's module path to, relative L2 per tensor -- logits 1e-5, gradients 2e-5 at "highest", 1e-4 at "high".
Inputs: fp16-valued features (so the fp16 and the fp32 store hold the same numbers and must give the same bits), weights of torch's Linear scale, and NO
hidden pre-activation within tau = 2^-15 (|a| |W|^T + |b| + 1) of the ReLU's kink (`_clear_of_the_relu_kink`, the rule of tests/test_gpu_abmil.py): ReLU'
jumps at 0, and an element whose |z| is below the arithmetic's rounding has no gradient fp64 could pin.
Shapes: five geometries (odd widths; the reference's default on CHIEF's width; `Linear` 1 536 -> 4; the widest input; three layers) x rows 1, 13, 64, 65, 200: one row, a partial 16-row tile, the last row count whose K slices run as separate workgroups,
the first that walks them in one wave, several row tiles with a partial last one; widths that are multiples of nothing (37, 29, 3) next to the reference's.
Every figure is printed before it is asserted."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import guarded as G
import mlp_oracle as O

pytestmark = pytest.mark.gpu

GEOMS = {"odd": (37, 29, 3, 4), "chief": (768, 512, 2, 2), "linear": (1536, 1, 4, 1), "wide": (2560, 512, 1, 2), "small": (96, 16, 2, 3)}
ROWS = [1, 13, 64, 65, 200]
P_DROP, SEED = 0.25, 4242
BAR_LOGITS, BAR_GRAD, BAR_GRAD_HIGH = 1e-5, 2e-5, 1e-4


def _layer_dims(dims):
    Fd, H, Cc, L = dims
    return [Fd if i == 0 else H for i in range(L)], [Cc if i == L - 1 else H for i in range(L)]


def _weights(dims, seed=0):
    g = torch.Generator().manual_seed(50 + seed)
    ins, outs = _layer_dims(dims)
    ws = [(torch.rand(o, i, generator=g) * 2 - 1) / i ** 0.5 for i, o in zip(ins, outs)]
    bs = [(torch.rand(o, generator=g) * 2 - 1) / i ** 0.5 for i, o in zip(ins, outs)]
    return ws, bs


def _clear_of_the_relu_kink(x, ws, bs, masks, scale):
    """Shifts hidden biases (by multiples of 2 tau, the smallest that works) until no hidden pre-activation lies within tau of zero; layer by layer, since a
    layer's input depends on the biases below it."""
    a = x.double()
    for i in range(len(ws) - 1):
        W, b = ws[i].double(), bs[i].double().clone()
        mag = a.abs() @ W.abs().T
        z0 = a @ W.T
        for l in range(W.shape[0]):
            for k in range(4000):
                d = ((k + 1) // 2) * (1 if k % 2 else -1)
                tau = 2.0 ** -15 * (mag[:, l] + b[l].abs() + 1.0)
                bl = b[l] + d * 2.0 * float(tau.max())
                if bool(((z0[:, l] + bl).abs() >= tau).all()):
                    b[l] = bl
                    break
            else:
                raise AssertionError(f"no clear bias for unit {l} of layer {i}")
        bs[i] = b.float()
        z = a @ W.T + bs[i].double()
        assert bool((z.abs() >= 2.0 ** -16 * (mag + 1.0)).all())
        a = torch.clamp(z, min=0.0)
        if masks is not None:
            a = a * masks[i].double().cpu() * scale


_CASES: dict = {}


def _case(geom, rows, p, gpu):
    """-> dict(x fp16-valued fp32 [rows, F], ws, bs, masks (0/1 uint8 on the host) or None, scale, dlogits, ref = fp64 logits / dWs / dbs / dx), computed once."""
    key = (geom, rows, p)
    if key not in _CASES:
        from stamp_amd import _lib
        from stamp_amd import train_ops as T
        dims = GEOMS[geom]
        ws, bs = _weights(dims)
        g = torch.Generator().manual_seed(1000 + rows)
        x = (torch.randn(rows, dims[0], generator=g) * 0.7).half().float()
        masks, scale = None, 1.0
        if p > 0 and dims[3] > 1:
            masks = [T.dropout_mask(rows * dims[1], p, SEED, i, gpu).view(rows, dims[1]).cpu() for i in range(dims[3] - 1)]
            scale = float(_lib.lib().amds_dropout_keep_scale(C.c_float(p)))
        _clear_of_the_relu_kink(x, ws, bs, masks, scale)
        dl = torch.randn(rows, dims[2], generator=g)
        logits, cache = O.forward(x, ws, bs, masks, scale)
        dWs, dbs, dx = O.backward(cache, dl)
        _CASES[key] = dict(x=x, ws=ws, bs=bs, masks=masks, scale=scale, dlogits=dl, ref=dict(logits=logits, dWs=dWs, dbs=dbs, dx=dx))
    return _CASES[key]


def _struct(ws, bs, gpu):
    from stamp_amd import mlp_core
    return mlp_core.weights_struct([w.to(gpu).contiguous() for w in ws], [b.to(gpu).contiguous() for b in bs])


def _store(x, dtype, gpu, ld=None):
    """x on the GPU in `dtype`; ld: a row stride wider than F (the view of a wider buffer filled with NaN)."""
    x = x.to(gpu, dtype)
    if ld is None:
        return x
    wide = torch.full((x.shape[0], ld), float("nan"), dtype=dtype, device=gpu)
    wide[:, :x.shape[1]] = x
    return wide[:, :x.shape[1]]


def _run(case, dims, xg, w, p, need_x=True):
    from stamp_amd import mlp_core
    logits, saved = mlp_core.forward_train(w, dims, xg, p=p, seed=SEED)
    Gd, dx = mlp_core.backward(saved, case["dlogits"].to(xg.device), need_params=True, need_x=need_x)
    return logits, Gd, dx


def _check(tag, got_logits, Gd, dx, ref, bar_grad):
    figs = {"logits": (O.rel_l2(got_logits, ref["logits"]), BAR_LOGITS), "dx": (O.rel_l2(dx, ref["dx"]), bar_grad)}
    for i, (dw, db) in enumerate(zip(*Gd)):
        figs[f"dW{i}"] = (O.rel_l2(dw, ref["dWs"][i]), bar_grad)
        figs[f"db{i}"] = (O.rel_l2(db, ref["dbs"][i]), bar_grad)
    print(tag, " ".join(f"{k}={v:.2e}" for k, (v, _) in figs.items()))
    bad = {k: v for k, (v, bar) in figs.items() if not v < bar}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_three_calls_against_fp64(gpu, geom, rows):
    """1. Logits, every weight and bias gradient and dx against the fp64 oracle, at p = 0 and p = 0.25 with the masks `MLP.dropout_masks` reads back; the fp16 and
    the fp32 store (the 13-row case through a row stride of F + 3, which also takes every operand load off the 16-byte path) give the same bits; the eval
    forward equals the training forward at p = 0."""
    from stamp_amd import mlp_core, ops
    dims = GEOMS[geom]
    ld = dims[0] + 3 if rows == 13 else None
    for p in ((0.0, P_DROP) if dims[3] > 1 else (0.0,)):
        case = _case(geom, rows, p, gpu)
        w, _keep = _struct(case["ws"], case["bs"], gpu)
        x16, x32 = _store(case["x"], torch.float16, gpu, ld), _store(case["x"], torch.float32, gpu, ld)
        lg16, G16, dx16 = _run(case, dims, x16, w, p)
        lg32, G32, dx32 = _run(case, dims, x32, w, p)
        _check(f"{geom} rows={rows} p={p} fp16-store", lg16, G16, dx16, case["ref"], BAR_GRAD)
        assert torch.equal(lg16, lg32) and torch.equal(dx16, dx32) and all(torch.equal(a, b) for a, b in zip(G16[0] + G16[1], G32[0] + G32[1]))
        _, G_only, none = _run(case, dims, x16, w, p, need_x=False)          # dx not asked for: not computed, the gradients unchanged
        assert none is None and all(torch.equal(a, b) for a, b in zip(G16[0] + G16[1], G_only[0] + G_only[1]))
        if p == 0.0:
            assert torch.equal(mlp_core.forward_infer(w, dims, x16), lg16) and torch.equal(mlp_core.forward_infer(w, dims, x32), lg16)
        if rows == 64:          # the backward may follow torch's matmul precision: the bar at "high"; the forward never changes
            with ops.float32_matmul_precision("high"):
                lgh, Gh, dxh = _run(case, dims, x16, w, p)
            _check(f"{geom} rows={rows} p={p} high", lgh, Gh, dxh, case["ref"], BAR_GRAD_HIGH)
            assert torch.equal(lgh, lg16)


def test_masks_are_the_modules_and_the_drop_rate_is_p(gpu):
    from stamp_amd.mil import MLP
    m = MLP(dim_input=96, dim_hidden=512, dim_output=2, num_layers=3, dropout=P_DROP).to(gpu)
    masks = m.dropout_masks(200, SEED)
    case = _case("chief", 200, P_DROP, gpu)
    assert torch.equal(masks[0].cpu(), case["masks"][0].bool())          # the oracle's masks ARE `MLP.dropout_masks` (site = hidden layer, element = row * cols + col)
    rate = 1.0 - masks[0].float().mean().item()
    print(f"realised drop rate at 200 x 512: {rate:.4f}")
    assert abs(rate - P_DROP) < 0.01


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_a_logits_row_depends_on_its_own_features_only(gpu, geom):
    """2. Bitwise: row i of a 200-row call = its own one-row call = its row in a call over a permutation of the rows = its row in the 13-, 64- and 65-row
    calls; the same for the training forward at p = 0."""
    from stamp_amd import mlp_core
    dims = GEOMS[geom]
    case = _case(geom, 200, 0.0, gpu)
    w, _keep = _struct(case["ws"], case["bs"], gpu)
    x = case["x"].to(gpu, torch.float16)
    perm = torch.randperm(200, generator=torch.Generator().manual_seed(3)).to(gpu)
    for name, fwd in (("eval", lambda t: mlp_core.forward_infer(w, dims, t)), ("train p=0", lambda t: mlp_core.forward_train(w, dims, t, p=0.0, seed=0)[0])):
        full = fwd(x)
        for i in (0, 57, 199):
            assert torch.equal(fwd(x[i:i + 1])[0], full[i]), (name, i)
        assert torch.equal(fwd(x[perm]), full[perm]), name
        for n in (13, 64, 65):
            assert torch.equal(fwd(x[:n]), full[:n]), (name, n)
            assert torch.equal(fwd(x[200 - n:]), full[200 - n:]), (name, n)


def test_workspaces_saved_block_and_flat_gradients_are_contained(gpu, monkeypatch):
    """3. Guard bands around workspace, saved block, the flat gradient buffer, dx and logits stay intact; a workspace poisoned with 0x00 or 0xFF gives the same bits."""
    from stamp_amd import _lib, mlp_core
    for geom, rows in (("odd", 13), ("chief", 64), ("small", 200)):
        dims = GEOMS[geom]
        case = _case(geom, rows, P_DROP, gpu)
        w, _keep = _struct(case["ws"], case["bs"], gpu)
        ins, outs = _layer_dims(dims)
        sizes = [n for i, o in zip(ins, outs) for n in (o * i, o)]          # state_dict order: weight, bias per layer

        def call(pattern):
            with G.scratch_hook(monkeypatch, pattern) as log:
                b = G.Bufs(gpu, pattern)
                x = b.inp(case["x"].half(), ld=dims[0] + 5, name="x")
                flat = b.out((sum(sizes),), torch.float32, name="flat G")
                views, o = [], 0
                for n in sizes:
                    views.append(flat[o:o + n])
                    o += n
                grads, _k = mlp_core.weights_struct(views[0::2], views[1::2], _lib.MlpGrads)
                logits, saved = mlp_core.forward_train(w, dims, x, p=P_DROP, seed=SEED)
                _, dx = mlp_core.backward(saved, case["dlogits"].to(gpu), grads=grads, need_x=True)
                ev = mlp_core.forward_infer(w, dims, x)
                torch.cuda.synchronize()
                log.assert_bands_intact()
                assert {t for t, _ in log.requests} >= {"mlp", "mlp_train", "alloc"}
                return b.result(logits=logits, flat=flat, dx=dx, eval_logits=ev)

        out = G.run_contract(call)
        e = O.rel_l2(out["logits"], case["ref"]["logits"])
        print(f"{geom} rows={rows}: guarded logits rel-L2 {e:.2e}")
        assert e < BAR_LOGITS


def test_two_identical_steps_leave_identical_state(gpu):
    from stamp_amd.mil import MLP
    from stamp_amd.mlp_train import HipMlpTrainer
    torch.manual_seed(12)
    model = MLP(dim_input=768, dim_hidden=512, dim_output=2, num_layers=2, dropout=P_DROP)
    x = torch.randn(64, 768, device=gpu).half()
    y = torch.nn.functional.one_hot(torch.arange(64) % 2, 2).float().to(gpu)
    states = []
    for _ in range(2):
        tr = HipMlpTrainer(model, device=gpu, max_lr=1e-3, total_steps=8, sched_interval="step")
        for s in range(2):
            tr.step(x, y, seed=77 + s)
        states.append((tr.P.clone(), tr.m.clone(), tr.v.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*states)) and not torch.equal(states[0][0], HipMlpTrainer(model, device=gpu).P)


def test_bad_configurations_are_refused_before_any_launch(gpu):
    from stamp_amd import _lib, mlp_core
    lib = _lib.lib()
    dims = GEOMS["small"]
    case = _case("small", 13, 0.0, gpu)
    w, _keep = _struct(case["ws"], case["bs"], gpu)
    x = case["x"].to(gpu)
    logits = torch.full((13, dims[2]), 7.0, device=gpu)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=gpu)
    stream = torch.cuda.current_stream().cuda_stream

    def fwd(cfg, xp, ld, wp=C.byref(w), out=logits.data_ptr()):
        return lib.amds_mlp_forward(C.byref(cfg), wp, xp, _lib.F32, ld, 13, out, ws.data_ptr(), ws.numel(), stream)

    good = _lib.MlpCfg(*dims)
    assert fwd(good, x.data_ptr(), dims[0]) == 0
    torch.cuda.synchronize()
    want = logits.clone()
    logits.fill_(7.0)
    nine = _lib.MlpCfg(dims[0], dims[1], dims[2], 9)
    assert fwd(nine, x.data_ptr(), dims[0]) == -1 and b"num_layers=9" in lib.amds_last_error()          # AMDS_ERR_INVALID
    assert lib.amds_mlp_workspace_bytes(C.byref(nine), 13) == 0 and lib.amds_mlp_train_saved_bytes(C.byref(nine), 13) == 0
    assert fwd(good, None, dims[0]) == -1 and fwd(good, x.data_ptr(), dims[0], wp=None) == -1 and fwd(good, x.data_ptr(), dims[0], out=None) == -1
    assert fwd(good, x.data_ptr(), dims[0] - 1) == -1 and b"row stride" in lib.amds_last_error()
    assert lib.amds_mlp_forward(C.byref(good), C.byref(w), x.data_ptr(), _lib.F32, dims[0], 13, logits.data_ptr(), ws.data_ptr(), 16, stream) == -2      # AMDS_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((logits == 7.0).all())          # nothing was launched
    with pytest.raises(ValueError, match="1 to 8 layers"):
        mlp_core.forward_infer(w, (dims[0], dims[1], dims[2], 9), x)
    # rows == 0 succeeds without a launch
    assert mlp_core.forward_infer(w, dims, x[:0]).shape == (0, dims[2])
    assert fwd(good, x.data_ptr(), dims[0]) == 0
    torch.cuda.synchronize()
    assert torch.equal(logits, want)


def test_trainer_follows_the_module_path_under_adamw_and_onecycle(gpu):
    """4. Five steps of HipMlpTrainer(dropout=False) against mil.MLP + torch.optim.AdamW under the same OneCycle values on the same batches."""
    from stamp_amd import ops
    from stamp_amd.mil import MLP
    from stamp_amd.mlp_train import HipMlpTrainer
    torch.manual_seed(21)
    kw = dict(dim_input=768, dim_hidden=512, dim_output=2, num_layers=2, dropout=P_DROP)
    model, ref = MLP(**kw), MLP(**kw)
    ref.load_state_dict(model.state_dict())
    ref = ref.to(gpu).train()
    ref.dropout_p = 0.0
    tr = HipMlpTrainer(model, device=gpu, max_lr=1e-3, div_factor=25.0, total_steps=8, weight_decay=0.01, dropout=False, sched_interval="step")
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, total_steps=8, max_lr=1e-3, div_factor=25.0)
    g = torch.Generator().manual_seed(5)
    cw = torch.tensor([0.3, 0.7], device=gpu)
    for s in range(5):
        x = torch.randn(64, 768, generator=g).half().to(gpu)
        y = torch.nn.functional.one_hot(torch.randint(0, 2, (64,), generator=g), 2).float().to(gpu)
        loss, logits = tr.step(x, y, cw)
        opt.zero_grad()
        out = ref(x)
        lref = torch.nn.functional.cross_entropy(out, y, weight=cw)
        lref.backward()
        opt.step()
        sched.step()
        print(f"step {s}: loss {float(loss):.6f} / {lref.item():.6f} logits rel-L2 {O.rel_l2(logits, out.detach()):.2e}")
    tr.sync_to_model()
    for (k, a), (_, b) in zip(model.state_dict().items(), ref.state_dict().items()):
        e = O.rel_l2(a, b)
        print(f"{k}: weights rel-L2 {e:.2e}")
        assert e < 1e-5, k
    xe = torch.randn(33, 768, generator=g).half().to(gpu)
    with torch.no_grad():
        e = O.rel_l2(tr.predict(xe), model.to(gpu).eval()(xe))
    print(f"predict vs model.eval(): {e:.2e}")
    assert e < 1e-5
    # a [B, T, F] batch takes the step of its pooled [B, F] batch, bit for bit
    bags = torch.randn(16, 9, 768, generator=g).half().to(gpu)
    y = torch.nn.functional.one_hot(torch.arange(16) % 2, 2).float().to(gpu)
    a, b = HipMlpTrainer(model, device=gpu, dropout=False), HipMlpTrainer(model, device=gpu, dropout=False)
    la, lga = a.step(bags, y)
    lb, lgb = b.step(ops.mean_pool(bags.contiguous()), y)
    assert torch.equal(la, lb) and torch.equal(lga, lgb) and torch.equal(a.P, b.P) and torch.equal(a.G, b.G)
    assert torch.equal(a.predict(bags), a.predict(ops.mean_pool(bags.contiguous())))


# ---- 5. / 6.: fit and crossval on files ----------------------------------------------------------------------------------------------------------------------
N_FIT, F_FIT = 120, 96


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """120 entries x 96-d, planted so that a linear rule separates the classes: x = noise + s * direction, s = +-1.5 by class; regression target and survival
    time follow the same projection."""
    from stamp_amd import h5io
    d = tmp_path_factory.mktemp("planted")
    rng = np.random.default_rng(8)
    direction = rng.standard_normal(F_FIT)
    direction /= np.linalg.norm(direction)
    labels = ["pos" if i % 2 else "neg" for i in range(N_FIT)]
    files, proj = [], []
    for i in range(N_FIT):
        x = (rng.standard_normal(F_FIT) * 0.5 + (1.5 if labels[i] == "pos" else -1.5) * direction + 0.3 * rng.standard_normal() * direction).astype(np.float16)
        proj.append(float(x.astype(np.float64) @ direction))
        p = d / f"e{i:03d}.h5"
        h5io.write_slide_features(p, x if i % 2 else x[None], encoder="test", precision="fp16", code_hash="0", stamp_version="2.5.0", feat_type="slide" if i < 60 else "patient")
        files.append(p)
    return files, labels, proj


def _pdata(files, gts):
    from stamp_amd.bags import PatientData
    return [PatientData(ground_truth=g, feature_files=[f]) for f, g in zip(files, gts)]


def _mlp_trainer(gpu, dim_in, dim_out, seed, steps=64, linear=False):
    from stamp_amd.mil import MLP, Linear
    from stamp_amd.mlp_train import HipMlpTrainer
    torch.manual_seed(seed)
    model = Linear(dim_in, dim_out) if linear else MLP(dim_input=dim_in, dim_hidden=32, dim_output=dim_out, num_layers=2, dropout=P_DROP)
    return HipMlpTrainer(model, device=gpu, max_lr=1e-2, total_steps=steps, sched_interval="step")


def test_fit_on_a_resident_feature_table(gpu, planted):
    from stamp_amd import bags as B
    from stamp_amd import losses
    from stamp_amd.cohort import ResidentFeatureTable
    from stamp_amd.mil_train import fit
    files, labels, proj = planted
    table = ResidentFeatureTable(_pdata(files, labels), task="classification", device=gpu)
    assert table.dtype == torch.float16 and tuple(table.feats.shape) == (N_FIT, F_FIT) and table.categories == ["neg", "pos"]
    train, valid = table.view(range(0, 90)), table.view(range(90, 120))
    first = next(iter(train.train_batches(32, generator=torch.Generator().manual_seed(1))()))
    order = torch.randperm(90, generator=torch.Generator().manual_seed(1))[:32]
    assert first[0].dtype == torch.float32 and torch.equal(first[0], table.feats[order.to(gpu)].float()) and first[1] is None and first[2] is None
    assert torch.equal(first[3], table.targets[order].to(gpu))
    assert [b[0].shape[0] for b in train.train_batches(32)()] == [32, 32, 26]          # the tail batch
    weights = B.class_weights(table.targets[train.entries], table.categories)
    hists = []
    for per_call in (1, 64):
        tr = _mlp_trainer(gpu, F_FIT, 2, seed=3)
        torch.manual_seed(99)          # the dropout seeds of the steps
        hists.append(fit(tr, train.train_batches(32, generator=torch.Generator().manual_seed(2)), valid.valid_batches(), max_epochs=6, patience=6, class_weights=weights,
                         valid_bags_per_call=per_call, valid_auroc=True))
    print("classification:", json.dumps(hists[0]))
    assert hists[0] == hists[1]                                                          # the one-call validation gives the default loop's history, best_epoch included
    assert max(hists[0]["validation_auroc"]) > 0.9
    # the validation loss of a one-call validation is the unweighted mean of the per-entry cross-entropies: the reference's batch-1 mean
    tr = _mlp_trainer(gpu, F_FIT, 2, seed=3)
    torch.manual_seed(99)
    h1 = fit(tr, train.train_batches(32, generator=torch.Generator().manual_seed(2)), valid.valid_batches(), max_epochs=1, valid_bags_per_call=30)
    lg = tr.predict(table.feats[90:120])
    ce = torch.nn.functional.cross_entropy(lg, table.targets[90:120].to(gpu), reduction="none")
    mean = sum(float(v) for v in ce.tolist()) / 30
    print(f"validation loss {h1['validation_loss'][0]:.8f} vs mean of per-entry CE {mean:.8f}")
    assert abs(h1["validation_loss"][0] - mean) < 1e-6
    # regression and survival run and improve on their first epoch
    reg = ResidentFeatureTable(_pdata(files, [2.0 * v for v in proj]), task="regression", device=gpu)
    tr = _mlp_trainer(gpu, F_FIT, 1, seed=4)
    torch.manual_seed(98)
    hr = fit(tr, reg.view(range(90)).train_batches(32, generator=torch.Generator().manual_seed(2)), reg.view(range(90, 120)).valid_batches(), max_epochs=6, patience=6,
             loss_fn=losses.l1_loss, valid_bags_per_call=64)
    print("regression:", json.dumps(hr))
    assert min(hr["validation_loss"][1:]) < hr["validation_loss"][0] and all(np.isfinite(hr["validation_loss"]))
    surv = ResidentFeatureTable(_pdata(files, [(float(np.exp(-0.8 * v)) * 10.0, "dead" if i % 4 else "alive") for i, v in enumerate(proj)]), task="survival", device=gpu)
    tr = _mlp_trainer(gpu, F_FIT, 1, seed=5, linear=True)
    hs = fit(tr, surv.view(range(90)).train_batches(32, generator=torch.Generator().manual_seed(2)), surv.view(range(90, 120)).valid_batches(), max_epochs=6, patience=6,
             loss_fn=losses.cox_survival_loss, monitor="val_cindex", valid_bags_per_call=64)
    print("survival:", json.dumps(hs))
    assert max(hs["val_cindex"][1:]) > hs["val_cindex"][0] and tr.train_pred_median is not None


@pytest.mark.parametrize("kind", ["slide", "patient"])
def test_crossval_on_feature_vectors(gpu, planted, tmp_path, kind):
    """6. 60 entries x 3 folds of slide-level (entries 0-59) or patient-level (60-119) files."""
    from stamp_amd import crossval as X
    from stamp_amd import deploy
    from stamp_amd.bags import PatientData
    from stamp_amd.cohort import ResidentFeatureTable
    files, labels, _ = planted
    lo = 0 if kind == "slide" else 60
    data = {f"e{i:03d}": PatientData(ground_truth=labels[i], feature_files=[files[i]]) for i in range(lo, lo + 60)}
    ids = list(data)
    splits = [{"train_patients": [p for j, p in enumerate(ids) if j % 3 != k], "test_patients": [p for j, p in enumerate(ids) if j % 3 == k]} for k in range(3)]
    made = []

    def make(*, fold, dim_feats, categories, class_weights):
        made.append(fold)
        return _mlp_trainer(gpu, dim_feats, len(categories), seed=30 + fold, steps=16)

    out = tmp_path / "cv"
    torch.manual_seed(7)
    res = X.crossval(data, task="classification", make_trainer=make, splits=splits, output_dir=out, batch_size=16, max_epochs=3, ground_truth_label="KRAS", device=gpu,
                     generator=torch.Generator().manual_seed(0), valid_bags_per_call=32, predict_bags_per_call=32)
    assert made == [0, 1, 2] and isinstance(res.cohort, ResidentFeatureTable) and len(res.cohort) == 60
    assert X.read_splits(out / "splits.json") == res.splits
    seen = []
    for i, (s, frame, preds) in enumerate(zip(res.splits, res.frames, res.predictions)):
        d = out / f"split-{i}"
        assert (d / "model.pt").exists() and json.loads((d / "history.json").read_text()) == res.histories[i] and (d / "patient-preds.csv").exists()
        assert list(frame.columns) == ["PATIENT", "KRAS", "pred", "KRAS_neg", "KRAS_pos", "loss"] and set(preds) == set(s["test_patients"])
        seen += list(preds)
    assert sorted(seen) == ids
    print(f"{kind}: test-fold accuracy {np.mean([float(f['KRAS'].eq(f['pred']).mean()) for f in res.frames]):.3f}")
    assert all(p.shape == (2,) and abs(float(p.sum()) - 1) < 1e-5 for preds in res.predictions for p in preds.values())
    boom = lambda **kw: (_ for _ in ()).throw(AssertionError("a finished fold was trained again"))  # noqa: E731
    res2 = X.crossval(data, task="classification", make_trainer=boom, splits=splits, output_dir=out, batch_size=16, max_epochs=3, ground_truth_label="KRAS", device=gpu)
    assert res2.cohort is None and all(a.to_csv(index=False) == b.to_csv(index=False) for a, b in zip(res.frames, res2.frames))
    # a loaded fold model: 32 rows a call = the one-row loop, bit for bit (and = the run's own predictions)
    model, doc = X.load_fold_model(out / "split-2" / "model.pt")
    assert doc["head"] == "MLP" and doc["head_kwargs"]["dim_input"] == F_FIT
    order = {p: j for j, p in enumerate(p for s in res.splits for p in ids if p in set(s["test_patients"]))}
    view = res.cohort.view([order[p] for p in res.predictions[2]])
    one = deploy.predict_(model, view.valid_batches()(), list(res.predictions[2]), task="classification", device=gpu)
    many = deploy.predict_(model, view.valid_batches()(), list(res.predictions[2]), task="classification", device=gpu, bags_per_call=32)
    assert all(torch.equal(one[p], many[p]) and torch.equal(one[p], res.predictions[2][p]) for p in one)
