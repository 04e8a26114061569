"""The gated-attention MIL head on the GPU (stamp_amd/abmil.py, csrc/abmil.hip) against tests/abmil_oracle.py in fp64.

Bars.  Per tensor, err = max |hip - fp64| / max |fp64|.
  "highest": the yardstick is the same oracle run by torch in fp32 on the CPU on the same inputs; bar = max(4 x its error, gamma(n)).  The factor 4 is for
             another summation order over up to 257 rows / 1023 rows of a call and K <= 384 terms; gamma(n) (tests/gap_oracle.py) is the floor for a yardstick that
             happens to be exact, n = the longest sum behind the tensor: max(F, L, D, longest bag) for forward tensors, max(that, rows of the call) for the
             gradients (a weight gradient sums over every row of the call).
  "high":    2e-4 relative L2 per tensor: the bar tests/test_gpu_transmil_train.py applies to TransMIL's gradients at "high" (similar products and depth).
A tensor that is zero in exact arithmetic (d c_b always; the six score-path gradients when a bag's rows are equal) is measured against the size of the two
terms that cancel in it instead of against fp64's rounding noise: tests/abmil_oracle.py's docstring.
Every figure is printed before it is asserted (profiles/abmil_kernel_errors.txt holds a run's output).
Row blocks of the kernels: the weight gradients' row chunks (the "long" case); 4 rows a workgroup (one wave per row; the pooling's four row lanes), 256 (the per-bag softmax / d-score stride, the products' row
padding): the ragged case holds 3, 4, 5 and 255, 256, 257 next to the lengths the issue lists.
"""
import copy
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import abmil_oracle as O
import guarded as G

pytestmark = pytest.mark.gpu

GEOMS = {"small": (48, 64, 32, 3), "xs": (384, 256, 256, 2)}
RAGGED = [1, 2, 15, 16, 17, 63, 64, 65, 257, 3, 4, 5, 255, 256]
DENSE = [33, 33, 33]
HIGH_BAR = 2e-4
FWD = ("logits", "attn_raw", "pooled")
GOLD = Path(__file__).resolve().parent / "golden"


def _clear_of_the_relu_kink(x, w):
    """Shifts entries of the fc bias (by multiples of 2 tau, the smallest that works) until no pre-activation z = x Wfc^T + bfc lies within tau of zero,
    tau = 2^-15 (|x| |Wfc|^T + |bfc|) -- four times the rounding a product of "high" may carry (operands of 16+ mantissa bits: 2 x 2^-17 per term).  ReLU's
    derivative jumps at z = 0: an element whose |z| is below the arithmetic's own rounding has no gradient that fp64 could pin, for torch's fp32 and TF32
    products as little as for these kernels (measured before this existed: ONE element with |z| = 1.9e-6 among 65 472 moved dx, dW_fc and db_fc of the
    48/64/32/3 ragged case at "high" from 4e-6 to 2.0e-4 relative L2)."""
    xd, W, b = x.double(), w[O.FC_W].double(), w[O.FC_B].double().clone()
    mag = xd.abs() @ W.abs().T
    z0 = xd @ W.T
    for l in range(W.shape[0]):
        for k in range(2000):
            d = ((k + 1) // 2) * (1 if k % 2 else -1)
            tau = 2.0 ** -15 * (mag[:, l] + b[l].abs() + 1.0)
            bl = b[l] + d * 2.0 * float(tau.max())
            if bool(((z0[:, l] + bl).abs() >= tau).all()):
                b[l] = bl
                break
        else:
            raise AssertionError(f"no clear bias for hidden unit {l}")
    w[O.FC_B] = b.float()
    z = xd @ W.T + w[O.FC_B].double()
    assert bool((z.abs() >= 2.0 ** -16 * (mag + w[O.FC_B].double().abs())).all())


def _case(geom: str, lengths, family: str, seed: int = 0):
    """-> (x fp16-valued fp32 [rows, F], weights), no pre-activation at the ReLU's kink (`_clear_of_the_relu_kink`).  families: "random";
    "peak": one tile of every bag holds about 95 % of its attention: the bag is its best-scoring row and N - 1 copies of the drawn row whose score lies
      closest to ln(19 (N - 1)) nats below it (scores scaled to a spread of 4 nats first).  Why 95 % and not 99.99 %: ds_top = P_top (g_top - sum P g) cancels
      to a (1 - P_top) share of its terms, so every gradient through the score carries the products' rounding times 1 / (1 - P_top); "high" products round at
      about 1e-5 (2^-17 per factor, a few factors deep) and the bar at "high" is 2e-4: a factor 20 = 1 / (1 - 0.95) is what that bar can resolve.
    "equal": every row of a bag is the same row (P = 1 / N)."""
    F, L, D, Cc = GEOMS[geom]
    w = O.random_weights(F, L, D, Cc, seed=11 + seed)
    g = torch.Generator().manual_seed(100 + seed)
    rows = sum(lengths)
    x = (torch.randn(rows, F, generator=g) * 0.7).half().float()
    _clear_of_the_relu_kink(x, w)
    starts = np.cumsum([0] + list(lengths[:-1]))
    if family == "peak":
        s0 = O.forward(x, lengths, w, dtype=torch.float64)["attn_raw"]
        w[O.C_W] = w[O.C_W] * float(4.0 / s0.std())
        s = O.forward(x, lengths, w, dtype=torch.float64)["attn_raw"]
        pool = x.clone()
        for a, n in zip(starts, lengths):
            top = int(a) + int(s[a:a + n].argmax())
            if n > 1:
                other = int((s - (s[top] - np.log(19.0 * (n - 1)))).abs().argmin())
                x[a:a + n] = pool[other]
            x[a] = pool[top]
    if family == "equal":
        x = torch.cat([x[i:i + 1].expand(n, F) for i, n in zip(starts, lengths)]).contiguous()
    return x, w


_REF_CACHE: dict = {}


def _refs(key, x, lengths, w, dlogits, masks=None):
    """fp64 reference and fp32 CPU yardstick of a case, computed once."""
    if key not in _REF_CACHE:
        _REF_CACHE[key] = (O.gradients(x, lengths, w, dlogits, masks, torch.float64), O.gradients(x, lengths, w, dlogits, masks, torch.float32))
    return _REF_CACHE[key]


def _dlogits(bags, Cc, seed=0):
    return torch.randn(bags, Cc, generator=torch.Generator().manual_seed(7 + seed))


def _module(geom, w, gpu, dropout=0.25):
    from stamp_amd.abmil import GatedAttentionMIL
    F, L, D, Cc = GEOMS[geom]
    m = GatedAttentionMIL(F, L, D, Cc, dropout)
    m.load_state_dict(w)
    return m.to(gpu)


def _run_hip(geom, x, lengths, w, dlogits, gpu, p=0.0, seed=0):
    """forward_train + backward through the library on packed ragged rows -> dict like the oracle's."""
    from stamp_amd import abmil
    dims = GEOMS[geom]
    wd = {k: w[k].to(gpu).contiguous() for k in O.KEYS}
    ws, keep = abmil._weights_struct(lambda k: wd[k])
    offs = abmil._offsets(lengths, gpu)
    xg = x.to(gpu)
    logits, saved = abmil.forward_train(ws, dims, xg, offs, len(lengths), p_fc=p, p_gate=p, seed=seed)
    Gd, dx = abmil.backward(saved, dlogits.to(gpu), need_params=True, need_x=True)
    lg2, raw, pooled = abmil.forward_infer(ws, dims, xg, offs, len(lengths), return_attn=True, return_pooled=True)
    res = {"logits": logits, "dx": dx, "eval_logits": lg2, "eval_attn_raw": raw, "eval_pooled": pooled}
    res.update({"g:" + k: Gd[k] for k in O.KEYS})
    return res


def _longest(geom, lengths, grad: bool) -> int:
    F, L, D, _ = GEOMS[geom]
    return max(F, L, D, max(lengths), sum(lengths) if grad else 0)


def _check(tag, geom, lengths, got: dict, ref64: dict, ref32: dict, names, precision):
    bad = []
    for n in names:
        scale = ref64.get("scale:" + n, 0.0)          # used only where the fp64 tensor is zero in exact arithmetic (abmil_oracle's docstring)
        e = O.rel_err(got[n], ref64[n], scale)
        if precision == "highest":
            yard = O.rel_err(ref32[n], ref64[n], scale)
            bar = max(4 * yard, O.gamma(_longest(geom, lengths, n not in FWD)))
            print(f"abmil {tag} {precision} {n}: err {e:.3e} yardstick {yard:.3e} bar {bar:.3e}")
        else:
            r = ref64[n].double().cpu()
            den = float(r.norm())
            if float(r.abs().max()) < 1e-9 * scale:
                den = scale * r.numel() ** 0.5
            e = float((got[n].double().cpu().reshape(r.shape) - r).norm()) / den
            bar = HIGH_BAR
            print(f"abmil {tag} {precision} {n}: rel-L2 {e:.3e} bar {bar:.3e}")
        if not e <= bar:
            bad.append((n, e, bar))
    assert not bad, bad


GRADS = ["dx"] + ["g:" + k for k in O.KEYS]
# "long": 8 400 rows pad to 33 x 256, where the weight gradients' row chunks (512 rows here) leave a shorter last chunk; the ragged case (4 whole chunks) and the
# dense one (a single chunk: the direct product) take the other two paths
LONG = [4200, 4100, 100]
CASES = [("ragged", RAGGED, "random"), ("dense", DENSE, "random"), ("peak", RAGGED, "peak"), ("equal", [1, 2, 17, 65, 257], "equal"), ("long", LONG, "random")]


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_forward_and_every_gradient_against_fp64(gpu, geom, case, precision):
    from stamp_amd import ops
    tag, lengths, family = case
    x, w = _case(geom, lengths, family)
    dl = _dlogits(len(lengths), GEOMS[geom][3])
    ref64, ref32 = _refs((geom, tag), x, lengths, w, dl)
    probs = ref64["probs"].split(lengths)
    if family == "peak":
        assert all(0.90 < float(p.max()) < 0.98 for p, n in zip(probs, lengths) if n > 1), [float(p.max()) for p in probs]
    if family == "equal":
        assert all(torch.allclose(p, torch.full_like(p, 1.0 / n), rtol=1e-12) for p, n in zip(probs, lengths))
    with ops.float32_matmul_precision(precision):
        got = _run_hip(geom, x, lengths, w, dl, gpu)
    got.update({"attn_raw": got["eval_attn_raw"], "pooled": got["eval_pooled"]})
    _check(f"{geom}/{tag}", geom, lengths, got, ref64, ref32, list(FWD) + GRADS, precision)
    assert torch.equal(got["logits"], got["eval_logits"])          # p = 0: the training forward gives the eval path's bits


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_train_mode_with_the_masks_read_back(gpu, geom, precision):
    """Dropout live (p = 0.25): the masks come back through amds_dropout_mask (stream ids 1, 2, 3 over the call's packed rows) and go to the oracle."""
    from stamp_amd import _lib, abmil, ops
    lengths = RAGGED
    x, w = _case(geom, lengths, "random", seed=1)
    dl = _dlogits(len(lengths), GEOMS[geom][3], 1)
    p, seed = 0.25, 2 ** 40 + 12345
    mh, ma, mg = abmil.dropout_masks(sum(lengths), GEOMS[geom], p, p, seed, gpu)
    scale = float(_lib.lib().amds_dropout_keep_scale(p))          # the fp32 factor the kernels multiply by
    assert abs(scale - 1.0 / (1.0 - p)) < 1e-7
    for m in (mh, ma, mg):
        assert abs(float(m.float().mean()) - (1 - p)) < 0.02
    assert not torch.equal(ma, mg)
    masks = tuple(m.cpu().double() * scale for m in (mh, ma, mg))
    ref64, ref32 = _refs((geom, "train"), x, lengths, w, dl, masks)
    with ops.float32_matmul_precision(precision):
        got = _run_hip(geom, x, lengths, w, dl, gpu, p=p, seed=seed)
    _check(f"{geom}/train-p0.25", geom, lengths, got, ref64, ref32, ["logits"] + GRADS, precision)
    assert not torch.equal(got["logits"], got["eval_logits"])


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_each_bags_eval_logits_are_its_own_calls_bits(gpu, geom, precision):
    from stamp_amd import ops
    x, w = _case(geom, RAGGED, "random", seed=2)
    bags = [b.half().to(gpu) for b in x.split(RAGGED)]
    m = _module(geom, w, gpu).eval()
    with torch.no_grad(), ops.float32_matmul_precision(precision):
        together = m.forward_ragged(bags)
        grouped = m.forward_ragged(bags, bags_per_call=4)
        alone = torch.cat([m(b[None]) for b in bags])
        wts, raw = m.attention(bags[8])
    assert together.shape == (len(RAGGED), GEOMS[geom][3]) and torch.equal(together, alone) and torch.equal(grouped, alone)
    assert wts.shape == (257,) and abs(float(wts.sum()) - 1) < 1e-5 and torch.equal(torch.softmax(raw, 0), wts)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_two_runs_give_identical_bits(gpu, geom):
    x, w = _case(geom, RAGGED, "random", seed=3)
    dl = _dlogits(len(RAGGED), GEOMS[geom][3], 3)
    a = _run_hip(geom, x, RAGGED, w, dl, gpu, p=0.25, seed=9)
    b = _run_hip(geom, x, RAGGED, w, dl, gpu, p=0.25, seed=9)
    assert all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])]
    c = _run_hip(geom, x, RAGGED, w, dl, gpu, p=0.25, seed=10)
    assert not torch.equal(a["logits"], c["logits"])


@pytest.mark.parametrize("geom", list(GEOMS))
def test_workspace_and_saved_state_contracts(gpu, geom, monkeypatch):
    """Poisoned on entry (0x00 / 0xFF), exactly the requested sizes, guard bands intact, outputs bit-identical and finite; one byte short is refused."""
    from stamp_amd import _lib, abmil
    lengths = [1, 17, 65, 257, 5]
    x, w = _case(geom, lengths, "random", seed=4)
    dl = _dlogits(len(lengths), GEOMS[geom][3], 4)
    lib, cfg = _lib.lib(), abmil._cfg(GEOMS[geom])
    want = [fn(C.byref(cfg), len(lengths), sum(lengths)) for fn in (lib.amds_abmil_workspace_bytes, lib.amds_abmil_train_saved_bytes, lib.amds_abmil_train_workspace_bytes)]

    def call(pattern):
        with G.scratch_hook(monkeypatch, pattern) as log:
            out = _run_hip(geom, x, lengths, w, dl, gpu, p=0.25, seed=5)
            torch.cuda.synchronize()
        assert log.bytes_for("abmil") == [want[0]] and log.bytes_for("abmil_train") == [want[2], want[2]]
        assert want[1] in log.bytes_for("alloc")
        return G.Result(out, log.handles)

    G.run_contract(call)
    with G.scratch_hook(monkeypatch, 0xFF, short_by=1) as log:
        with pytest.raises(RuntimeError, match="workspace"):
            _run_hip(geom, x, lengths, w, dl, gpu)
        torch.cuda.synchronize()
        log.assert_bands_intact()


def test_bad_arguments_launch_nothing(gpu):
    from stamp_amd import _lib, abmil
    dims = GEOMS["small"]
    lengths = [5, 9]
    x, w = _case("small", lengths, "random")
    wd = {k: w[k].to(gpu).contiguous() for k in O.KEYS}
    ws_, keep = abmil._weights_struct(lambda k: wd[k])
    lib, cfg = _lib.lib(), abmil._cfg(dims)
    xg, offs = x.to(gpu), abmil._offsets(lengths, gpu)
    n_ws = lib.amds_abmil_train_workspace_bytes(C.byref(cfg), 2, 14)
    n_sv = lib.amds_abmil_train_saved_bytes(C.byref(cfg), 2, 14)
    bufs = G.Bufs(gpu, 0xFF)
    wsb, sv = bufs.out((n_ws,), torch.uint8, name="ws"), bufs.out((n_sv,), torch.uint8, name="saved")
    logits, dxb = bufs.out((2, 3), torch.float32, name="logits"), bufs.out((14, 48), torch.float32, name="dx")
    dl = torch.ones(2, 3, device=gpu)
    st = G.cur_stream()
    drop_bad, drop = _lib.AbmilDropout(1.0, 0.25, 1), _lib.AbmilDropout(0.25, 0.25, 1)
    half = _lib.AbmilWeights()
    half.fc_w = ws_.fc_w
    fwd = lambda **k: lib.amds_abmil_forward(C.byref(k.get("cfg", cfg)), C.byref(k.get("w", ws_)), k.get("x", xg.data_ptr()), k.get("dt", _lib.F32), k.get("offs", offs.data_ptr()),  # noqa: E731
                                             k.get("bags", 2), k.get("rows", 14), k.get("logits", logits.data_ptr()), None, None, wsb.data_ptr(), k.get("wsn", n_ws), st)
    cases = [("null logits", dict(logits=None), "null pointer"), ("bad dtype", dict(dt=7), "bad x dtype"), ("no offsets", dict(offs=None), "row_offsets"),
             ("incomplete weights", dict(w=half), "incomplete weights"), ("rows < bags", dict(rows=1), "at least one row"), ("null x", dict(x=None), "null pointer")]
    for name, kw, text in cases:
        rc = fwd(**kw)
        assert rc == -1 and text in lib.amds_last_error().decode(), (name, rc, lib.amds_last_error())
    assert fwd(wsn=lib.amds_abmil_workspace_bytes(C.byref(cfg), 2, 14) - 1) == -2 and "workspace" in lib.amds_last_error().decode()
    tf = lambda d: lib.amds_abmil_train_forward(C.byref(cfg), C.byref(ws_), xg.data_ptr(), _lib.F32, offs.data_ptr(), 2, 14, C.byref(d), logits.data_ptr(), sv.data_ptr(), n_sv,  # noqa: E731
                                                wsb.data_ptr(), n_ws, st)
    assert tf(drop_bad) == -1 and "[0, 1)" in lib.amds_last_error().decode()
    tb = lambda g, dx: lib.amds_abmil_train_backward(C.byref(cfg), C.byref(ws_), xg.data_ptr(), _lib.F32, offs.data_ptr(), 2, 14, C.byref(drop), dl.data_ptr(), sv.data_ptr(), n_sv,  # noqa: E731
                                                     g, dx, wsb.data_ptr(), n_ws, st)
    assert tb(None, None) == -1 and "nothing to compute" in lib.amds_last_error().decode()
    gh = _lib.AbmilGrads()
    assert tb(C.byref(gh), dxb.data_ptr()) == -1 and "incomplete gradient buffers" in lib.amds_last_error().decode()
    torch.cuda.synchronize()
    for t in (wsb, sv, logits, dxb):
        assert bool((t.view(torch.uint8) == 0xFF).all())          # nothing was launched: every byte keeps its poison
    for h in bufs.handles:
        h.assert_bands_intact()
    # the input gradient alone (grads_host NULL) equals the full backward's
    assert tf(drop) == 0 and tb(None, dxb.data_ptr()) == 0
    full = _run_hip("small", x, lengths, w, dl.cpu(), gpu, p=0.25, seed=1)
    assert torch.equal(dxb, full["dx"])


def test_module_autograd_fills_every_grad_and_the_bags(gpu):
    x, w = _case("small", DENSE, "random", seed=5)
    m = _module("small", w, gpu).eval()
    bags = x.view(3, 33, 48).to(gpu).requires_grad_(True)
    y = torch.tensor([0, 2, 1], device=gpu)
    loss = torch.nn.functional.cross_entropy(m(bags, coords=torch.zeros(3, 33, 2, device=gpu)), y)
    loss.backward()
    ref64 = O.gradients(x, DENSE, w, dtype=torch.float64, loss_fn=lambda lg: torch.nn.functional.cross_entropy(lg, y.cpu()))
    ref32 = O.gradients(x, DENSE, w, dtype=torch.float32, loss_fn=lambda lg: torch.nn.functional.cross_entropy(lg, y.cpu()))
    got = {"g:" + k: p.grad for k, p in m.named_parameters()}
    got["dx"] = bags.grad.reshape(-1, 48)
    _check("small/module", "small", DENSE, got, ref64, ref32, GRADS, "highest")
    with pytest.raises(ValueError, match="mask"):
        m(bags, mask=torch.ones(3, 33, dtype=torch.bool, device=gpu))
    with torch.no_grad():
        assert torch.equal(m(bags.detach()), m.forward_ragged(list(bags.detach())))
    m.train()
    torch.manual_seed(0)
    a = m(bags.detach())
    torch.manual_seed(0)
    b = m(bags.detach())
    assert torch.equal(a, b) and not torch.equal(a, m.eval()(bags.detach()))


def test_one_trainer_step_equals_module_and_torch_adamw(gpu):
    from stamp_amd.abmil import HipAbmilTrainer
    x, w = _case("small", DENSE, "random", seed=6)
    m = _module("small", w, gpu, dropout=0.0)
    bags = x.view(3, 33, 48).half().to(gpu)
    targets = torch.nn.functional.one_hot(torch.tensor([0, 2, 1]), 3).float().to(gpu)
    tr = HipAbmilTrainer(copy.deepcopy(m), device=gpu, max_lr=1e-3, total_steps=10, sched_interval="step", dropout=False)
    lr0, b1 = tr.clock.current()
    loss_t, logits_t = tr.step(bags, targets)
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=lr0, betas=(b1, 0.999), weight_decay=0.01)
    out = m(bags)
    loss_m = torch.nn.functional.cross_entropy(out, targets)
    loss_m.backward()
    assert torch.equal(out, logits_t) and torch.equal(loss_m.detach(), loss_t)
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, tr.g(k)), k          # the same two library calls
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt.step()
    # AdamW's first step moves every weight by lr (1 + O(eps / |g|)) sign(g) + lr wd w: the two implementations agree to fp32 rounding of that step
    for k, p in m.named_parameters():
        step_ref = (p.detach() - before[k]).abs().max().item()
        err = (p.detach() - tr.p(k)).abs().max().item()
        print(f"abmil trainer step {k}: step {step_ref:.3e} difference {err:.3e}")
        assert err <= 1e-5 * step_ref + 2 ** -23 * before[k].abs().max().item(), (k, err, step_ref)
    assert tr.step_count == 1 and not any(torch.equal(tr.p(k), before[k]) for k in before)


@pytest.fixture(scope="module")
def cohort_files(tmp_path_factory):
    from stamp_amd import h5io
    d = tmp_path_factory.mktemp("abmil_cohort")
    rng = np.random.default_rng(0)
    files = []
    for i, n in enumerate([5, 90, 32, 33, 61, 20, 47, 80, 12, 64, 31, 70]):
        feats = rng.standard_normal((n, 48)).astype(np.float32)
        feats[:, 0] += 1.5 if i % 2 else -1.5
        coords = np.stack([rng.integers(0, 40, n), rng.integers(0, 40, n)], 1).astype(np.float32) * 256.0
        p = d / f"p{i}.h5"
        h5io.write_tile_features(p, feats.astype(np.float16), coords, extractor="test", tile_size_um=256.0, tile_size_px=224, code_hash="0", stamp_version="2.4.0")
        files.append(p)
    return files


def _fit(gpu, cohort, dim_output, **kw):
    from stamp_amd.abmil import GatedAttentionMIL, HipAbmilTrainer
    from stamp_amd.mil_train import fit
    torch.manual_seed(3)
    tr = HipAbmilTrainer(GatedAttentionMIL(48, 64, 32, dim_output), device=gpu, max_lr=5e-3, total_steps=6, sched_interval="step", dropout=False)
    snaps = []
    feed = cohort.train_batches(batch_size=8, bag_size=32, out_dtype=torch.float16, generator=torch.Generator().manual_seed(1))
    hist = fit(tr, feed, cohort.valid_batches(), max_epochs=3, log=lambda msg: snaps.append(tr.P.clone()) if msg.startswith("epoch") else None, **kw)
    return tr, hist, snaps


def test_fit_on_a_resident_cohort_classification_regression_survival(gpu, cohort_files):
    from stamp_amd import bags as B
    from stamp_amd import losses
    from stamp_amd.cohort import ResidentCohort
    mk = lambda gts, task: ResidentCohort([B.PatientData(ground_truth=g, feature_files=[f]) for g, f in zip(gts, cohort_files)], task=task, device=gpu)  # noqa: E731
    cohort = mk(["pos" if i % 2 else "neg" for i in range(12)], "classification")
    assert cohort.dtype == torch.float16 and len(cohort) == 12
    tr, hist, snaps = _fit(gpu, cohort, 2, valid_bags_per_call=4)
    print("abmil fit classification: train", hist["train_loss"], "validation", hist["validation_loss"], "best", hist["best_epoch"])
    vl = hist["validation_loss"]
    assert len(vl) == 3 and all(np.isfinite(vl)) and hist["train_loss"][-1] < hist["train_loss"][0]
    assert hist["best_epoch"] == min(range(3), key=vl.__getitem__) and torch.equal(tr.P, snaps[hist["best_epoch"]]) and tr.step_count == 6
    rb = cohort.ragged_group(0, 12)
    with torch.no_grad():
        assert torch.equal(tr.model.to(gpu).eval().forward_infer_ragged(rb), tr.predict_infer_ragged(rb))
    # regression (L1) and survival (Cox, selection by the validation C-index) through the same loop
    tr, hist, _ = _fit(gpu, mk([1.0 if i % 2 else -1.0 for i in range(12)], "regression"), 1, loss_fn=losses.l1_loss)
    print("abmil fit regression: train", hist["train_loss"], "validation", hist["validation_loss"])
    assert all(np.isfinite(hist["train_loss"])) and all(np.isfinite(hist["validation_loss"])) and tr.step_count == 6
    tr, hist, _ = _fit(gpu, mk([(2.0 + (i % 2) * 5.0 + 0.1 * i, 1.0 if i % 3 else 0.0) for i in range(12)], "survival"), 1, loss_fn=losses.cox_survival_loss,
                       monitor="val_cindex")
    print("abmil fit survival: val_cindex", hist["val_cindex"], "median", hist["train_pred_median"])
    assert len(hist["val_cindex"]) == 3 and all(np.isfinite(hist["val_cindex"])) and np.isfinite(tr.train_pred_median)


def test_from_chief_reproduces_the_fixtures_logits(gpu):
    from stamp_amd import deploy
    from stamp_amd.abmil import GatedAttentionMIL
    fx = np.load(GOLD / "abmil_xs.npz")
    base = np.load(GOLD / "chief_gated_attention_xs.npz")
    sd = {k[2:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("w:")}
    sd.update({k[2:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("w:")})
    m = GatedAttentionMIL.from_chief("xs", sd, dim_output=2).to(gpu).eval()
    bags = [b.to(gpu) for b in torch.from_numpy(fx["x"]).split([int(n) for n in fx["lengths"]])]
    with torch.no_grad():
        lg = m.forward_ragged(bags)
        _, raw = m.attention(bags[0])
    np.testing.assert_allclose(lg.cpu().numpy(), fx["logits"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(raw.cpu().numpy(), fx["attention_raw"][:77], rtol=1e-5, atol=1e-6)
    preds = deploy.predict_(m, [(b[None], None, None, None) for b in bags], ["a", "b"], task="classification", device=gpu, bags_per_call=2)
    np.testing.assert_allclose(torch.stack([preds["a"], preds["b"]]).numpy(), torch.softmax(torch.from_numpy(fx["logits"]), 1).numpy(), rtol=1e-5, atol=1e-6)
