"""Dynamic loss scaling of fp16 MIL training: the kernels (amds_grad_unscale_check, amds_adamw_guarded, amds_loss_scale_update) through the
C ABI, HipMilVitTrainer skipping a step whose fp16 gradients overflow (and keeping the static scale's bits on finite runs), and the
drop-in module returning finite gradients / logits where fp16 overflows."""
import contextlib
import copy
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from oracle.mil_vit import mil_vit_forward, running_mean_update
from stamp_amd import mil_core
from stamp_amd import train_ops as T
from stamp_amd.mil import VisionTransformer
from stamp_amd.mil_train import HipMilVitTrainer

pytestmark = pytest.mark.gpu

DEFAULT_HEAD = dict(dim_output=2, dim_input=1024, dim_model=512, n_layers=2, n_heads=8, dim_feedforward=512)


@contextlib.contextmanager
def _precision(level):
    """torch.set_float32_matmul_precision for a block (the level the drop-in module reads), restored on exit."""
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(level)
    try:
        yield
    finally:
        torch.set_float32_matmul_precision(old)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _words(st):
    return st.cpu().tolist()


def _scale(st):
    return T.loss_scale_of(st).item()


def _flag(st, gpu):
    """Count one non-finite value into the state (what an overflowing backward does)."""
    T.grad_unscale_check(torch.tensor([1.0, float("nan"), 2.0], device=gpu), st)


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 257, 1023, 4096, 4099, (1 << 20) + 3, 3_700_001])
@pytest.mark.parametrize("offset", [0, 1])          # 1: a pointer that is not 16-byte aligned (the scalar path)
def test_unscale_check_counts_and_bits(gpu, n, offset):
    g = torch.Generator().manual_seed(n + offset)
    base = torch.randn(n + offset, generator=g) * 3e4
    x = base[offset:].clone()
    where = sorted({i for i in (0, n - 1, n - 1 - (n % 4) + 1, n // 2) if 0 <= i < n})   # first, last, first of the tail past the float4s, middle
    vals = [float("nan"), float("inf"), float("-inf")]
    for j, i in enumerate(where):
        x[i] = vals[j % 3]
    dev = torch.empty(n + offset, device=gpu)
    dev[offset:] = x.to(gpu)
    gd = dev[offset:]
    assert (gd.data_ptr() % 16 != 0) == bool(offset) or n == 0
    st = T.loss_scale_state(gpu, 1024.0)
    T.grad_unscale_check(gd, st)
    w = _words(st)
    assert w[T.LS_NONFINITE] == len(where), (w, where)
    ref = x.to(gpu) * torch.tensor(1.0 / 1024.0, device=gpu)
    fin = torch.isfinite(ref)
    assert torch.equal(gd[fin].view(torch.int32), ref[fin].view(torch.int32))
    assert torch.equal(torch.isnan(gd), torch.isnan(ref)) and torch.equal(torch.isposinf(gd), torch.isposinf(ref))
    assert torch.equal(torch.isneginf(gd), torch.isneginf(ref))
    # a second tensor of the same step adds to the count; a clean one adds nothing
    T.grad_unscale_check(torch.ones(1000, device=gpu), st)
    assert _words(st)[T.LS_NONFINITE] == len(where)


def _adam_inputs(n, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 1e-3
    v = torch.rand(n, generator=g) * 1e-5
    grad = torch.randn(n, generator=g) * 1e-2
    return [t.to(gpu) for t in (p, grad, m, v)]


def test_adamw_guarded_is_adamw_on_a_clean_step_and_a_noop_on_a_flagged_one(gpu):
    n = 100_003
    p, g, m, v = _adam_inputs(n, 1, gpu)
    st = T.loss_scale_state(gpu, 1024.0)
    for step in (1, 2, 7):
        a = [t.clone() for t in (p, m, v)]
        b = [t.clone() for t in (p, m, v)]
        T.adamw(a[0], g, a[1], a[2], 3e-4, step, betas=(0.93, 0.999), weight_decay=0.01)
        T.adamw_guarded(b[0], g, b[1], b[2], 3e-4, step, st, betas=(0.93, 0.999), weight_decay=0.01)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), step
    _flag(st, gpu)
    b = [t.clone() for t in (p, m, v)]
    T.adamw_guarded(b[0], g, b[1], b[2], 3e-4, 3, st, betas=(0.93, 0.999), weight_decay=0.01)
    assert all(torch.equal(x, y) for x, y in zip((p, m, v), b))


def test_adamw_guarded_after_skips_counts_applied_steps_like_torch(gpu):
    """A run with skipped steps against an fp64 restatement of torch.optim.AdamW that only sees the applied steps (t = applied steps): the parameters
    within 1e-6.  The moments are held to the same restatement at the fp32 values of the hyper-parameters the kernel is handed (amds_adamw's own
    arithmetic: 1 - 0.999f is 0.00099998713, which alone moves v by 1.3e-5 from the fp64 value)."""
    n = 50_000
    p, _, m, v = _adam_inputs(n, 2, gpu)
    m.zero_(); v.zero_()
    pd, md, vd = p.cpu().double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    md32, vd32 = md.clone(), vd.clone()
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))       # noqa: E731
    st = T.loss_scale_state(gpu, 1024.0, growth_interval=1000)
    gen = torch.Generator().manual_seed(3)
    lr, wd, b2, eps = 2e-3, 0.01, 0.999, 1e-8
    t = 0
    pattern = [0, 1, 0, 1, 1, 0, 0, 1, 0, 0]
    for i, bad in enumerate(pattern):
        scale = _scale(st)
        grad = torch.randn(n, generator=gen) * 1e-2
        gs = (grad * scale).to(gpu)
        if bad:
            gs[17] = float("inf")
        b1 = 0.95 - 0.01 * i
        T.grad_unscale_check(gs, st)
        T.adamw_guarded(p, gs, m, v, lr, i + 1, st, betas=(b1, b2), weight_decay=wd)
        T.loss_scale_update(st, apply=True)
        if not bad:
            t += 1
            gd = grad.double()
            pd = pd * (1 - lr * wd)
            md = b1 * md + (1 - b1) * gd
            vd = b2 * vd + (1 - b2) * gd * gd
            pd = pd - (lr / (1 - b1 ** t)) * md / ((vd.sqrt() / (1 - b2 ** t) ** 0.5) + eps)
            md32 = f32(b1) * md32 + (1 - f32(b1)) * gd
            vd32 = f32(b2) * vd32 + (1 - f32(b2)) * gd * gd
    assert _words(st)[T.LS_SKIPPED] == sum(pattern)
    assert _rel(p.cpu(), pd) < 1e-6, _rel(p.cpu(), pd)
    assert _rel(m.cpu(), md32) < 1e-6 and _rel(v.cpu(), vd32) < 1e-6, (_rel(m.cpu(), md32), _rel(v.cpu(), vd32))


def test_scale_backoff_floor_growth_and_cap(gpu):
    st = T.loss_scale_state(gpu, 1024.0, growth_interval=3, min_scale=256.0)
    seq = []

    def step(bad):
        if bad:
            _flag(st, gpu)
        T.loss_scale_update(st, apply=True)
        w = _words(st)
        assert w[T.LS_NONFINITE] == 0 and w[T.LS_LAST_NONFINITE] == int(bad)
        assert T.loss_scale_of(st).item() * st.view(torch.float32)[T.LS_INV_SCALE].item() == 1.0
        seq.append(_scale(st))

    for bad in (1, 1, 1):                 # back-off, back-off, floor
        step(bad)
    assert seq == [512.0, 256.0, 256.0] and _words(st)[T.LS_SKIPPED] == 3
    for _ in range(2):
        step(0)
    assert seq[-1] == 256.0 and _words(st)[T.LS_CLEAN_STEPS] == 2
    step(0)                               # the third clean step: growth
    assert seq[-1] == 512.0 and _words(st)[T.LS_CLEAN_STEPS] == 0
    step(0); step(1)                      # an overflow resets the clean-step count
    assert seq[-1] == 256.0 and _words(st)[T.LS_CLEAN_STEPS] == 0
    for _ in range(6):
        step(0)
    assert seq[-1] == 1024.0
    for _ in range(3):
        step(0)
    assert seq[-1] == 1024.0              # capped at the initial scale
    # apply=False (a step without update): the count is recorded and reset, the scale and the counters stay
    _flag(st, gpu)
    before = _words(st)
    T.loss_scale_update(st, apply=False)
    after = _words(st)
    assert after[T.LS_NONFINITE] == 0 and after[T.LS_LAST_NONFINITE] == 1 and _scale(st) == 1024.0
    assert after[T.LS_SKIPPED] == before[T.LS_SKIPPED] and after[T.LS_CLEAN_STEPS] == before[T.LS_CLEAN_STEPS]
    # n = 0 launches nothing and counts nothing
    T.grad_unscale_check(torch.empty(0, device=gpu), st)
    assert _words(st)[T.LS_NONFINITE] == 0


# ---- HipMilVitTrainer ------------------------------------------------------------------------------------------------------------------------------
def _batch(seed, Bb=4, Tn=256, Fd=1024):
    g = torch.Generator().manual_seed(seed)
    bags = torch.randn(Bb, Tn, Fd, generator=g).half()
    coords = (torch.rand(Bb, Tn, 2, generator=g) * 4e4 / 256).round() * 256
    targets = F.one_hot(torch.arange(Bb) % 2, 2).float()
    return bags, coords, targets


def _trainers(alibi, **kw):
    torch.manual_seed(31)
    model = VisionTransformer(**DEFAULT_HEAD, dropout=0.25, use_alibi=alibi)
    twin = copy.deepcopy(model)
    return model, twin


@pytest.mark.parametrize("alibi", [False, True])
def test_trainer_skips_an_overflowing_step_and_backs_off(gpu, alibi):
    m1, m2 = _trainers(alibi)
    tr = HipMilVitTrainer(m1, device=gpu, precision="high")
    twin = HipMilVitTrainer(m2, device=gpu, precision="high")
    assert tr.act == torch.float16 and tr.current_loss_scale == 1024.0 and tr.skipped_steps == 0

    def run(t, seed, loss_fn=None, update=True):
        bags, coords, targets = _batch(seed)
        return t.step(bags.to(gpu), targets, coords=coords.to(gpu), seed=seed, loss_fn=loss_fn, update=update)

    run(tr, 1); run(twin, 1)
    assert torch.equal(tr.P, twin.P)
    P0, m0, v0 = tr.P.clone(), tr.m.clone(), tr.v.clone()
    huge = lambda lg, t: F.cross_entropy(lg, t) * 1e8          # noqa: E731  -- dlogits * 2^10 leaves fp16's range in the backward
    # update=False: checked, but neither a step nor a scale decision
    run(tr, 2, huge, update=False)
    assert torch.equal(tr.P, P0) and tr.skipped_steps == 0 and tr.current_loss_scale == 1024.0
    loss, logits = run(tr, 2, huge)
    assert torch.isfinite(loss) and torch.isfinite(logits).all()
    assert not torch.isfinite(tr.G).all()                     # the gradients did overflow
    keep = torch.ones_like(tr.P, dtype=torch.bool)
    keep[tr._stat_idx] = False
    assert torch.equal(tr.P[keep], P0[keep]) and torch.equal(tr.m, m0) and torch.equal(tr.v, v0)
    assert tr.skipped_steps == 1 and tr.current_loss_scale == 512.0
    if alibi:       # the skipped step's forward updated the running means, as the reference module's would: the twin gets the same update
        bags, coords, _ = _batch(2)
        assert not torch.equal(tr.P[tr._stat_idx], P0[tr._stat_idx])
        mil_core.update_running_means(twin.p, twin.dims, mil_core._coords_with_cls(coords.to(gpu), bags.shape[0], gpu))
        twin._refresh()
        assert torch.equal(tr.P, twin.P)
    run(tr, 3); run(twin, 3)
    assert torch.isfinite(tr.P).all() and tr.skipped_steps == 1
    # (the updates themselves agree to ~2e-3: the two scales round the smallest fp16 gradients differently, and Adam's update is as large for them)
    assert _rel(tr.P, twin.P) < 1e-5 and _rel(tr.P - P0, twin.P - P0) < 1e-2, (_rel(tr.P, twin.P), _rel(tr.P - P0, twin.P - P0))


@pytest.mark.parametrize("alibi", [False, True])
def test_finite_runs_keep_the_static_scales_bits(gpu, alibi):
    m1, m2 = _trainers(alibi)
    dyn = HipMilVitTrainer(m1, device=gpu, precision="high", max_lr=1e-3, total_steps=10, sched_interval="step")
    sta = HipMilVitTrainer(m2, device=gpu, precision="high", max_lr=1e-3, total_steps=10, sched_interval="step", dynamic_loss_scale=False)
    assert dyn._ls is not None and sta._ls is None
    for s in range(5):
        bags, coords, targets = _batch(10 + s)
        l1, _ = dyn.step(bags.to(gpu), targets, coords=coords.to(gpu), seed=100 + s)
        l2, _ = sta.step(bags.to(gpu), targets, coords=coords.to(gpu), seed=100 + s)
        assert torch.equal(l1, l2), s
    assert torch.equal(dyn.P, sta.P) and torch.equal(dyn.m, sta.m) and torch.equal(dyn.v, sta.v)
    assert dyn.skipped_steps == 0 and dyn.current_loss_scale == 1024.0


def test_bf16_training_has_no_loss_scale(gpu):
    torch.manual_seed(2)
    tr = HipMilVitTrainer(VisionTransformer(**DEFAULT_HEAD, dropout=0.0, use_alibi=False), device=gpu, precision="medium")
    assert tr._ls is None and tr.current_loss_scale == 1.0 and tr.skipped_steps == 0


# ---- drop-in module under a torch optimiser -----------------------------------------------------------------------------------------------------
def _perturb(model, scale=0.05):
    """Move the 1-d parameters off their initial values (LayerNorm 1 / 0 makes some bias gradients tiny sums of cancelling terms)."""
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1 and "class_token" not in n and "bias_scale" not in n:
                p.add_(scale * torch.randn_like(p))


def _no_dropout(model):
    model.dims = dataclasses.replace(model.dims, p_drop=0.0, p_ff=0.0)
    return model


def _oracle(model, bags, coords, alibi, Bb):
    """fp64 autograd of the same network (train-mode semantics: the ALiBi scalers updated before use)."""
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    sd = dict(sd0)
    if alibi:
        cc = torch.cat([coords.new_zeros(Bb, 1, 2), coords], dim=1)
        dist = torch.cdist(cc, cc)
        for k in sd0:
            if k.endswith("running_mean"):
                n = k[: -len("running_mean")] + "items_so_far"
                sd[k], sd[n] = running_mean_update(sd0[k], sd0[n], dist)
    params = {k: v.clone().double().requires_grad_(not mil_core.is_buffer(k)) for k, v in sd.items()}
    x = bags.double().requires_grad_(True)
    return params, x, mil_vit_forward(x, coords.double(), None, params, n_heads=DEFAULT_HEAD["n_heads"], use_alibi=alibi, dtype=torch.float64)


def _grad_error(model, params, x, bags_grad):
    """-> the largest relative-L2 error of any parameter gradient and of d/d(bags) against fp64 autograd (all of them finite)."""
    named = dict(model.named_parameters())
    worst, bsg = [], {}
    for k, p in named.items():
        if "key_encoders" in k and k.endswith(".bias"):
            continue                      # (zero true gradient)
        g, r = p.grad.cpu().double(), params[k].grad.double()
        if k.endswith("in_proj_bias"):
            D = DEFAULT_HEAD["dim_model"]
            g, r = torch.cat([g[:D], g[2 * D:]]), torch.cat([r[:D], r[2 * D:]])
        floor = 0.0
        if "query_encoders" in k or "key_encoders" in k:
            floor = 0.05 * params[k.replace("query_encoders", "value_encoders").replace("key_encoders", "value_encoders")].grad.double().norm().item()
        assert torch.isfinite(p.grad).all(), k
        if k.endswith("bias_scale"):      # one scalar per head, each a signed sum over all rows: judged as one vector per layer
            a, b = bsg.setdefault(k.split(".mhsa.")[0], ([], []))
            a.append(g), b.append(r)
            continue
        worst.append((((g - r).norm() / max(r.norm().item(), floor, 1e-30)).item(), k))
    for layer, (a, b) in bsg.items():
        worst.append((_rel(torch.cat(a), torch.cat(b)), layer + ".mhsa.attentions.*.bias_scale"))
    assert torch.isfinite(bags_grad).all()
    worst.append((_rel(bags_grad.cpu(), x.grad), "bags"))
    worst.sort(reverse=True)
    print("largest relative-L2 gradient errors", [(round(a, 5), b) for a, b in worst[:5]])
    return worst[0][0]


@pytest.mark.parametrize("alibi", [False, True])
def test_drop_in_backward_overflow_returns_finite_gradients(gpu, alibi):
    """A loss 1e8 x too large: the fp16 backward overflows at every scale tried, and the step falls back to bf16 operands.  Its gradients are held
    to bf16-class accuracy: within 1e-2 relative L2 of fp64 autograd, or -- where bf16 operands themselves do not get there (the plain head's
    last feed-forward block at this geometry: 3.9e-2, measured on the MI355X) -- no worse than 1.25 x the error of a "medium" (bf16) run
    of the same network."""
    torch.manual_seed(41)
    Bb, Tn = 4, 1024
    model = _no_dropout(VisionTransformer(**DEFAULT_HEAD, dropout=0.0, use_alibi=alibi))
    _perturb(model)
    bags, coords, targets = _batch(5, Bb=Bb, Tn=Tn)
    bags = bags.float()
    params, x, ref = _oracle(model, bags, coords, alibi, Bb)
    (F.cross_entropy(ref, targets.double()) * 1e8).backward()
    bf = copy.deepcopy(model).to(gpu).train()
    bgb = bags.to(gpu).requires_grad_(True)
    with _precision("medium"):
        (F.cross_entropy(bf(bgb, coords=coords.to(gpu), mask=None), targets.to(gpu)) * 1e8).backward()
    bf16_err = _grad_error(bf, params, x, bgb.grad)
    model = model.to(gpu).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    bg = bags.to(gpu).requires_grad_(True)
    with _precision("high"):
        logits = model(bg, coords=coords.to(gpu), mask=None)
        (F.cross_entropy(logits, targets.to(gpu)) * 1e8).backward()
    assert model.fp16_overflow_events > 0
    err = _grad_error(model, params, x, bg.grad)
    assert err < max(1e-2, 1.25 * bf16_err), (err, bf16_err)
    opt.step()
    assert all(torch.isfinite(p).all() for p in model.parameters())
    # a loss of ordinary size takes no remedy: the counter stays
    n = model.fp16_overflow_events
    opt.zero_grad()
    with _precision("high"):
        F.cross_entropy(model(bags.to(gpu), coords=coords.to(gpu), mask=None), targets.to(gpu)).backward()
    assert model.fp16_overflow_events == n


@pytest.mark.parametrize("alibi", [False, True])
def test_drop_in_forward_overflow_falls_back_to_bf16(gpu, alibi):
    torch.manual_seed(43)
    Bb, Tn = 2, 256
    model = _no_dropout(VisionTransformer(**DEFAULT_HEAD, dropout=0.0, use_alibi=alibi))
    _perturb(model)
    bags, coords, targets = _batch(6, Bb=Bb, Tn=Tn)
    bags = bags.float() * 1e5                     # beyond fp16's 65504: the fp16 operands of the first product overflow
    params, x, ref = _oracle(model, bags, coords, alibi, Bb)
    F.cross_entropy(ref, targets.double()).backward()
    model = model.to(gpu).train()
    bg = bags.to(gpu).requires_grad_(True)
    with _precision("high"):
        logits = model(bg, coords=coords.to(gpu), mask=None)
        assert model.fp16_overflow_events == 1
        assert torch.isfinite(logits).all()
        assert (logits.detach().cpu().double() - ref.detach()).abs().max() < 3e-2 * max(1.0, ref.abs().max().item())
        F.cross_entropy(logits, targets.to(gpu)).backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters()) and torch.isfinite(bg.grad).all()


def test_drop_in_jacrev_goes_through_the_guarded_backward(gpu):
    from torch.func import jacrev
    torch.manual_seed(44)
    model = VisionTransformer(**DEFAULT_HEAD, dropout=0.0, use_alibi=False).to(gpu).eval()
    feats = torch.randn(64, DEFAULT_HEAD["dim_input"], device=gpu)
    with _precision("high"):
        jac = jacrev(lambda b: model(b.unsqueeze(0), coords=None, mask=None).squeeze(0))(feats)
    with _precision("medium"):
        jac16 = jacrev(lambda b: model(b.unsqueeze(0), coords=None, mask=None).squeeze(0))(feats)
    assert jac.shape == (2, 64, DEFAULT_HEAD["dim_input"]) and torch.isfinite(jac).all()
    assert _rel(jac, jac16) < 3e-2 and model.fp16_overflow_events == 0
