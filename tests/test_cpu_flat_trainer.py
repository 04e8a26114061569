"""`flat_trainer.FlatTrainer`, no GPU: a toy head whose forward and backward are written in torch drives the shared constructor and the `step` template
(AdamW under OneCycle against torch's own, `update=False`, a loss without a gradient, the seed draw, `_refresh`, `order`), and the three trainers that can be
built on the CPU are subclasses with the flat layout `test_cpu_transmil_trainer.py` asserts for TransMIL."""
import pytest
import torch

from stamp_amd import train_ops
from stamp_amd.abmil import CHIEF_SIZES, GatedAttentionMIL, HipAbmilTrainer
from stamp_amd.flat_trainer import FlatTrainer, flat_layout
from stamp_amd.mil import MLP, TransMIL
from stamp_amd.mlp_train import HipMlpTrainer
from stamp_amd.transmil_train import HipTransMilTrainer

WD = 0.05


class _Toy(FlatTrainer):
    """logits = bags @ W^T + b over the views of P; the gradients go into the views of G."""

    def __init__(self, model, *, live=False, order=None, sched_interval="epoch", total_steps=10):
        super().__init__(model, "cpu", max_lr=1e-2, div_factor=25.0, total_steps=total_steps, weight_decay=WD, sched_interval=sched_interval, order=order)
        self.live = live
        self.calls = []

    @property
    def dropout_live(self):
        return self.live

    def _forward_train(self, bags, coords, seed):
        self.calls.append(("forward", seed))
        return bags @ self.p("weight").t() + self.p("bias"), bags

    def _backward(self, saved, dlogits):
        self.calls.append(("backward",))
        self.g("weight").copy_(dlogits.t() @ saved)
        self.g("bias").copy_(dlogits.sum(0))

    def _refresh(self):
        self.calls.append(("refresh",))


def _adamw_in_torch(record):
    """`train_ops.adamw` restated in torch (torch.optim.AdamW's single-tensor update), recording its arguments."""

    def adamw(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
        record.append(dict(p=p, g=g, m=m, v=v, lr=lr, step=step, betas=betas, weight_decay=weight_decay))
        p.mul_(1.0 - lr * weight_decay)
        m.lerp_(g, 1.0 - betas[0])
        v.mul_(betas[1]).addcmul_(g, g, value=1.0 - betas[1])
        denom = (v.sqrt() / (1.0 - betas[1] ** step) ** 0.5).add_(eps)
        p.addcdiv_(m, denom, value=-lr / (1.0 - betas[0] ** step))

    return adamw


def _data(seed=0, n=5):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=gen), torch.eye(2)[torch.randint(0, 2, (n,), generator=gen)]


def _linear():
    torch.manual_seed(0)
    return torch.nn.Linear(3, 2)


@pytest.mark.parametrize("interval", ["epoch", "step"])
def test_steps_equal_torch_adamw_under_onecycle(monkeypatch, interval):
    """3 steps with an `epoch_end` after the second.  Bar: both sides are fp32 with values below 1 and updates of about lr <= 1e-2 a step; a handful of
    roundings of 2^-24 relative per step and element stay far below 1e-6, while a wrong lr, beta1, step count or weight decay moves P by 1e-5 and more."""
    record = []
    monkeypatch.setattr(train_ops, "adamw", _adamw_in_torch(record))
    model = _linear()
    ref = torch.nn.Linear(3, 2)
    ref.load_state_dict(model.state_dict())
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=WD)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, total_steps=10, max_lr=1e-2, div_factor=25.0)
    tr = _Toy(model, sched_interval=interval)
    weights = torch.tensor([0.7, 1.3])
    start = tr.P.clone()
    for i in range(3):
        bags, targets = _data(i)
        loss, logits = tr.step(bags, targets, weights)
        opt.zero_grad()
        ref_logits = ref(bags)
        ref_loss = torch.nn.functional.cross_entropy(ref_logits, targets, weight=weights)
        assert torch.allclose(logits, ref_logits.detach(), rtol=0, atol=1e-6) and abs(float(loss) - float(ref_loss.detach())) < 1e-6
        assert not loss.requires_grad
        ref_loss.backward()
        opt.step()
        if interval == "step":
            sched.step()
        if i == 1:
            tr.epoch_end()
            if interval == "epoch":
                sched.step()
        want = torch.cat([ref.state_dict()[k].reshape(-1) for k in tr.names])
        assert torch.allclose(tr.P, want, rtol=0, atol=1e-6), (i, (tr.P - want).abs().max())
    assert (tr.P - start).abs().min() > 1e-4                # (every element moved by far more than the bar)
    assert tr.step_count == 3 and [r["step"] for r in record] == [1, 2, 3] and tr.clock.pos == (3 if interval == "step" else 1)
    assert all(r["p"] is tr.P and r["g"] is tr.G and r["m"] is tr.m and r["v"] is tr.v and r["weight_decay"] == WD for r in record)
    at = [0, 1, 2] if interval == "step" else [0, 0, 1]
    assert [(r["lr"], r["betas"]) for r in record] == [(tr.clock.lrs[i], (tr.clock.b1s[i], 0.999)) for i in at]
    tr.sync_to_model()
    for k, t in model.state_dict().items():
        assert torch.equal(t, tr.p(k)) and t.data_ptr() != tr.p(k).data_ptr()


def test_update_false_fills_G_and_leaves_the_state(monkeypatch):
    record = []
    monkeypatch.setattr(train_ops, "adamw", _adamw_in_torch(record))
    tr = _Toy(_linear(), sched_interval="step")
    tr.step(*_data(0))                                      # (so that m, v, step_count and the clock are not at their initial values)
    before = [t.clone() for t in (tr.P, tr.m, tr.v)]
    tr.G.zero_()
    bags, targets = _data(1)
    loss, logits = tr.step(bags, targets, update=False)
    lg = (bags @ tr.p("weight").t() + tr.p("bias")).requires_grad_(True)
    want = torch.autograd.grad(torch.nn.functional.cross_entropy(lg, targets), lg)[0]
    assert torch.allclose(tr.g("weight"), want.t() @ bags, rtol=0, atol=1e-6) and torch.allclose(tr.g("bias"), want.sum(0), rtol=0, atol=1e-6)
    assert tr.G.abs().max() > 1e-3
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.P, tr.m, tr.v))) and tr.step_count == 1 and tr.clock.pos == 1 and len(record) == 1


@pytest.mark.parametrize("update", [True, False])
def test_a_loss_without_gradient_takes_no_step(monkeypatch, update):
    record = []
    monkeypatch.setattr(train_ops, "adamw", _adamw_in_torch(record))
    tr = _Toy(_linear(), sched_interval="step")
    tr.G.fill_(3.0)
    before = tr.P.clone()
    bags, targets = _data(0)
    loss, logits = tr.step(bags, targets, update=update, loss_fn=lambda lg, t: torch.zeros(()))
    assert float(loss) == 0.0 and logits.shape == (5, 2)
    assert [c[0] for c in tr.calls] == ["forward"] and record == []
    assert torch.equal(tr.G, torch.full_like(tr.G, 3.0)) and torch.equal(tr.P, before) and tr.step_count == 0 and tr.clock.pos == 0


def test_the_seed_is_drawn_only_when_dropout_is_live_and_none_is_given(monkeypatch):
    monkeypatch.setattr(train_ops, "adamw", _adamw_in_torch([]))
    bags, targets = _data(0)
    for live, seed, drawn in ((True, None, True), (False, None, False), (True, 1234567, False), (False, 77, False)):
        tr = _Toy(_linear(), live=live)
        torch.manual_seed(11)
        state = torch.get_rng_state()
        tr.step(bags, targets, seed=seed)
        assert torch.equal(torch.get_rng_state(), state) != drawn, (live, seed)
        torch.manual_seed(11)
        want = int(torch.randint(0, 2 ** 62, (1,)).item()) if drawn else (0 if seed is None else seed)
        assert tr.calls[0] == ("forward", want), (live, seed)


def test_load_from_model_calls_refresh():
    tr = _Toy(_linear())
    with torch.no_grad():
        tr.model.weight.add_(1.0)
    assert tr.calls == []
    tr.load_from_model()
    assert tr.calls == [("refresh",)] and torch.equal(tr.p("weight"), tr.model.weight)


def test_order_places_the_tensors_and_names_stay_the_state_dicts():
    model = _linear()
    tr = _Toy(model, order=["bias", "weight"])
    assert tr.names == ["weight", "bias"] and list(tr.offs) == ["bias", "weight"] and tr.offs == {"bias": (0, 2), "weight": (2, 6)}
    assert torch.equal(tr.P, torch.cat([model.bias.detach().reshape(-1), model.weight.detach().reshape(-1)]))
    assert torch.equal(tr.p("weight"), model.weight) and tr.p("weight").data_ptr() == tr.P.data_ptr() + 8
    tr.P.copy_(torch.arange(8.0))
    tr.sync_to_model()
    assert list(model.state_dict()) == ["weight", "bias"]
    assert torch.equal(model.bias, torch.arange(2.0)) and torch.equal(model.weight, torch.arange(2.0, 8.0).view(2, 3))
    tr.P.zero_()
    tr.load_from_model()
    assert torch.equal(tr.P, torch.arange(8.0))


def _transmil():
    return HipTransMilTrainer(TransMIL(dim_output=3, dim_input=24, dim_hidden=64), device="cpu")


def _abmil():
    return HipAbmilTrainer(GatedAttentionMIL(*CHIEF_SIZES["xs"], 2), device="cpu")


def _mlp():
    return HipMlpTrainer(MLP(24, 16, 3, 2, 0.25), device="cpu")


@pytest.mark.parametrize("build,aligned", [(_transmil, True), (_abmil, False), (_mlp, False)], ids=["transmil", "abmil", "mlp"])
def test_subclasses_lay_the_state_dict_out_flat_once_in_its_order(build, aligned):
    torch.manual_seed(0)
    tr = build()
    assert isinstance(tr, FlatTrainer)
    sd = tr.model.state_dict()
    assert tr.names == list(sd) and list(tr.offs) == tr.names
    at = 0
    for k in tr.names:                                     # back to back, in the state_dict's order: no gap, no overlap
        assert tr.offs[k] == (at, sd[k].numel()), k
        at += sd[k].numel()
    assert at == tr.P.numel() == tr.G.numel() == tr.m.numel() == tr.v.numel() == sum(v.numel() for v in sd.values())
    assert flat_layout({k: tuple(v.shape) for k, v in sd.items()}) == (tr.offs, at)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (tr.P, tr.G, tr.m, tr.v))
    for k in tr.names:                                     # views: same storage, the offset's address, the module's shape and values
        o = tr.offs[k][0]
        for view, flat in ((tr.p(k), tr.P), (tr.g(k), tr.G)):
            assert view.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and view.data_ptr() == flat.data_ptr() + 4 * o
            assert view.shape == sd[k].shape and view.is_contiguous() and (not aligned or (4 * o) % 16 == 0)
        assert torch.equal(tr.p(k), sd[k])
    first, last = tr.names[0], tr.names[-1]
    tr.p(first).view(-1)[1] = 7.0
    tr.g(last).view(-1)[-1] = -2.0
    assert tr.P[tr.offs[first][0] + 1] == 7.0 and tr.G[-1] == -2.0
    assert tr.skipped_steps == 0 and tr.current_loss_scale == 1.0 and tr.step_count == 0 and tr.train_pred_median is None
