"""Host logic of barspoon training on CPU (no kernels run): the pad / un-pad round trip of the decoder's K | V projection and of the gradient slicing,
the `forward_train` / trainer plumbing with the two library calls replaced by a linear stand-in, and the dropout-rate check."""
import pytest
import torch
from torch import nn

from stamp_amd import barspoon as bs
from stamp_amd.barspoon import EncDecTransformer
from stamp_amd.barspoon_train import HipBarspoonTrainer, multi_target_loss
from stamp_amd.mil_core import PackedVit, VitDims

TARGETS = {"A": 2, "B-1": 5, "C": 3}
KW = dict(d_model=128, num_encoder_heads=4, num_decoder_heads=2, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=192)


def test_kv_projection_padding_round_trips():
    g = torch.Generator().manual_seed(0)
    for D, Hd in ((128, 2), (256, 4), (132, 3), (64, 1), (512, 8)):
        hd, Dp, Db = D // Hd, bs._up(D, 256), 64 * Hd
        KVp = bs._up(2 * Db, 256)
        w, b = torch.randn(2 * D, D, generator=g), torch.randn(2 * D, generator=g)
        wp, bp = bs.pad_kv_w(w, Hd, D, Dp), bs.pad_kv_b(b, Hd, D)
        assert wp.shape == (2 * Db, Dp) and bp.shape == (2 * Db,)
        # K head h at rows 64 h .., V head h at Db + 64 h ..; channels >= hd, columns >= D are zero
        assert torch.equal(wp[64:64 + hd, :D], w[hd:2 * hd]) if Hd > 1 else True
        assert torch.equal(wp[Db:Db + hd, :D], w[D:D + hd]) and torch.equal(bp[Db:Db + hd], b[D:D + hd])
        assert wp.count_nonzero() == w.count_nonzero() and bp.count_nonzero() == b.count_nonzero()           # nothing lost, nothing but zeros added
        if hd < 64:
            assert not wp[hd:64].any() and not bp[hd:64].any()
        assert not wp[:, D:].any()
        # the gradient buffers are [KVp][Dp] / [KVp]: rows >= 2 Db and the padding are sliced off
        gw = torch.zeros(KVp, Dp)
        gw[:2 * Db] = wp
        gb = torch.zeros(KVp)
        gb[:2 * Db] = bp
        assert torch.equal(bs.unpad_kv_w(gw, Hd, D), w) and torch.equal(bs.unpad_kv_b(gb, Hd, D), b)


def _host_pack(model, dev="cpu"):
    """A TrainPack's host-side fields without touching the library (no operand copies, no C structs)."""
    pack = bs.TrainPack.__new__(bs.TrainPack)
    pack.model = model
    pack.dims = VitDims(F=model.d_features, D=model.d_model, H=model.num_encoder_heads, FF=model.dim_feedforward, C=1, L=model.num_encoder_layers, alibi=False)
    pack.pk = PackedVit.__new__(PackedVit)
    pack.pk.dims = pack.dims
    pack.KVp = bs._up(2 * 64 * model.num_decoder_heads, 256)
    pack.no = list(model.target_n_outs.values())
    pack.total_out = sum(pack.no)
    return pack


@pytest.mark.parametrize("kw", [KW, dict(d_model=256, num_encoder_heads=4, num_decoder_heads=4, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=256)])
def test_gradient_slicing_inverts_the_weight_padding(kw):
    """Padded buffers filled with the PADDED WEIGHTS themselves must un-pad to the parameters (q rows of padded encoder heads: scaled on the way in and on the
    way out, as PackedVit.unpad_in_w)."""
    torch.manual_seed(1)
    model = EncDecTransformer(200, TARGETS, **kw)
    pack = _host_pack(model)
    d, pk = pack.dims, pack.pk
    P = {k: v.detach() for k, v in model.named_parameters()}
    D, Hd = model.d_model, model.num_decoder_heads
    layout = dict(bs.grad_layout(pack))
    B = {k: torch.full(sh, float("nan")) for k, sh in layout.items()}

    def put(key, t):
        assert tuple(t.shape) == layout[key], (key, t.shape, layout[key])
        B[key] = t

    pad2 = lambda w, R, Cc: nn.functional.pad(w, (0, Cc - w.shape[1], 0, R - w.shape[0]))  # noqa: E731
    pad1 = lambda v, n: nn.functional.pad(v, (0, n - v.numel()))  # noqa: E731
    put("proj_w", pad2(P["projector.0.weight"], d.Dp, d.Fp))
    put("proj_b", pad1(P["projector.0.bias"], d.Dp))
    put("class_tokens", torch.stack([P[f"class_tokens.{bs.sanitize(t)}"] for t in TARGETS]))
    for l in range(d.L):
        p, e = f"transformer_encoder.layers.{l}.", f"enc{l}."
        put(e + "in_w", pk._pad_in(P[p + "self_attn.in_proj_weight"].view(3, d.H, d.hd, d.D)))
        put(e + "in_b", pk._pad_in(P[p + "self_attn.in_proj_bias"].view(3, d.H, d.hd)))
        put(e + "out_w", pk._pad_out(P[p + "self_attn.out_proj.weight"]))
        put(e + "out_b", pad1(P[p + "self_attn.out_proj.bias"], d.Dp))
        put(e + "fc1_w", pad2(P[p + "linear1.weight"], d.FFp, d.Dp)); put(e + "fc1_b", pad1(P[p + "linear1.bias"], d.FFp))
        put(e + "fc2_w", pad2(P[p + "linear2.weight"], d.Dp, d.FFp)); put(e + "fc2_b", pad1(P[p + "linear2.bias"], d.Dp))
        for a, b in (("ln1", "norm1"), ("ln2", "norm2")):
            put(e + a + "_w", P[p + b + ".weight"]); put(e + a + "_b", P[p + b + ".bias"])
    for l in range(model.num_decoder_layers):
        p, e = f"transformer_decoder.layers.{l}.", f"dec{l}."
        for k, n in bs._DEC_FP32:
            put(e + k, P[p + n])
        w, b = P[p + "multihead_attn.in_proj_weight"], P[p + "multihead_attn.in_proj_bias"]
        put(e + "ca_q_w", w[:D]); put(e + "ca_q_b", b[:D])
        put(e + "ca_kv_w", pad2(bs.pad_kv_w(w[D:], Hd, D, d.Dp), pack.KVp, d.Dp)); put(e + "ca_kv_b", pad1(bs.pad_kv_b(b[D:], Hd, D), pack.KVp))
    for j, t in enumerate(TARGETS):
        put(f"head{j}.w", P[f"heads.{bs.sanitize(t)}.weight"]); put(f"head{j}.b", P[f"heads.{bs.sanitize(t)}.bias"])
    G = bs.unpad_grads(pack, B)
    assert sorted(G) == sorted(P)
    q2 = d.qscale ** 2 if d.hd != 64 else 1.0
    for k, v in P.items():
        want = v.clone()
        if k.startswith("transformer_encoder") and "self_attn.in_proj" in k:
            want[: d.D] *= q2
        assert G[k].shape == v.shape and torch.allclose(G[k], want), k


def _patch_library(monkeypatch):
    """Stand-ins for the pack and the two library calls: logits_t = mean over tiles of the bag's first d_model features + class token t, through head t.
    Only the plumbing around them is under test."""
    calls = {"fwd": 0, "bwd": 0, "seeds": [], "p": []}

    class Pack:
        def __init__(self, model, get, act, dev):
            self.model, self.get, self.act = model, get, act
            self.no = list(model.target_n_outs.values())
            self.total_out = sum(self.no)

    def fwd(pack, x, pos, *, p, seed):
        calls["fwd"] += 1
        calls["seeds"].append(seed)
        calls["p"].append(p)
        m = pack.model
        pooled = x.float().mean(1)[:, : m.d_model]
        feats = [pooled + pack.get(f"class_tokens.{bs.sanitize(t)}") for t in m.target_labels]
        logits = torch.cat([f @ pack.get(f"heads.{bs.sanitize(t)}.weight").t() + pack.get(f"heads.{bs.sanitize(t)}.bias") for f, t in zip(feats, m.target_labels)], dim=1)
        return logits, dict(feats=feats, shape=tuple(x.shape))

    def bwd(pack, saved, dlogits, *, split_k=32, unscale=1.0):
        calls["bwd"] += 1
        dlogits = dlogits / unscale
        m = pack.model
        G = {n: torch.zeros_like(q) for n, q in m.named_parameters()}
        col = 0
        for f, t, n in zip(saved["feats"], m.target_labels, pack.no):
            s, dl = bs.sanitize(t), dlogits[:, col:col + n]
            G[f"heads.{s}.weight"], G[f"heads.{s}.bias"] = dl.t() @ f, dl.sum(0)
            G[f"class_tokens.{s}"] = (dl @ pack.get(f"heads.{s}.weight")).sum(0)
            col += n
        return G

    monkeypatch.setattr(bs, "TrainPack", Pack)
    monkeypatch.setattr(bs, "train_forward", fwd)
    monkeypatch.setattr(bs, "train_backward", bwd)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return calls


def test_forward_train_and_trainer_plumbing(monkeypatch):
    calls = _patch_library(monkeypatch)
    torch.manual_seed(2)
    model = EncDecTransformer(200, TARGETS, **KW)
    x, pos = torch.randn(3, 9, 200), torch.rand(3, 9, 2)
    targets = {t: nn.functional.one_hot(torch.randint(0, n, (3,)), n).float() for t, n in TARGETS.items()}
    weights = {t: torch.rand(n) + 0.5 for t, n in TARGETS.items()}
    out = model.forward_train(x, pos, seed=11)
    assert list(out) == list(TARGETS) and all(out[t].shape == (3, n) for t, n in TARGETS.items())
    assert calls["seeds"] == [11] and calls["p"] == [pytest.approx(0.1)]
    loss = multi_target_loss(out, targets, weights)
    loss.backward()
    assert calls["bwd"] == 1
    # the stand-in's arithmetic in plain torch autograd
    ref = {n: q.detach().clone().requires_grad_(True) for n, q in model.named_parameters()}
    pooled = x.mean(1)[:, :128]
    lg = {t: (pooled + ref[f"class_tokens.{bs.sanitize(t)}"]) @ ref[f"heads.{bs.sanitize(t)}.weight"].t() + ref[f"heads.{bs.sanitize(t)}.bias"] for t in TARGETS}
    multi_target_loss(lg, targets, weights).backward()
    for n, q in model.named_parameters():
        assert q.grad is not None and q.grad.shape == q.shape, n
        want = ref[n].grad if ref[n].grad is not None else torch.zeros_like(q)
        assert torch.allclose(q.grad, want, atol=1e-6), n
    # dropout=False switches every site off (and needs no seed); a float overrides the rate; without a seed one is drawn from torch's generator
    model.forward_train(x, pos, dropout=False)
    assert calls["p"][-1] == 0.0 and calls["seeds"][-1] == 0
    model.forward_train(x, pos, dropout=0.3)
    assert calls["p"][-1] == pytest.approx(0.3) and calls["seeds"][-1] != 0
    with torch.no_grad():
        o2 = model.forward_train(x, pos, seed=11)
    assert not o2["A"].requires_grad and torch.equal(o2["A"], out["A"].detach())
    with pytest.raises(ValueError, match="tile_positions"):
        model.forward_train(x, pos[:, :-1])
    with pytest.raises(ValueError, match="tile_tokens"):
        model.forward_train(x[..., :-1], pos)
    # operand type by torch's flag: "medium" -> bf16, otherwise fp16
    seen = []
    orig = bs.TrainPack

    class Spy(orig):
        def __init__(self, model, get, act, dev):
            seen.append(act)
            super().__init__(model, get, act, dev)

    monkeypatch.setattr(bs, "TrainPack", Spy)
    before = torch.get_float32_matmul_precision()
    try:
        for prec in ("medium", "high"):
            torch.set_float32_matmul_precision(prec)
            model.forward_train(x, pos, seed=1)
    finally:
        torch.set_float32_matmul_precision(before)
    assert seen == [torch.bfloat16, torch.float16]


def test_trainer_steps_fit_and_refuses_cpu(monkeypatch):
    with pytest.raises(RuntimeError, match="GPU"):
        HipBarspoonTrainer(EncDecTransformer(200, TARGETS, **KW), device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        EncDecTransformer(200, TARGETS, **KW).forward_train(torch.zeros(1, 2, 200), torch.zeros(1, 2, 2))
    calls = _patch_library(monkeypatch)
    torch.manual_seed(3)
    model = EncDecTransformer(200, TARGETS, **KW)
    tr = HipBarspoonTrainer.__new__(HipBarspoonTrainer)          # (the constructor moves the module to a GPU; the rest is host logic)
    tr.dev, tr.model, tr.dropout, tr.steps = torch.device("cpu"), model, None, 0
    tr.optimizer = torch.optim.Adam(model.parameters(), lr=1e-2)
    tr._gen = torch.Generator().manual_seed(0)
    assert isinstance(tr.optimizer, torch.optim.Adam) and not isinstance(tr.optimizer, torch.optim.AdamW)
    x, pos = torch.randn(4, 9, 200), torch.rand(4, 9, 2)
    targets = {t: nn.functional.one_hot(torch.randint(0, n, (4,)), n).float() for t, n in TARGETS.items()}
    before = {n: q.detach().clone() for n, q in model.named_parameters()}
    loss0, logits = tr.step(x, pos, targets, None, update=False)
    assert all(torch.equal(before[n], q) for n, q in model.named_parameters()) and tr.steps == 0
    assert model.heads["A"].bias.grad is not None
    losses = [tr.step(x, pos, targets)[0].item() for _ in range(8)]
    assert losses[-1] < loss0.item() and tr.steps == 8
    assert len(set(calls["seeds"])) == len(calls["seeds"])                        # a fresh mask seed per step
    # fit: validation after every epoch, early stopping, the best epoch restored
    monkeypatch.setattr(tr, "predict", lambda f, p: {t: v.detach() for t, v in model.forward_train(f, p, dropout=False).items()})
    vals = iter([1.0, 0.5, 0.7, 0.9, 0.8, 0.2])
    snap = {}

    def valid():
        snap[len(snap)] = model.heads["A"].bias.detach().clone()
        return [(x, pos, targets)]

    import stamp_amd.barspoon_train as bt
    real = bt.multi_target_loss

    def loss_spy(lg, tg, w=None):
        if not any(v.requires_grad for v in lg.values()):
            return torch.tensor(next(vals), dtype=torch.float64)
        return real(lg, tg, w)

    monkeypatch.setattr(bt, "multi_target_loss", loss_spy)
    hist = tr.fit(lambda: [(x, pos, targets)], valid, max_epochs=10, patience=3)
    assert hist["validation_loss"] == [1.0, 0.5, 0.7, 0.9, 0.8] and hist["best_epoch"] == 1 and hist["stopped_epoch"] == 4
    assert torch.equal(model.heads["A"].bias.detach(), snap[1])                   # weights as they were when epoch 1 was validated


def test_dropout_rates_must_agree(monkeypatch):
    model = EncDecTransformer(200, TARGETS, **KW)
    assert bs.dropout_rate(model) == pytest.approx(0.1)
    model.transformer_decoder.layers[1].dropout2.p = 0.3
    with pytest.raises(ValueError, match="ONE dropout rate"):
        bs.dropout_rate(model)
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
        with pytest.raises(ValueError, match="disagree"):
            model.forward_train(torch.zeros(1, 2, 200), torch.zeros(1, 2, 2))
    model.transformer_decoder.layers[1].dropout2.p = 0.1
    model.transformer_encoder.layers[0].self_attn.dropout = 0.0
    with pytest.raises(ValueError):
        bs.dropout_rate(model)
