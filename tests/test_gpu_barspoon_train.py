"""Training the barspoon head on the HIP path: the training cross-attention alone, the whole step against fp64 autograd of the oracle (with and
without dropout, the library's own masks fed to a masked twin), edges, the module / trainer front end and the C-ABI contract of the two calls."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import barspoon as ob
from stamp_amd import _lib, barspoon as bs, ops
from stamp_amd import train_ops as T
from stamp_amd.barspoon import EncDecTransformer
from stamp_amd.barspoon_train import HipBarspoonTrainer, multi_target_loss
import guarded as gd

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634


# ---- the cross-attention alone ----------------------------------------------------------------------------------------------------------------
CA_SHAPES = [(1, 1, 1, 1, 64), (2, 63, 3, 2, 64), (1, 65, 1, 2, 32), (3, 200, 5, 2, 64), (1, 1025, 3, 8, 64), (2, 129, 17, 1, 16)]


def _ca_inputs(B, Tn, nt, H, hd, dt, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * Tn + nt)
    q = torch.randn(B, nt, H * hd, generator=g)
    kv = torch.zeros(B * Tn, 2, H, 64)
    kv[..., :hd] = torch.randn(B * Tn, 2, H, hd, generator=g)            # channels >= hd are the zero padding of the K | V projection
    kv = kv.reshape(B * Tn, 128 * H).to(dt)
    dout = torch.randn(B, nt, H * hd, generator=g)
    return q, kv, dout


def _ca_reference(q, kv, dout, B, Tn, nt, H, hd, mult):
    """fp64 autograd on the same 16-bit-rounded K | V; `mult` [B, H, nt, Tn]: keep mask times keep scale (1 everywhere without dropout)."""
    qd = q.double().requires_grad_(True)
    kvd = kv.double().requires_grad_(True)
    k = kvd.view(B, Tn, 2, H, 64)[:, :, 0, :, :hd].permute(0, 2, 1, 3)       # [B, H, Tn, hd]
    v = kvd.view(B, Tn, 2, H, 64)[:, :, 1, :, :hd].permute(0, 2, 1, 3)
    qh = qd.view(B, nt, H, hd).permute(0, 2, 1, 3)
    s = qh @ k.transpose(-1, -2) / hd ** 0.5
    out = ((torch.softmax(s, -1) * mult) @ v).permute(0, 2, 1, 3).reshape(B, nt, H * hd)
    out.backward(dout.double())
    return out.detach(), torch.logsumexp(s.detach(), -1) * LOG2E, qd.grad, kvd.grad


def _ca_check(gpu, shape, dt, p, seed):
    B, Tn, nt, H, hd = shape
    q, kv, dout = _ca_inputs(*shape, dt)
    sid = 5003
    mult = torch.ones(B, H, nt, Tn, dtype=torch.float64)
    if p > 0:
        keep = T.attention_dropout_mask_rows(B * H * nt, Tn, p, seed, sid, gpu).view(B, H, nt, Tn).cpu().double()
        mult = keep * _lib.lib().amds_dropout_keep_scale(p)
    r_out, r_lse, r_dq, r_dkv = _ca_reference(q, kv, dout, *shape, mult)
    qg, kvg, dg = q.to(gpu), kv.to(gpu), dout.to(gpu)
    out, lse = T.cross_attention_fwd_train(qg, kvg, B, Tn, nt, H, hd, p, seed, sid)
    dq, dkv = T.cross_attention_bwd_train(qg, kvg, out, dg, lse, B, Tn, nt, H, hd, p, seed, sid)
    dq2, dkv2 = T.cross_attention_bwd_train(qg, kvg, out, dg, lse, B, Tn, nt, H, hd, p, seed, sid)
    eps = gd.act_eps(dt)
    e_out = (out.cpu().double() - r_out).abs().max().item()
    e_lse = (lse.cpu().double() - r_lse).abs().max().item()
    e_dq = (dq.cpu().double() - r_dq).abs().max().item()
    e_dkv = (dkv.cpu().double() - r_dkv).abs().max().item()
    print(f"cross-attention {shape} {dt} p={p}: out {e_out:.3e} lse {e_lse:.3e} dq {e_dq:.3e} dkv {e_dkv:.3e}")
    assert e_out < 4 * eps * max(1.0, r_out.abs().max().item()), (e_out, r_out.abs().max().item())
    assert e_lse < 1e-2, e_lse
    assert e_dq < 8 * eps * max(1.0, r_dq.abs().max().item()), (e_dq, r_dq.abs().max().item())
    assert e_dkv < 8 * eps * max(1.0, r_dkv.abs().max().item()), (e_dkv, r_dkv.abs().max().item())
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)                  # deterministic: a second backward is bit-equal
    if p > 0:
        out0, lse0 = T.cross_attention_fwd_train(qg, kvg, B, Tn, nt, H, hd, 0.0, seed, sid)
        assert torch.equal(lse, lse0)                                       # the saved statistic is that of the undropped softmax


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", CA_SHAPES)
def test_cross_attention_forward_backward_vs_autograd(gpu, shape, dt):
    """out within 4 eps max(1, |ref|max), dq / dkv within 8 eps max(1, |g|max), lse within 1e-2 (eps = 2^-7 bf16, 2^-10 fp16: the bars of
    test_attention_backward_vs_autograd), against fp64 autograd on the same 16-bit-rounded K | V; without dropout, and with p = 0.25 and the
    read-back mask fed to the oracle."""
    _ca_check(gpu, shape, dt, 0.0, 0)
    _ca_check(gpu, shape, dt, 0.25, 991 + shape[1])


def test_cross_attention_mask_keep_rate(gpu):
    p = 0.3
    m = T.attention_dropout_mask_rows(2 * 4 * 8, 1 << 14, p, 12345, 5003, gpu)           # 2^20 mask elements
    assert m.numel() >= 1 << 20
    want = 1.0 - round(p * 65536) / 65536
    rate = m.float().mean().item()
    assert abs(rate - want) < 0.01 * want, (rate, want)


# ---- the whole step -----------------------------------------------------------------------------------------------------------------------------
GEOMS = {
    "padded": dict(F=200, targets={"A": 2, "B-1": 5, "C": 3}, Bb=3, Tn=65,
                   kw=dict(d_model=128, num_encoder_heads=4, num_decoder_heads=2, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=192)),
    "aligned": dict(F=256, targets={"only": 4}, Bb=2, Tn=200,
                    kw=dict(d_model=256, num_encoder_heads=4, num_decoder_heads=4, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=256,
                            positional_encoding=False)),
}


def _make(name, seed=3, **over):
    g = GEOMS[name]
    torch.manual_seed(seed)
    kw = dict(g["kw"])
    kw.update(over)
    model = EncDecTransformer(g["F"], g["targets"], **kw)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    Bb, Tn = g["Bb"], g["Tn"]
    x = torch.randn(Bb, Tn, g["F"]).half().float()
    pos = torch.rand(Bb, Tn, 2) * 50000.0
    targets = {t: F.one_hot(torch.randint(0, n, (Bb,)), n).float() for t, n in g["targets"].items()}
    weights = {t: torch.rand(n) + 0.5 for t, n in g["targets"].items()}
    return model, x, pos, targets, weights


def _loss64(logits, targets, weights):
    return sum(F.cross_entropy(logits[t], targets[t].double(), weight=weights[t].double()) for t in logits)


def _twin_forward(x, pos, sd, labels, He, Hd, positional_encoding, mult):
    """fp64 twin of oracle.barspoon.barspoon_forward in TRAIN mode: torch's documented norm_first=True dropout sites, each multiplied by `mult[key]`
    (keep mask x keep scale, stamp_amd.barspoon.step_masks' keys).  With every multiplier 1 it is the oracle itself (asserted by the tests)."""
    lin = F.linear

    def mha(q_in, kv_in, p, H, m):
        D = q_in.shape[-1]
        w, b = sd[p + "in_proj_weight"], sd[p + "in_proj_bias"]
        q, k, v = lin(q_in, w[:D], b[:D]), lin(kv_in, w[D:2 * D], b[D:2 * D]), lin(kv_in, w[2 * D:], b[2 * D:])
        B, Lq, _ = q.shape
        hd = D // H
        q, k, v = (t.view(B, -1, H, hd).transpose(1, 2) for t in (q, k, v))
        a = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1) * m
        return lin((a @ v).transpose(1, 2).reshape(B, Lq, D), sd[p + "out_proj.weight"], sd[p + "out_proj.bias"])

    ln = lambda t, p: F.layer_norm(t, (t.shape[-1],), sd[p + "weight"], sd[p + "bias"], 1e-5)  # noqa: E731
    ff = lambda t, p, m: lin(torch.relu(lin(t, sd[p + "linear1.weight"], sd[p + "linear1.bias"])) * m, sd[p + "linear2.weight"], sd[p + "linear2.bias"])  # noqa: E731
    x = torch.relu(lin(x, sd["projector.0.weight"], sd["projector.0.bias"]))
    if positional_encoding:
        x = x + ob.positional_encodings(pos.to(x.dtype), x.shape[-1])
    l = 0
    while f"transformer_encoder.layers.{l}.norm1.weight" in sd:
        p, e = f"transformer_encoder.layers.{l}.", f"enc{l}."
        h = ln(x, p + "norm1.")
        x = x + mha(h, h, p + "self_attn.", He, mult[e + "attn"]) * mult[e + "sa"]
        x = x + ff(ln(x, p + "norm2."), p, mult[e + "ff1"]) * mult[e + "ff2"]
        l += 1
    t = torch.stack([sd["class_tokens." + ob.sanitize(tl)] for tl in labels]).expand(x.shape[0], -1, -1)
    l = 0
    while f"transformer_decoder.layers.{l}.norm1.weight" in sd:
        p, e = f"transformer_decoder.layers.{l}.", f"dec{l}."
        h = ln(t, p + "norm1.")
        t = t + mha(h, h, p + "self_attn.", Hd, mult[e + "attn"]) * mult[e + "sa"]
        t = t + mha(ln(t, p + "norm2."), x, p + "multihead_attn.", Hd, mult[e + "cattn"]) * mult[e + "ca"]
        t = t + ff(ln(t, p + "norm3."), p, mult[e + "ff1"]) * mult[e + "ff2"]
        l += 1
    return {tl: lin(t[:, j], sd[f"heads.{ob.sanitize(tl)}.weight"], sd[f"heads.{ob.sanitize(tl)}.bias"]) for j, tl in enumerate(labels)}


class _Ones(dict):
    def __missing__(self, k):
        return 1.0


@functools.lru_cache(maxsize=None)
def _reference(name):
    """fp64 autograd of the oracle at one geometry, computed once and shared: (loss, logits, gradients)."""
    model, x, pos, targets, weights = _make(name)
    sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in model.state_dict().items()}
    kw = GEOMS[name]["kw"]
    logits = ob.barspoon_forward(x.double(), pos.double(), sd, list(targets), num_encoder_heads=kw["num_encoder_heads"], num_decoder_heads=kw["num_decoder_heads"],
                                 positional_encoding=kw.get("positional_encoding", True))
    loss = _loss64(logits, targets, weights)
    loss.backward()
    with torch.no_grad():
        twin = _twin_forward(x.double(), pos.double(), {k: v.detach() for k, v in sd.items()}, list(targets), kw["num_encoder_heads"], kw["num_decoder_heads"],
                             kw.get("positional_encoding", True), _Ones())
        assert all(torch.allclose(twin[t], logits[t].detach(), atol=1e-12) for t in targets)          # the masked twin with no masks IS the oracle
    return loss.item(), {t: v.detach() for t, v in logits.items()}, {k: v.grad for k, v in sd.items()}


def _hip_step(model, x, pos, targets, weights, gpu, **kw):
    model.to(gpu).zero_grad(set_to_none=True)
    logits = model.forward_train(x.to(gpu), pos.to(gpu), **kw)
    loss = multi_target_loss(logits, targets, weights)
    loss.backward()
    return loss.item(), {t: v.detach().cpu() for t, v in logits.items()}, {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}


def _compare(tag, got, ref, bar):
    loss, logits, grads = got
    r_loss, r_logits, r_g = ref
    assert abs(loss - r_loss) < 2e-2 * max(1.0, abs(r_loss)), (loss, r_loss)
    for t in r_logits:
        assert (logits[t].double() - r_logits[t]).abs().max() < 3e-2 * max(1.0, r_logits[t].abs().max().item()), t
    worst = (0.0, None)
    for k, r in r_g.items():
        assert r.norm().item() > 0, k                                                               # every parameter has a gradient here
        rel = ((grads[k].double() - r).norm() / r.norm()).item()
        worst = max(worst, (rel, k))
    print(f"{tag}: loss {loss:.6f} (ref {r_loss:.6f}); worst relative-L2 gradient error {worst[0]:.4e} at {worst[1]}")
    for k, r in r_g.items():
        rel = ((grads[k].double() - r).norm() / r.norm()).item()
        assert rel < bar, (k, rel, r.norm().item())
    return worst


@pytest.mark.parametrize("precision", ["medium", "high"])
@pytest.mark.parametrize("name", ["padded", "aligned"])
def test_training_step_matches_fp64_autograd(gpu, name, precision):
    """p = 0: loss within 2e-2 max(1, |ref|), logits within 3e-2 max(1, |ref|max), every parameter gradient below 5e-2 relative L2 (the bars of the MIL
    `vit` step, tests/test_gpu_train.py), on bf16 ("medium") and on fp16 ("high") operands; the worst tensor is printed."""
    model, x, pos, targets, weights = _make(name)
    before = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(precision)
    try:
        got = _hip_step(model, x, pos, targets, weights, gpu, dropout=False)
    finally:
        torch.set_float32_matmul_precision(before)
    assert model.fp16_overflow_events == 0
    _compare(f"barspoon step {name} {precision}", got, _reference(name), 5e-2)


def test_training_step_with_dropout_matches_masked_twin(gpu):
    """p = 0.1 (the module's own rate) at the first geometry: the twin is fed the masks the kernels drew (rebuilt from (p, seed, shapes) by the library's
    generators); bar 6e-2 (the MIL `vit` step's with dropout).  Same seed: bit-equal gradients; another seed: different ones."""
    name, seed = "padded", 424242
    model, x, pos, targets, weights = _make(name)
    kw = GEOMS[name]["kw"]
    assert bs.dropout_rate(model) == pytest.approx(0.1)
    got = _hip_step(model, x, pos, targets, weights, gpu, seed=seed)
    again = _hip_step(model, x, pos, targets, weights, gpu, seed=seed)
    other = _hip_step(model, x, pos, targets, weights, gpu, seed=seed + 1)
    assert all(torch.equal(got[2][k], again[2][k]) for k in got[2])
    assert any(not torch.equal(got[2][k], other[2][k]) for k in got[2])
    p = 0.1
    ks = _lib.lib().amds_dropout_keep_scale(p)
    masks = bs.step_masks(model, x.shape[0], x.shape[1], p, seed, gpu)
    assert 0.85 < torch.cat([m.reshape(-1).float() for m in masks.values()]).mean().item() < 0.95
    mult = {k: m.cpu().double() * ks for k, m in masks.items()}
    sd = {k: v.detach().cpu().clone().double().requires_grad_(True) for k, v in model.state_dict().items()}
    logits = _twin_forward(x.double(), pos.double(), sd, list(targets), kw["num_encoder_heads"], kw["num_decoder_heads"], True, mult)
    loss = _loss64(logits, targets, weights)
    loss.backward()
    ref = (loss.item(), {t: v.detach() for t, v in logits.items()}, {k: v.grad for k, v in sd.items()})
    _compare("barspoon step with dropout", got, ref, 6e-2)


@pytest.mark.parametrize("case", ["one_tile", "one_bag", "no_decoder", "no_encoder"])
def test_training_step_edges(gpu, case):
    over = {"no_decoder": dict(num_decoder_layers=0), "no_encoder": dict(num_encoder_layers=0)}.get(case, {})
    model, x, pos, targets, weights = _make("padded", **over)
    if case == "one_tile":
        x, pos = x[:, :1], pos[:, :1]
    if case == "one_bag":
        x, pos, targets = x[:1], pos[:1], {t: v[:1] for t, v in targets.items()}
    loss, logits, grads = _hip_step(model, x, pos, targets, weights, gpu, seed=5)
    assert loss == loss and abs(loss) < 1e4
    for t, n in GEOMS["padded"]["targets"].items():
        assert logits[t].shape == (x.shape[0], n) and torch.isfinite(logits[t]).all()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    for k, g in grads.items():
        assert tuple(g.shape) == shapes[k] and torch.isfinite(g).all(), k
    if case == "no_decoder":                                # logits are the heads on the raw class tokens: nothing reaches the encoder or the projector
        for j, t in enumerate(targets):
            s = ob.sanitize(t)
            want = F.linear(model.class_tokens[s].detach().cpu(), model.heads[s].weight.detach().cpu(), model.heads[s].bias.detach().cpu())
            assert torch.allclose(logits[t], want.expand(x.shape[0], -1), atol=1e-5)
        for k, g in grads.items():
            if k.startswith(("transformer_encoder.", "projector.")):
                assert not g.any(), k
            else:
                assert g.any(), k


# ---- module and trainer --------------------------------------------------------------------------------------------------------------------------
def test_module_and_trainer(gpu):
    model, x, pos, targets, weights = _make("padded")
    keys = list(model.state_dict())
    ref_model = EncDecTransformer(GEOMS["padded"]["F"], GEOMS["padded"]["targets"], **GEOMS["padded"]["kw"])
    assert keys == list(ref_model.state_dict())                                              # the state_dict keys are unchanged
    seed = 99
    _, _, g_mod = _hip_step(model, x, pos, targets, weights, gpu, seed=seed)
    tr = HipBarspoonTrainer(model, device=gpu, learning_rate=1e-3)
    tr.step(x.to(gpu), pos.to(gpu), targets, weights, update=False, seed=seed)
    for k, p in model.named_parameters():
        r = g_mod[k]
        assert (p.grad.cpu() - r).norm() <= 1e-5 * max(r.norm().item(), 1e-30), k               # forward_train + loss.backward() = the trainer's gradients
    losses = [tr.step(x.to(gpu), pos.to(gpu), targets, weights)[0].item() for _ in range(8)]
    assert losses[-1] < losses[0], losses
    assert all(torch.isfinite(p).all() for p in model.parameters())
    out = tr.predict(x.to(gpu), pos.to(gpu))
    model.eval()
    with torch.no_grad():
        want = model(x.to(gpu), pos.to(gpu))
    assert all(torch.equal(out[t], want[t]) for t in targets)                                  # predict = the eval forward on the updated weights
    with pytest.raises(NotImplementedError, match="deploy / validation"):
        model.train()(x.to(gpu), pos.to(gpu))                                                  # `forward` itself still refuses to train
    with pytest.raises(RuntimeError, match="GPU"):
        model.forward_train(x, pos)
    with pytest.raises(RuntimeError, match="GPU"):
        tr.step(x, pos, targets, weights)
    assert list(model.state_dict()) == keys


# ---- C-ABI contract ---------------------------------------------------------------------------------------------------------------------------------
def test_abi_poisoned_workspace_guard_bands_and_two_backwards(gpu, monkeypatch):
    """`saved`, `ws`, logits and the gradient buffers live in guarded allocations poisoned with 0x00 / 0xFF: identical results under both bytes, every
    guard band intact; two backwards after one forward are bit-equal."""
    model, x, pos, targets, weights = _make("padded")
    model.to(gpu)
    names = [n for n, _ in model.named_parameters()]
    get = lambda n: dict(model.named_parameters())[n].detach().float()  # noqa: E731
    dl = torch.randn(x.shape[0], sum(GEOMS["padded"]["targets"].values()), generator=torch.Generator().manual_seed(1)).to(gpu)

    def call(pattern):
        with gd.scratch_hook(monkeypatch, pattern) as log:
            pack = bs.TrainPack(model, get, torch.bfloat16, gpu)
            logits, saved = bs.train_forward(pack, x.to(gpu), pos.to(gpu), p=0.1, seed=7)
            arena0 = saved["arena"].clone()
            G1 = bs.train_backward(pack, saved, dl, split_k=4)
            G1 = {k: v.clone() for k, v in G1.items()}
            G2 = bs.train_backward(pack, saved, dl, split_k=4)
            assert torch.equal(saved["arena"], arena0)                                       # `saved` is read-only after the forward
            assert all(torch.equal(G1[k], G2[k]) for k in names)
            assert {t for t, _ in log.requests} >= {"alloc", "barspoon_train"}                # arena, logits, gradients; the backward's workspace
        return gd.Result({"logits": logits, **{f"g:{k}": G1[k] for k in names}}, log.handles)

    gd.run_contract(call)


def test_abi_refuses_bad_configurations(gpu):
    lib = _lib.lib()
    ok = _lib.BarspoonCfg(200, 128, 4, 2, 192, 2, 2, 3, 1, _lib.BF16)
    assert lib.amds_barspoon_train_saved_bytes(C.byref(ok), 3, 65) > 0 and lib.amds_barspoon_train_workspace_bytes(C.byref(ok), 3, 65, 4) > 0
    for bad, what in ((_lib.BarspoonCfg(200, 128, 4, 2, 192, 2, 2, 3, 1, _lib.F32), "bf16 or fp16"), (_lib.BarspoonCfg(200, 130, 4, 2, 192, 2, 2, 3, 1, _lib.BF16), "divisible"),
                      (_lib.BarspoonCfg(200, 256, 2, 2, 192, 2, 2, 3, 1, _lib.BF16), "head_dim"), (_lib.BarspoonCfg(200, 128, 4, 2, 192, 2, 2, 0, 1, _lib.BF16), "bad config")):
        assert lib.amds_barspoon_train_saved_bytes(C.byref(bad), 3, 65) == 0
        assert what in lib.amds_last_error().decode()
    assert lib.amds_barspoon_train_saved_bytes(C.byref(ok), 0, 65) == 0 and "bad shape" in lib.amds_last_error().decode()
    assert lib.amds_barspoon_train_workspace_bytes(C.byref(ok), 3, 65, 0) == 0 and "split_k" in lib.amds_last_error().decode()
    # an arena one byte short, a null gradient struct, a dropout rate of 1: refused with a message, nothing launched
    model, x, pos, _, _ = _make("padded")
    model.to(gpu)
    get = lambda n: dict(model.named_parameters())[n].detach().float()  # noqa: E731
    pack = bs.TrainPack(model, get, torch.bfloat16, gpu)
    need = lib.amds_barspoon_train_saved_bytes(C.byref(pack.cfg), 3, 65)
    arena = torch.zeros(need, dtype=torch.uint8, device=gpu)
    logits = torch.zeros(3, pack.total_out, device=gpu)
    xg, pg = x.to(gpu).contiguous(), pos.to(gpu).contiguous()
    drop = _lib.BarspoonDropout(0.0, 0)
    args = lambda nbytes, d: (C.byref(pack.cfg), C.byref(pack.wc), xg.data_ptr(), _lib.F32, pg.data_ptr(), C.byref(d), logits.data_ptr(), 3, 65, arena.data_ptr(), nbytes,  # noqa: E731
                              ops._stream())
    assert lib.amds_barspoon_train_forward(*args(need - 1, drop)) != 0 and "arena" in lib.amds_last_error().decode()
    assert lib.amds_barspoon_train_forward(*args(need, _lib.BarspoonDropout(1.0, 0))) != 0 and "dropout" in lib.amds_last_error().decode()
    torch.cuda.synchronize()
    assert not arena.any() and not logits.any()
    assert lib.amds_barspoon_train_forward(*args(need, drop)) == 0
    ws = torch.zeros(lib.amds_barspoon_train_workspace_bytes(C.byref(pack.cfg), 3, 65, 4), dtype=torch.uint8, device=gpu)
    rc = lib.amds_barspoon_train_backward(C.byref(pack.cfg), C.byref(pack.wc), logits.data_ptr(), C.byref(drop), 3, 65, arena.data_ptr(), need, None, 4, ws.data_ptr(),
                                          ws.numel(), ops._stream())
    assert rc != 0 and "null pointer" in lib.amds_last_error().decode()
