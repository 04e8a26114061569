"""Ragged bags through the MIL `vit` head: N bags of different lengths packed without padding, one library call
(amds_mil_vit_forward_ragged and the varlen attention entries), each bag's logits bit-identical to its own call."""
import ctypes as C
import random

import pytest
import torch

from oracle.mil_vit import mil_vit_forward
from stamp_amd import _lib, mil_core
from stamp_amd.mil import VisionTransformer

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 1000, 1024, 3001]
DEFAULT = dict(dim_input=1024, dim_model=512, n_heads=8, dim_feedforward=512, n_layers=2)
REFDIMS = dict(dim_input=456, dim_model=4 * 33, n_heads=4, dim_feedforward=135, n_layers=3)       # the reference's tests/test_model.py:9-32


def _model(dims, alibi, C=3, seed=0):
    torch.manual_seed(seed)
    m = VisionTransformer(dim_output=C, dropout=0.0, use_alibi=alibi, **dims).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1 and "class_token" not in n and "bias_scale" not in n:
                p.add_(0.05 * torch.randn_like(p))
    return m


def _bags(lengths, F, seed=1):
    g = torch.Generator().manual_seed(seed)
    bags = [torch.randn(t, F, generator=g).half() for t in lengths]
    coords = [torch.rand(t, 2, generator=g) * 2000 for t in lengths]
    return bags, coords


@pytest.mark.parametrize("alibi", [False, True])
@pytest.mark.parametrize("dims", ["default", "reference"])
def test_forward_ragged_equals_per_bag_calls(gpu, alibi, dims):
    d = DEFAULT if dims == "default" else REFDIMS
    m = _model(d, alibi).to(gpu)
    lengths = LENGTHS[:]
    random.Random(7).shuffle(lengths)
    bags, coords = _bags(lengths, d["dim_input"])
    bags, coords = [b.to(gpu) for b in bags], [c.to(gpu) for c in coords]
    with torch.no_grad():
        out = m.forward_ragged(bags, coords=coords)
        assert out.shape == (len(bags), 3) and torch.isfinite(out).all()
        for i, (b, c) in enumerate(zip(bags, coords)):
            one = m(b[None], coords=c[None], mask=None)
            assert torch.equal(out[i:i + 1], one), (i, lengths[i], out[i], one)


@pytest.mark.parametrize("alibi", [False, True])
def test_forward_ragged_matches_oracle(gpu, alibi):
    m = _model(REFDIMS, alibi, seed=3)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    lengths = [75, 1, 129, 300, 64]
    bags, coords = _bags(lengths, REFDIMS["dim_input"], seed=4)
    m = m.to(gpu)
    with torch.no_grad():
        out = m.forward_ragged([b.to(gpu) for b in bags], coords=[c.to(gpu) for c in coords]).cpu()
    for i, (b, c) in enumerate(zip(bags, coords)):
        ref = mil_vit_forward(b.float()[None], c[None], None, sd, n_heads=4, use_alibi=alibi)[0]
        assert (out[i] - ref).abs().max() < 6e-3 * max(1.0, ref.abs().max().item()), (i, out[i], ref)


def test_long_bag_in_a_group_equals_per_bag_calls(gpu):
    """A bag of 33 000 tiles (past the class-row tail's 32 768 tokens) among short ones: it runs in a call of its own, the others share one."""
    m = _model(DEFAULT, False).to(gpu)
    lengths = [300, 33000, 5, 1200]
    bags, _ = _bags(lengths, 1024, seed=5)
    bags = [b.to(gpu) for b in bags]
    with torch.no_grad():
        out = m.forward_ragged(bags)
        for i, b in enumerate(bags):
            assert torch.equal(out[i:i + 1], m(b[None], mask=None)), (i, lengths[i])
    pk = m._infer_pack(gpu)
    assert mil_core.max_shared_tiles(pk) < 33000


# ---- the varlen attention entries against the fixed-pitch ones, bag by bag -----------------------------------------------------------
def _ws(n):
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device="cuda")


def _offsets(lengths, dev):
    o = [0]
    for t in lengths:
        o.append(o[-1] + t)
    return torch.tensor(o, dtype=torch.int32, device=dev), o


@pytest.mark.parametrize("H", [8, 6])
def test_attention_varlen_entries_equal_per_bag_calls(gpu, H):
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    tiles = [127, 0, 128, 255, 256, 1000, 63, 383]                  # token counts 128, 1, 129, 256, 257, 1001, 64, 384: both sides of the 128-query blocks
    n, total, mx = len(tiles), sum(tiles), max(tiles)
    M, Dm = total + n, H * 64
    g = torch.Generator().manual_seed(9)
    qkv = (torch.randn(M, 3 * Dm, generator=g) * 0.5).half().to(gpu)
    coords = (torch.rand(M, 2, generator=g) * 1000).to(gpu)
    hs = (torch.rand(H, generator=g) * 1e-3).to(gpu)
    q = (torch.randn(n, Dm, generator=g) * 0.5).half().to(gpu)
    offs, o = _offsets(tiles, gpu)
    ws = _ws(lib.amds_attention_varlen_workspace_bytes(n, total))
    out = torch.empty(M, Dm, dtype=torch.float16, device=gpu)
    _lib.check(lib.amds_attention_varlen(qkv.data_ptr(), offs.data_ptr(), out.data_ptr(), n, total, mx, H, _lib.F16, ws.data_ptr(), ws.numel(), st))
    outa = torch.empty(M, Dm, dtype=torch.bfloat16, device=gpu)
    _lib.check(lib.amds_attention_alibi_varlen(qkv.data_ptr(), coords.data_ptr(), hs.data_ptr(), offs.data_ptr(), outa.data_ptr(), n, total, mx, H, _lib.F16,
                                               ws.data_ptr(), ws.numel(), st))
    outr = torch.empty(n, Dm, dtype=torch.float16, device=gpu)
    _lib.check(lib.amds_attention_row_varlen(q.data_ptr(), Dm, qkv.data_ptr(), offs.data_ptr(), outr.data_ptr(), Dm, n, total, mx, H, _lib.F16,
                                             ws.data_ptr(), ws.numel(), st))
    for i, t in enumerate(tiles):
        r0, T = o[i] + i, t + 1
        sl = qkv[r0:r0 + T].contiguous()
        ref = torch.empty(T, Dm, dtype=torch.float16, device=gpu)
        _lib.check(lib.amds_attention(sl.data_ptr(), ref.data_ptr(), 1, T, H, _lib.F16, st))
        assert torch.equal(out[r0:r0 + T], ref), (i, T)
        cs = coords[r0:r0 + T].contiguous()
        refa = torch.empty(T, Dm, dtype=torch.bfloat16, device=gpu)
        _lib.check(lib.amds_attention_alibi(sl.data_ptr(), cs.data_ptr(), hs.data_ptr(), refa.data_ptr(), 1, T, H, _lib.F16, st))
        assert torch.equal(outa[r0:r0 + T], refa), (i, T)
        refr = torch.empty(1, Dm, dtype=torch.float16, device=gpu)
        qi = q[i:i + 1].contiguous()
        _lib.check(lib.amds_attention_row(qi.data_ptr(), Dm, sl.data_ptr(), refr.data_ptr(), Dm, 1, T, H, _lib.F16, st))
        assert torch.equal(outr[i:i + 1], refr), (i, T)


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def test_ragged_edges(gpu):
    m = _model(REFDIMS, True).to(gpu)
    bags, coords = _bags([40], REFDIMS["dim_input"], seed=6)
    b, c = bags[0].to(gpu), coords[0].to(gpu)
    with torch.no_grad():
        one = m.forward_ragged([b], coords=[c])
        assert torch.equal(one, mil_core.forward_infer(m._infer_pack(gpu), b[None], c[None], None))
        assert m.forward_ragged([]).shape == (0, 3)
        with pytest.raises(ValueError):
            m.forward_ragged([b, b[:0]], coords=[c, c[:0]])
        with pytest.raises(ValueError):
            m.forward_ragged([b[:, :100]], coords=[c])
        with pytest.raises(ValueError):
            m.forward_ragged([b])                                   # ALiBi without coords
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_ragged([b], coords=[c])                           # grad enabled
    m.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval"):
        m.forward_ragged([b], coords=[c])


def test_ragged_c_guards(gpu):
    lib = _lib.lib()
    m = _model(REFDIMS, False).to(gpu)
    cfg, wc = m._infer_pack(gpu).c_structs()
    st = torch.cuda.current_stream().cuda_stream
    feats = torch.zeros(10, REFDIMS["dim_input"], dtype=torch.float16, device=gpu)
    offs = torch.tensor([0, 4, 10], dtype=torch.int32, device=gpu)
    logits = torch.empty(2, 3, device=gpu)
    need = lib.amds_mil_vit_ragged_workspace_bytes(C.byref(cfg), 2, 10, 6)
    assert need > 0 and lib.amds_mil_vit_ragged_workspace_bytes(C.byref(cfg), -1, 10, 6) == 0
    ws = _ws(need)
    args = lambda **kw: dict(dict(feats=feats.data_ptr(), offs=offs.data_ptr(), n=2, ws_bytes=ws.numel()), **kw)  # noqa: E731

    def call(a):
        return lib.amds_mil_vit_forward_ragged(C.byref(cfg), C.byref(wc), a["feats"], _lib.F16, None, a["offs"], logits.data_ptr(), a["n"], 10, 6,
                                               ws.data_ptr(), a["ws_bytes"], st)

    assert call(args(feats=None)) != 0 and b"null pointer" in lib.amds_last_error()
    assert call(args(n=-1)) != 0 and b"bad shape" in lib.amds_last_error()
    assert call(args(ws_bytes=need - 1)) != 0 and b"workspace" in lib.amds_last_error()
    assert call(args(n=0)) == 0
    assert call(args()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all()
    qkv = torch.zeros(12, 3 * 256, dtype=torch.float16, device=gpu)
    assert lib.amds_attention_varlen(None, offs.data_ptr(), qkv.data_ptr(), 2, 10, 6, 4, _lib.F16, ws.data_ptr(), ws.numel(), st) != 0
    assert b"null pointer" in lib.amds_last_error()
    assert lib.amds_attention_row_varlen(qkv.data_ptr(), 256, qkv.data_ptr(), offs.data_ptr(), qkv.data_ptr(), 256, 2, 10, 6, 4, _lib.F16, ws.data_ptr(), 1,
                                         st) != 0
    assert b"workspace" in lib.amds_last_error()


# ---- predict_ and fit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["classification", "regression", "survival"])
def test_predict_grouped_equals_one_bag_loop(gpu, task):
    from stamp_amd.deploy import predict_

    m = _model(dict(dim_input=256, dim_model=128, n_heads=2, dim_feedforward=256, n_layers=2), False, C=3 if task == "classification" else 1, seed=11)
    g = torch.Generator().manual_seed(12)
    lengths = [int(x) for x in torch.randint(1, 900, (23,), generator=g)]
    batches = [(torch.randn(1, t, 256, generator=g).half(), torch.rand(1, t, 2, generator=g), None, None) for t in lengths]
    pids = [f"p{i}" for i in range(len(lengths))]
    base = predict_(m, batches, pids, task=task, device=gpu)
    for k in (7, 64):
        got = predict_(m, batches, pids, task=task, device=gpu, bags_per_call=k)
        assert list(got) == list(base)
        for pid in pids:
            assert torch.equal(got[pid], base[pid]), (k, pid)


@pytest.mark.parametrize("alibi", [False, True])
def test_fit_with_grouped_validation_equals_default(gpu, alibi):
    from stamp_amd.mil_train import HipMilVitTrainer, fit

    Fd = 64
    g = torch.Generator().manual_seed(21)
    train = []
    for _ in range(4):
        y = torch.randint(0, 2, (6,), generator=g)
        bags = torch.randn(6, 32, Fd, generator=g) + (y.float() * 2 - 1)[:, None, None]
        train.append((bags, torch.rand(6, 32, 2, generator=g) * 500, None, torch.nn.functional.one_hot(y, 2).float()))
    valid = []
    for t in [5, 70, 1, 33, 128, 129, 90, 12, 300, 64, 7]:
        y = torch.randint(0, 2, (1,), generator=g)
        bags = torch.randn(1, t, Fd, generator=g) + (y.float() * 2 - 1)[:, None, None]
        valid.append((bags, torch.rand(1, t, 2, generator=g) * 500, None, torch.nn.functional.one_hot(y, 2).float()))

    def run(**kw):
        torch.manual_seed(0)
        model = VisionTransformer(dim_output=2, dim_input=Fd, dim_model=64, n_layers=1, n_heads=2, dim_feedforward=64, dropout=0.0, use_alibi=alibi)
        tr = HipMilVitTrainer(model, device=gpu, max_lr=3e-3, total_steps=12, sched_interval="step", dropout=False)
        hist = fit(tr, lambda: train, lambda: valid, max_epochs=3, patience=8, **kw)
        return hist, tr.P.clone()

    h1, p1 = run()
    h8, p8 = run(valid_bags_per_call=8)
    assert h1["validation_loss"] == h8["validation_loss"] and h1["best_epoch"] == h8["best_epoch"]
    assert torch.equal(p1, p8)
