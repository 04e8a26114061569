"""Ragged bags through the barspoon head: N bags of different lengths packed without padding, one library call (amds_barspoon_forward_ragged and the
class-token-less varlen attention entry), each bag's logits bit-identical to its own amds_barspoon_forward call."""
import ctypes as C
import functools
import itertools

import pytest
import torch

from guarded import FLAT_BAND_BYTES, Bufs, cur_stream, guarded, ptr, run_contract
from oracle import barspoon as ob
from stamp_amd import _lib, mil_core, ops
from stamp_amd.barspoon import EncDecTransformer

pytestmark = pytest.mark.gpu

# both sides of the 64-key tile and of the 128-query block; one-tile and two-tile bags
LENGTHS = [1, 63, 64, 65, 127, 128, 129, 300, 2]
GEOMS = {
    # encoder head_dim 32 (zero-padded heads, Ha padding), decoder head_dim 64, widths that are no multiples of 256
    "small": dict(F=96, targets={"KRAS": 2, "MSI status": 3, "grade-x": 4},
                  kw=dict(d_model=128, num_encoder_heads=4, num_decoder_heads=2, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=256)),
    "default": dict(F=768, targets={"A": 2, "B-1": 5}, kw={}),
}


@functools.lru_cache(maxsize=None)
def _model(geom: str, pe: bool):
    g = GEOMS[geom]
    torch.manual_seed(11)
    m = EncDecTransformer(g["F"], g["targets"], positional_encoding=pe, **g["kw"]).eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to("cuda:0"), sd


@functools.lru_cache(maxsize=None)
def _bags(geom: str, half: bool, lengths=tuple(LENGTHS), seed=1):
    """CPU bags (fp16-exact values; fp16 or fp32 storage) and positions."""
    g = torch.Generator().manual_seed(seed)
    bags = [torch.randn(t, GEOMS[geom]["F"], generator=g).half() for t in lengths]
    pos = [torch.rand(t, 2, generator=g) * 50000.0 for t in lengths]
    return [b if half else b.float() for b in bags], pos


@functools.lru_cache(maxsize=None)
def _per_bag(geom: str, half: bool, pe: bool, precision: str):
    """Each bag's own dense call (the yardstick for bits), computed once and shared."""
    m, _ = _model(geom, pe)
    bags, pos = _bags(geom, half)
    with torch.no_grad(), ops.float32_matmul_precision(precision):
        return [m(b.cuda()[None], p.cuda()[None] if pe else None) for b, p in zip(bags, pos)]


def _ragged(m, bags, pos, pe, **kw):
    with torch.no_grad():
        return m.forward_ragged([b.cuda() for b in bags], [p.cuda() for p in pos] if pe else None, **kw)


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("pe", [True, False])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("geom", ["small", "default"])
def test_forward_ragged_equals_per_bag_calls(gpu, geom, half, pe, precision):
    m, _ = _model(geom, pe)
    bags, pos = _bags(geom, half)
    one = _per_bag(geom, half, pe, precision)
    targets = GEOMS[geom]["targets"]
    n = len(bags)
    with ops.float32_matmul_precision(precision):
        out = _ragged(m, bags, pos, pe)                                      # N = 9, one call
        again = _ragged(m, bags, pos, pe)
        assert list(out) == list(targets)
        for t, k in targets.items():
            assert out[t].shape == (n, k) and out[t].dtype == torch.float32 and torch.isfinite(out[t]).all()
            assert torch.equal(out[t], again[t]), t
            for i in range(n):
                assert torch.equal(out[t][i:i + 1], one[i][t]), (t, i, LENGTHS[i], out[t][i], one[i][t])
        for i in (0, 7):                                                     # N = 1
            solo = _ragged(m, bags[i:i + 1], pos[i:i + 1], pe)
            for t in targets:
                assert torch.equal(solo[t], one[i][t]), (t, i)
        for k in (2, 4, 9):                                                  # groups of k, and the same bags in reversed order
            fw = _ragged(m, bags, pos, pe, bags_per_call=k)
            rv = _ragged(m, bags[::-1], pos[::-1], pe, bags_per_call=k)
            for t in targets:
                assert torch.equal(fw[t], out[t]), (t, k)
                assert torch.equal(rv[t].flip(0), out[t]), (t, k)


@pytest.mark.parametrize("pe", [True, False])
@pytest.mark.parametrize("geom", ["small", "default"])
def test_forward_ragged_matches_oracle(gpu, geom, pe):
    """The bar tests/test_gpu_barspoon.py states for this head: 5e-3 of the logit scale (fp16 MFMA operands on the tile side, fp32 accumulation)."""
    m, sd = _model(geom, pe)
    bags, pos = _bags(geom, True)
    targets = GEOMS[geom]["targets"]
    out = _ragged(m, bags, pos, pe)
    kw = GEOMS[geom]["kw"]
    for i, (b, p) in enumerate(zip(bags, pos)):
        ref = ob.barspoon_forward(b.float()[None], p[None], sd, list(targets), num_encoder_heads=kw.get("num_encoder_heads", 8),
                                  num_decoder_heads=kw.get("num_decoder_heads", 8), positional_encoding=pe)
        for t in targets:
            err = (out[t][i:i + 1].cpu() - ref[t]).abs().max().item()
            print(f"{geom} pe={pe} bag {i} ({LENGTHS[i]} tiles) {t}: err {err:.3e} scale {ref[t].abs().max().item():.3e}")
            assert err < 5e-3 * max(1.0, ref[t].abs().max().item()), (i, t, err)


@pytest.mark.parametrize("geom", ["small", "default"])
def test_a_nan_bag_leaves_the_other_bags_bits(gpu, geom):
    m, _ = _model(geom, True)
    bags, pos = _bags(geom, True)
    targets = GEOMS[geom]["targets"]
    out = _ragged(m, bags, pos, True)
    for bad in (0, 4, 8):
        poisoned = list(bags)
        poisoned[bad] = torch.full_like(bags[bad], float("nan"))
        got = _ragged(m, poisoned, pos, True)
        for t in targets:
            keep = [i for i in range(len(bags)) if i != bad]
            assert torch.equal(got[t][keep], out[t][keep]), (t, bad)


def test_long_bag_runs_alone_and_keeps_its_bits(gpu, monkeypatch):
    """Default geometry: the widest GEMM (T, 2048, 512) leaves the small-problem kernel at ceil(T / 256) * 8 >= 192, so the limit is finite (5888) and a
    bag of limit + 1 tiles between two short ones takes a call of its own."""
    m, _ = _model("default", True)
    limit = m.max_shared_tiles(gpu)
    assert 1 <= limit < 100000
    lengths = (5, limit + 1, 7)
    bags, pos = _bags("default", True, lengths=lengths, seed=3)
    assert mil_core.group_bags(lengths, len(lengths), 1 << 62, limit, extra_rows=0) == [(0, 1), (1, 2), (2, 3)]
    assert mil_core.group_bags((5, limit, 7), 3, 1 << 62, limit, extra_rows=0) == [(0, 3)]
    calls = []
    real = mil_core.pack_bags
    monkeypatch.setattr(mil_core, "pack_bags", lambda *a, **k: calls.append(real(*a, **k)) or calls[-1])
    out = _ragged(m, bags, pos, True)
    assert [rb.lengths for rb in calls] == [(5,), (limit + 1,), (7,)]          # one library call per group
    with torch.no_grad():
        for i, (b, p) in enumerate(zip(bags, pos)):
            one = m(b.cuda()[None], p.cuda()[None])
            for t in GEOMS["default"]["targets"]:
                assert torch.equal(out[t][i:i + 1], one[t]), (t, i)


# ---- the class-token-less varlen attention entry against the fixed-pitch one, bag by bag ---------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("H", [8, 6])
def test_attention_varlen_rows_equals_per_bag_calls(gpu, H, dt):
    """H = 6 twice: as six heads, and as the model callers lay it out -- padded to 8 heads of which two are zero."""
    lib = _lib.lib()
    st = cur_stream()
    code = _lib.F16 if dt == torch.float16 else _lib.BF16
    n, total, mx = len(LENGTHS), sum(LENGTHS), max(LENGTHS)
    offs = torch.tensor([0] + list(itertools.accumulate(LENGTHS)), dtype=torch.int32, device=gpu)
    ws = torch.empty(max(int(lib.amds_attention_varlen_workspace_bytes(n, total)), 256), dtype=torch.uint8, device=gpu)
    g = torch.Generator().manual_seed(9)
    layouts = [(H, None)] + ([(8, 6)] if H == 6 else [])
    for Hc, live in layouts:
        Dm = Hc * 64
        qkv = torch.randn(total, 3, Hc, 64, generator=g) * 0.5
        if live is not None:
            qkv[:, :, live:] = 0
        qkv = qkv.reshape(total, 3 * Dm).to(dt).to(gpu)
        out = torch.empty(total, Dm, dtype=dt, device=gpu)
        _lib.check(lib.amds_attention_varlen_rows(qkv.data_ptr(), offs.data_ptr(), out.data_ptr(), n, total, mx, Hc, code, ws.data_ptr(), ws.numel(), st))
        r0 = 0
        for i, T in enumerate(LENGTHS):
            sl = qkv[r0:r0 + T].contiguous()
            ref = torch.empty(T, Dm, dtype=dt, device=gpu)
            _lib.check(lib.amds_attention(sl.data_ptr(), ref.data_ptr(), 1, T, Hc, code, st))
            assert torch.equal(out[r0:r0 + T], ref), (Hc, live, i, T)
            r0 += T
        assert torch.isfinite(out.float()).all()


# ---- the C contract ---------------------------------------------------------------------------------------------------------------------------------
def test_forward_ragged_c_contract(gpu):
    """The call on a guarded workspace poisoned with 0x00 and with 0xFF: logits bit-identical between the two, finite, every band intact.  feats, positions
    and offsets sit in guarded buffers (the ABI takes them contiguous -- it has no pitch argument -- so their poison is in the bands)."""
    lib = _lib.lib()
    m, _ = _model("small", True)
    pack = m._pack(gpu)
    cfg, wc = pack.cfg, pack.wc
    lengths = (5, 130, 64, 1)
    bags, pos = _bags("small", True, lengths=lengths, seed=5)
    n, total, mx = len(lengths), sum(lengths), max(lengths)
    feats, posc = torch.cat(bags), torch.cat(pos)
    offsets = torch.tensor([0] + list(itertools.accumulate(lengths)), dtype=torch.int32)
    need = lib.amds_barspoon_ragged_workspace_bytes(C.byref(cfg), n, total, mx)
    assert need > 0

    def call(pattern):
        B = Bufs(gpu, pattern)
        f, p, o = B.inp(feats, name="feats"), B.inp(posc, name="positions"), B.inp(offsets, name="offsets")
        lg = B.out((n, pack.total_out), torch.float32, name="logits")
        ws, h = guarded((need,), torch.uint8, gpu, band_bytes=FLAT_BAND_BYTES, pattern=pattern, name="ws")
        B.handles.append(h)
        _lib.check(lib.amds_barspoon_forward_ragged(C.byref(cfg), C.byref(wc), ptr(f), _lib.F16, ptr(p), ptr(o), ptr(lg), n, total, mx, ptr(ws), need, cur_stream()),
                   "barspoon_forward_ragged")
        return B.result(logits=lg)

    got = run_contract(call)["logits"]
    want = _ragged(m, bags, pos, True)
    assert torch.equal(got, torch.cat([want[t] for t in GEOMS["small"]["targets"]], dim=1))

    # host-side refusals
    f, p, o = feats.to(gpu), posc.to(gpu), offsets.to(gpu)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=gpu)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256
    logits = torch.full((n, pack.total_out), 7.0, device=gpu)
    dflt = dict(cfg=C.byref(cfg), w=C.byref(wc), feats=f.data_ptr(), pos=p.data_ptr(), offs=o.data_ptr(), logits=logits.data_ptr(), n=n, total=total, mx=mx, ws=base,
                ws_bytes=need)

    def run(**kw):
        a = dict(dflt, **kw)
        return lib.amds_barspoon_forward_ragged(a["cfg"], a["w"], a["feats"], _lib.F16, a["pos"], a["offs"], a["logits"], a["n"], a["total"], a["mx"], a["ws"],
                                                a["ws_bytes"], cur_stream())

    for k in ("cfg", "w", "feats", "offs", "logits", "ws"):
        assert run(**{k: None}) == -1 and b"null pointer" in lib.amds_last_error(), k
    assert run(ws_bytes=need - 1) == -2 and b"workspace" in lib.amds_last_error()                  # AMDS_ERR_WORKSPACE
    assert run(ws=base + 16) == -1 and b"256-byte aligned" in lib.amds_last_error()
    assert run(pos=None) == -1 and b"needs tile positions" in lib.amds_last_error()
    span = (1 << 31) // (3 * 4 * 128) + 1                                                          # Ha = 4: max_tiles * 3 * Ha * 128 >= 2^31
    assert run(mx=span) == -1 and b"2 GB" in lib.amds_last_error()
    assert run(mx=span - 2) == 0                                                                   # (a bound, not a length: the clamps take the shorter)
    assert run(n=0, total=0, mx=0) == 0
    torch.cuda.synchronize()
    logits.fill_(7.0)
    assert run(n=0, total=0, mx=0) == 0                                                            # AMDS_OK, nothing launched
    torch.cuda.synchronize()
    assert bool((logits == 7.0).all())


# ---- predict_ and fit -----------------------------------------------------------------------------------------------------------------------------------
def test_predict_grouped_equals_one_bag_loop(gpu):
    from stamp_amd.deploy import predict_

    m, _ = _model("small", True)
    g = torch.Generator().manual_seed(12)
    F = GEOMS["small"]["F"]
    shapes = [(1, 40), (1, 1), (1, 129), (2, 33), (1, 64), (1, 300), (1, 7), (1, 65)]             # seven one-bag batches, one two-bag batch in the middle
    batches = [(torch.randn(b, t, F, generator=g).half(), torch.rand(b, t, 2, generator=g) * 50000.0, None, None) for b, t in shapes]
    pids = [f"p{i}" for i in range(sum(b for b, _ in shapes))]
    base = predict_(m, batches, pids, task="classification", device=gpu)
    got = predict_(m, batches, pids, task="classification", device=gpu, bags_per_call=4)
    assert list(got) == list(base) == pids
    for pid in pids:
        assert list(got[pid]) == list(GEOMS["small"]["targets"])
        for t in got[pid]:
            assert torch.equal(got[pid][t], base[pid][t]), (pid, t)


def test_fit_with_grouped_validation_equals_default(gpu):
    from stamp_amd.barspoon_train import HipBarspoonTrainer

    Fd, targets = 32, {"A": 2, "B": 3}
    g = torch.Generator().manual_seed(21)

    def onehot(n):
        return {t: torch.nn.functional.one_hot(torch.randint(0, k, (n,), generator=g), k).float() for t, k in targets.items()}

    train = [(torch.randn(4, 24, Fd, generator=g), torch.rand(4, 24, 2, generator=g) * 500, onehot(4)) for _ in range(3)]
    valid = [(torch.randn(1, t, Fd, generator=g), torch.rand(1, t, 2, generator=g) * 500, onehot(1)) for t in (5, 70, 1, 33, 128, 129, 90, 12, 65, 64, 7)]

    def run(**kw):
        torch.manual_seed(0)
        model = EncDecTransformer(Fd, targets, d_model=64, num_encoder_heads=2, num_decoder_heads=1, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=64)
        tr = HipBarspoonTrainer(model, device=gpu, learning_rate=1e-3, dropout=False, seed=3)
        hist = tr.fit(lambda: train, lambda: valid, max_epochs=3, patience=8, **kw)
        return hist, {k: v.detach().clone() for k, v in model.state_dict().items()}

    h1, p1 = run()
    h8, p8 = run(valid_bags_per_call=8)
    assert len(h1["validation_loss"]) == 3
    assert h1["validation_loss"] == h8["validation_loss"] and h1["best_epoch"] == h8["best_epoch"]
    assert p1.keys() == p8.keys() and all(torch.equal(p1[k], p8[k]) for k in p1)
