"""Batch isolation (family C of the C-ABI contract tests): every row of ONE bag / sequence / tile of a batch is filled with 0xFF bytes (NaN in every float format);
for every OTHER bag the outputs must stay finite and bit-identical to the all-clean run.  A kernel that lets a key tile, a row tile or a reduction run over the
boundary between two bags cannot pass: NaN times a masked probability of 0 is NaN.

Left out on purpose: the dense amds_transmil_forward and any amds_nystrom_attn_* call of more than one bag -- they share ONE pseudo-inverse scale (the maxima over
all bags' landmark matrices) across the batch, as the reference does at batch > 1 (trans_mil.py:26-28), so a poisoned bag reaches its neighbours by definition; and the
training backwards, whose weight gradients are sums over the bags."""

import pytest
import torch

from stamp_amd import _lib, mil_core, ops
from guarded import cur_stream as _st, ptr as _p

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


def _poison_rows(t, lo, hi):
    """A copy of `t` with rows lo .. hi - 1 set to 0xFF bytes."""
    d = t.clone()
    d[lo:hi].view(torch.uint8).fill_(0xFF)
    assert not t.is_floating_point() or bool(torch.isnan(d[lo:hi].float()).all())
    return d


def _isolated(run, x, spans, out_rows, victims=None):
    """run(x) -> {name: tensor}; spans[j] = (lo, hi) rows of x owned by bag j; out_rows(name, j) -> the slice of output `name` that belongs to bag j."""
    clean = {k: v.clone() for k, v in run(x).items()}
    torch.cuda.synchronize()
    for k, v in clean.items():
        assert bool(torch.isfinite(v.float()).all()), k
    for j in (range(len(spans)) if victims is None else victims):
        dirty = run(_poison_rows(x, *spans[j]))
        torch.cuda.synchronize()
        for k, v in dirty.items():
            for i in range(len(spans)):
                if i == j:
                    continue
                sl = out_rows(k, i)
                assert bool(torch.isfinite(v[sl].float()).all()), f"{k}: bag {i} not finite with bag {j} poisoned"
                assert torch.equal(v[sl], clean[k][sl]), f"{k}: bag {i} changed with bag {j} poisoned"


def _even(B, T):
    return [(b * T, (b + 1) * T) for b in range(B)]


# ---- attention ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("entry,B,T,H,hd", [("attention", 3, 129, 4, 64), ("attention", 2, 1025, 8, 64), ("vit", 2, 257, 2, 64), ("vit", 3, 261, 2, 64), ("vit", 2, 257, 2, 80),
                                            ("vit", 2, 33, 1, 64), ("fwd_lse", 2, 129, 3, 64), ("fwd_train", 2, 129, 3, 64), ("alibi", 3, 129, 2, 64), ("masked", 3, 129, 4, 64)])
def test_attention_bags_do_not_see_each_other(gpu, dt, entry, B, T, H, hd):
    lib, D = _lib.lib(), H * hd
    g = torch.Generator().manual_seed(B * T + H)
    qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).to(gpu, dt)
    coords = (torch.rand(B * T, 2, generator=g) * 1000).to(gpu)
    hs = (torch.rand(H, generator=g) * 1e-3).to(gpu)
    pad = (torch.rand(B, T, generator=g) > 0.5).to(torch.uint8)
    pad[:, 0] = 0
    pad = pad.to(gpu)
    code = ops.act_code(dt)

    def run(x):
        out = torch.empty(B * T, D, dtype=torch.bfloat16 if entry == "alibi" else dt, device=gpu)
        o = {"out": out}
        if entry == "attention":
            rc = lib.amds_attention(_p(x), _p(out), B, T, H, code, _st())
        elif entry == "vit":
            rc = lib.amds_attention_vit_hd(_p(x), _p(out), B, T, H, hd, code, _st())
        elif entry in ("fwd_lse", "fwd_train"):
            o["lse"] = torch.empty(B, H, T, device=gpu)
            rc = (lib.amds_attention_fwd_lse(_p(x), _p(out), _p(o["lse"]), B, T, H, code, _st()) if entry == "fwd_lse" else
                  lib.amds_attention_fwd_train(_p(x), _p(out), _p(o["lse"]), B, T, H, code, 0.25, 7, 3, _st()))
        elif entry == "alibi":
            rc = lib.amds_attention_alibi(_p(x), _p(coords), _p(hs), _p(out), B, T, H, code, _st())
        else:
            rc = lib.amds_attention_masked(_p(x), _p(pad), _p(out), B, T, H, H, code, _st())
        _lib.check(rc, entry)
        return o

    _isolated(run, qkv, _even(B, T), lambda k, i: slice(i, i + 1) if k == "lse" else slice(i * T, (i + 1) * T))


BF = torch.bfloat16
TRAIN_ENTRIES = [(e, dt) for e in ("bwd", "bwd_train", "row_train") for dt in DTYPES] + [("alibi_train", BF), ("row_alibi_train", BF), ("row_alibi_train", torch.float16),
                                                                                       ("alibi_masked", BF), ("alibi_masked", torch.float16)]


@pytest.mark.parametrize("entry,dt", TRAIN_ENTRIES, ids=[f"{e}-{str(d).split('.')[-1]}" for e, d in TRAIN_ENTRIES])
def test_attention_training_entries_bags_do_not_see_each_other(gpu, entry, dt):
    """The per-bag training entries, forward and backward together (their dqkv, lse and d bias_scale partials are per bag; only WEIGHT gradients sum over bags, and these
    produce none): amds_attention_fwd_lse + _bwd, _fwd_train + _bwd_train (p = 0.25), the row pair, the ALiBi pair, the row ALiBi pair; and amds_attention_alibi_masked.
    The poisoned bag's qkv rows make its own out / lse NaN, which its backward then reads -- the other bags' must not.  Rows the row forms leave alone start as zeros."""
    lib, (B, T, H) = _lib.lib(), (3, 129, 2)
    D, code, p = H * 64, ops.act_code(dt), 0.25
    g = torch.Generator().manual_seed(17)
    qkv = (torch.randn(B * T, 3 * D, generator=g) * 0.8).to(gpu, dt)
    dout = (torch.randn(B * T, D, generator=g) * 0.5).to(gpu, dt)
    coords = torch.rand(B, T, 2, generator=g) * 4000.0
    coords[:, 0] = 0.0
    coords = coords.reshape(B * T, 2).to(gpu)
    bs, rm = (torch.rand(H, generator=g) * 0.5 + 0.1).to(gpu), (torch.rand(H, generator=g) * 500.0 + 1800.0).to(gpu)
    inv_rm, ds = 1.0 / rm, bs / rm
    pad = (torch.rand(B, T, generator=g) > 0.5).to(torch.uint8)
    pad[:, 0] = 0
    pad = pad.to(gpu)
    z = lambda *sh, d=dt: torch.zeros(*sh, dtype=d, device=gpu)  # noqa: E731

    def run(x):
        o = {"out": z(B * T, D, d=BF if entry == "alibi_masked" else dt)}
        if entry == "alibi_masked":
            _lib.check(lib.amds_attention_alibi_masked(_p(x), _p(coords), _p(ds), _p(pad), _p(o["out"]), B, T, H, code, _st()), entry)
            return o
        o["lse"], o["dqkv"] = z(B, H, T, d=torch.float32), z(B * T, 3 * D)
        ws = z(B, H, T, d=torch.float32)
        if entry == "bwd":
            _lib.check(lib.amds_attention_fwd_lse(_p(x), _p(o["out"]), _p(o["lse"]), B, T, H, code, _st()), "fwd_lse")
            _lib.check(lib.amds_attention_bwd(_p(x), _p(o["out"]), _p(dout), _p(o["lse"]), _p(ws), _p(o["dqkv"]), B, T, H, code, _st()), "bwd")
        elif entry == "bwd_train":
            _lib.check(lib.amds_attention_fwd_train(_p(x), _p(o["out"]), _p(o["lse"]), B, T, H, code, p, 7, 3, _st()), "fwd_train")
            _lib.check(lib.amds_attention_bwd_train(_p(x), _p(o["out"]), _p(dout), _p(o["lse"]), _p(ws), _p(o["dqkv"]), B, T, H, code, p, 7, 3, _st()), "bwd_train")
        elif entry == "row_train":
            _lib.check(lib.amds_attention_row_fwd_train(_p(x), _p(o["out"]), _p(o["lse"]), B, T, H, 0, code, p, 7, 3, _st()), "row_fwd_train")
            _lib.check(lib.amds_attention_row_bwd_train(_p(x), _p(o["out"]), _p(dout), _p(o["lse"]), _p(o["dqkv"]), B, T, H, 0, code, p, 7, 3, _st()), "row_bwd_train")
        elif entry == "alibi_train":
            o["u"], o["osm"], o["dbs_part"] = z(B * T, D), z(B * T, D), z(B, H, T, d=torch.float32)
            _lib.check(lib.amds_attention_alibi_fwd_train(_p(x), _p(coords), _p(inv_rm), _p(bs), _p(o["out"]), _p(o["u"]), _p(o["osm"]), _p(o["lse"]), B, T, H, code, _st()), "alibi fwd")
            _lib.check(lib.amds_attention_alibi_bwd(_p(x), _p(o["osm"]), _p(o["u"]), _p(dout), _p(o["lse"]), _p(coords), _p(bs), _p(ds), _p(ws), _p(o["dbs_part"]), _p(o["dqkv"]),
                                                    B, T, H, _st()), "alibi bwd")
        else:
            o["u"], o["osm"], o["dbs"] = z(B * T, D), z(B * T, D), z(B, H, d=torch.float32)
            _lib.check(lib.amds_attention_row_alibi_fwd_train(_p(x), _p(coords), _p(inv_rm), _p(bs), _p(o["out"]), _p(o["u"]), _p(o["osm"]), _p(o["lse"]), B, T, H, 0, code, _st()),
                       "row alibi fwd")
            _lib.check(lib.amds_attention_row_alibi_bwd_train(_p(x), _p(o["osm"]), _p(o["u"]), _p(dout), _p(o["lse"]), _p(coords), _p(bs), _p(inv_rm), _p(o["dqkv"]), _p(o["dbs"]),
                                                              B, T, H, 0, code, _st()), "row alibi bwd")
        return o

    _isolated(run, qkv, _even(B, T), lambda k, i: slice(i, i + 1) if k in ("lse", "dbs", "dbs_part") else slice(i * T, (i + 1) * T))


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_row_forms_bags_do_not_see_each_other(gpu, dt):
    """amds_attention_row and amds_attention_cls_f32: one query per bag against that bag's keys / values only."""
    lib, (B, T, H) = _lib.lib(), (3, 212, 4)
    D = H * 64
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(B * T, 3 * D, generator=g) * 1.5).to(gpu, dt)
    q16, q32 = (torch.randn(B, D, generator=g) * 1.5).to(gpu, dt), torch.randn(B, D, generator=g).to(gpu)

    def run(x):
        o16, o32 = torch.empty(B, D, dtype=dt, device=gpu), torch.empty(B, D, device=gpu)
        _lib.check(lib.amds_attention_row(_p(q16), D, _p(x), _p(o16), D, B, T, H, ops.act_code(dt), _st()), "attention_row")
        _lib.check(lib.amds_attention_cls_f32(_p(q32), D, _p(x), _p(o32), D, B, T, H, 64, ops.act_code(dt), _st()), "attention_cls_f32")
        return {"row": o16, "cls_f32": o32}

    _isolated(run, qkv, _even(B, T), lambda k, i: slice(i, i + 1))


def test_attention_varlen_bags_do_not_see_each_other(gpu):
    lib, H = _lib.lib(), 4
    tiles = [1, 77, 300, 63]
    n, total, mx = len(tiles), sum(tiles), max(tiles)
    M, D = total + n, H * 64
    g = torch.Generator().manual_seed(9)
    qkv = (torch.randn(M, 3 * D, generator=g) * 0.5).half().to(gpu)
    coords, hs = (torch.rand(M, 2, generator=g) * 1000).to(gpu), (torch.rand(H, generator=g) * 1e-3).to(gpu)
    q = (torch.randn(n, D, generator=g) * 0.5).half().to(gpu)
    o = [0]
    for t in tiles:
        o.append(o[-1] + t)
    offs = torch.tensor(o, dtype=torch.int32, device=gpu)
    spans = [(o[i] + i, o[i + 1] + i + 1) for i in range(n)]
    need = lib.amds_attention_varlen_workspace_bytes(n, total)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=gpu)

    def run(x):
        out, outa, outr = torch.empty(M, D, dtype=torch.float16, device=gpu), torch.empty(M, D, dtype=torch.bfloat16, device=gpu), torch.empty(n, D, dtype=torch.float16, device=gpu)
        _lib.check(lib.amds_attention_varlen(_p(x), _p(offs), _p(out), n, total, mx, H, _lib.F16, _p(ws), need, _st()), "varlen")
        _lib.check(lib.amds_attention_alibi_varlen(_p(x), _p(coords), _p(hs), _p(offs), _p(outa), n, total, mx, H, _lib.F16, _p(ws), need, _st()), "alibi_varlen")
        _lib.check(lib.amds_attention_row_varlen(_p(q), D, _p(x), _p(offs), _p(outr), D, n, total, mx, H, _lib.F16, _p(ws), need, _st()), "row_varlen")
        return {"plain": out, "alibi": outa, "row": outr}

    _isolated(run, qkv, spans, lambda k, i: slice(i, i + 1) if k == "row" else slice(*spans[i]))


@pytest.mark.parametrize("grid,heads,shift", [(14, 12, 3), (7, 24, 0)])
def test_window_attention_tiles_do_not_see_each_other(gpu, grid, heads, shift):
    from stamp_amd.swin import rel_bias_lane_table, shift_mask_bits
    B, L = 3, grid * grid
    g = torch.Generator().manual_seed(grid)
    qkv = (torch.randn(B * L, 3 * heads * 32, generator=g) * 1.5).half().to(gpu)
    lane, bits = rel_bias_lane_table(torch.randn(169, heads, generator=g)).to(gpu), shift_mask_bits().to(gpu)
    _isolated(lambda x: {"out": ops.window_attention(x, lane, bits, B, grid, heads, shift)}, qkv, _even(B, L), lambda k, i: slice(i * L, (i + 1) * L))


# ---- whole-model calls, below the Python overflow re-run ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alibi", [False, True])
@pytest.mark.parametrize("tail", [True, False])
def test_mil_vit_forward_bags_do_not_see_each_other(gpu, alibi, tail):
    """amds_mil_vit_forward through mil_core.forward_infer (the model's forward above it would re-run a non-finite fp16 result on bf16)."""
    from test_gpu_mil_ragged import REFDIMS, _model
    m = _model(REFDIMS, alibi, seed=3).to(gpu)
    pk = m._infer_pack(gpu)
    Bb, T, F = 3, 130, REFDIMS["dim_input"]
    g = torch.Generator().manual_seed(2)
    bags, coords = torch.randn(Bb * T, F, generator=g).half().to(gpu), (torch.rand(Bb, T, 2, generator=g) * 2000).to(gpu)
    was = ops.set_mil_cls_tail(tail)
    try:
        with torch.no_grad():
            _isolated(lambda x: {"logits": mil_core.forward_infer(pk, x.view(Bb, T, F), coords, None)}, bags, _even(Bb, T), lambda k, i: slice(i, i + 1))
    finally:
        ops.set_mil_cls_tail(was)


@pytest.mark.parametrize("alibi", [False, True])
def test_mil_vit_forward_ragged_bags_do_not_see_each_other(gpu, alibi):
    """amds_mil_vit_forward_ragged through mil_core.forward_infer_ragged: bags of 1, 77, 300 and 64 tiles packed back to back."""
    from test_gpu_mil_ragged import REFDIMS, _model
    m = _model(REFDIMS, alibi, seed=3).to(gpu)
    pk = m._infer_pack(gpu)
    lengths = [1, 77, 300, 64]
    g = torch.Generator().manual_seed(4)
    feats, cc = torch.randn(sum(lengths), REFDIMS["dim_input"], generator=g).half().to(gpu), (torch.rand(sum(lengths), 2, generator=g) * 2000).to(gpu)
    o = [0]
    for t in lengths:
        o.append(o[-1] + t)
    offs = torch.tensor(o, dtype=torch.int32, device=gpu)

    def run(x):
        with torch.no_grad():
            return {"logits": mil_core.forward_infer_ragged(pk, mil_core.RaggedBags(x, cc if alibi else None, offs, tuple(lengths)))}

    _isolated(run, feats, list(zip(o[:-1], o[1:])), lambda k, i: slice(i, i + 1))


def test_transmil_forward_ragged_bags_do_not_see_each_other(gpu):
    """amds_transmil_forward_ragged: every bag has its own grid, padding and pseudo-inverse scale, so -- unlike the dense call -- a poisoned bag stays alone."""
    from stamp_amd import transmil_core
    from test_gpu_transmil_ragged import _model
    m = _model(24, 64).to(gpu)
    lengths = [1, 50, 300, 50]                     # two bags share a bucket of equal np
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(sum(lengths), 24, generator=g).to(gpu)
    o = [0]
    for t in lengths:
        o.append(o[-1] + t)
    w = m._c_weights(gpu)

    def run(x):
        with torch.no_grad():
            return {"logits": transmil_core.forward_infer_ragged(w, (24, 64, 3), [x[a:e] for a, e in zip(o[:-1], o[1:])])}

    _isolated(run, feats, list(zip(o[:-1], o[1:])), lambda k, i: slice(i, i + 1))


@pytest.mark.parametrize("mode", ["slab", "split"])
def test_gated_attn_pool_batched_bags_do_not_see_each_other(gpu, mode):
    from oracle.gated_attention import KEYS
    from test_gpu_seams import _gap_sd
    sd, g = _gap_sd(384, 256, 256, seed=384)
    w = {k: sd[v].to(gpu).contiguous() for k, v in KEYS.items()}
    lens = [1, 64, 63, 65, 17, 300, 16]
    x = torch.randn(sum(lens), 384, generator=g).to(gpu)
    o = [0]
    for t in lens:
        o.append(o[-1] + t)
    spans = list(zip(o[:-1], o[1:]))

    def run(a):
        out, araw = ops.gated_attn_pool_batched(a, lens, w, return_attn=True, mode=mode)
        return {"out": out, "attn_raw": araw}

    _isolated(run, x, spans, lambda k, i: slice(i, i + 1) if k == "out" else slice(*spans[i]))


# ---- row kernels: a "bag" is a block of rows ------------------------------------------------------------------------------------------------------
def test_row_kernels_rows_do_not_see_each_other(gpu):
    """amds_layernorm, amds_layernorm_train, amds_ln_stats_cast, amds_softmax_rows, amds_mean_pool, amds_landmark_mean and amds_dwconv_seq: blocks of rows that end
    inside a workgroup's row group (37 rows each)."""
    lib, (B, T, D) = _lib.lib(), (4, 37, 256)
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(B * T, D, generator=g) * 2 + 0.5).to(gpu)
    gamma, beta = (1 + 0.2 * torch.randn(D, generator=g)).to(gpu), (0.1 * torch.randn(D, generator=g)).to(gpu)

    def run(a):
        o = {"ln": torch.empty(B * T, D, dtype=torch.float16, device=gpu), "ln_train": torch.empty(B * T, D, dtype=torch.bfloat16, device=gpu),
             "mean": torch.empty(B * T, device=gpu), "rstd": torch.empty(B * T, device=gpu), "xh": torch.empty(B * T, D, dtype=torch.float16, device=gpu),
             "rowstat": torch.empty(B * T, 2, device=gpu), "softmax": a.clone(), "pool": torch.empty(B, D, device=gpu)}
        _lib.check(lib.amds_layernorm(_p(a), D, _p(gamma), _p(beta), _p(o["ln"]), D, B * T, D, 1e-5, _lib.F16, _st()), "layernorm")
        _lib.check(lib.amds_layernorm_train(_p(a), D, _p(gamma), _p(beta), _p(o["ln_train"]), D, _p(o["mean"]), _p(o["rstd"]), B * T, D, 1e-5, _lib.BF16, _st()), "ln_train")
        _lib.check(lib.amds_ln_stats_cast(_p(a), D, B * T, D, 1e-6, _p(o["xh"]), D, _p(o["rowstat"]), _lib.F16, _st()), "ln_stats_cast")
        _lib.check(lib.amds_softmax_rows(_p(o["softmax"]), B * T, D, _st()), "softmax_rows")
        _lib.check(lib.amds_mean_pool(_p(a), _p(o["pool"]), B, T, D, _lib.F32, _st()), "mean_pool")
        return o

    _isolated(run, x, _even(B, T), lambda k, i: slice(i, i + 1) if k == "pool" else slice(i * T, (i + 1) * T))
    # TransMIL's per-(bag, head) kernels on a packed qkv [b][np][3 C]
    b_, H, np_, d, m, taps = 3, 8, 70, 8, 35, 33
    Cd = H * d
    qkv = torch.randn(b_ * np_, 3 * Cd, generator=g).to(gpu)
    wc = (torch.randn(H, taps, generator=g) * 0.2).to(gpu)

    def run2(a):
        lm, conv = torch.empty(b_ * H * m, d, device=gpu), torch.zeros(b_ * np_, Cd, device=gpu)
        _lib.check(lib.amds_landmark_mean(_p(a), np_ * 3 * Cd, d, 3 * Cd, _p(lm), b_, H, m, 2, d, 0.5, _st()), "landmark_mean")
        _lib.check(lib.amds_dwconv_seq(a.data_ptr() + 2 * Cd * 4, np_ * 3 * Cd, d, 3 * Cd, _p(wc), _p(conv), np_ * Cd, d, Cd, b_, H, np_, d, taps, _st()), "dwconv_seq")
        return {"lm": lm, "conv": conv}

    _isolated(run2, qkv, _even(b_, np_), lambda k, i: slice(i * H * m, (i + 1) * H * m) if k == "lm" else slice(i * np_, (i + 1) * np_))
