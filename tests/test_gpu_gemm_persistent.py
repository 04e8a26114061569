"""The persistent form of the production GEMM (gemm_4w16.h PERSIST: kernel id 16, and id 12 unless AMDS_GEMM_PERSIST=0) against the one-tile-per-
workgroup form of the same library.

Both forms run the same K loop and the same streamed epilogue per output tile; the persistent one walks several tiles per workgroup, prefetches the
next tile's first operands under the last K tile and keeps the epilogue's stores in flight under the next tile.  Per-tile arithmetic and order are
unchanged, so the yardstick is the library with AMDS_GEMM_PERSIST=0 and the bar is torch.equal: no tolerance.  Operands sit in guarded allocations
(tests/guarded.py): poison 0x00 and 0xFF, outputs bit-identical between the two, finite, bands and pitch padding untouched.

On a 256-CU part a small problem has fewer tiles than workgroups and nothing would loop: AMDS_GEMM_PERSIST_WGS=8 (unless stated) makes 18 tiles a walk
of 2-3 tiles per workgroup.  Shapes: (1300, 768) = 6 x 3 tiles with a ragged last row tile; (257, 2304) = 2 x 9 with a nearly empty row tile that
several workgroups visit; (513, 512) = 6 tiles, fewer than the grid; (2048, 256) = 8 tiles, exactly the grid.  K = 64 ... 256 is 1 ... 4 K tiles: both
stage parities per output tile, and the case where the last K tile is also the first."""

import pytest
import torch

import guarded as G
from guarded import Bufs, cur_stream as _st, ptr as _p
from stamp_amd import _lib, ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
EPIS = {"BIAS": _lib.EPI_BIAS, "GELU": _lib.EPI_BIAS_GELU}
PERSIST, WGS, STREAM = "AMDS_GEMM_PERSIST", "AMDS_GEMM_PERSIST_WGS", "AMDS_GEMM_EPI_STREAM"
SHAPES = [(1300, 768), (257, 2304), (513, 512), (2048, 256)]


def _operands(M, N, K, dt, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(dt)
    a[:, 0] += torch.arange(M).to(dt) * 0.01                 # rows differ: a tile stored at another tile's place cannot pass
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dt)
    w[:, 0] += (torch.arange(N) * 0.003).to(dt)             # ... and so do columns
    bias = torch.randn(N, generator=g)
    rowstat = torch.stack([0.5 + torch.rand(M, generator=g), torch.randn(M, generator=g)], 1).contiguous()
    colsum = torch.randn(N, generator=g)
    return a, w, bias, rowstat, colsum


def _gemm_ex(cfg, a, w, bias, M, N, K, dt, code, out_ptr, ldo, what):
    _lib.check(_lib.lib().amds_gemm_ex(cfg, _p(a), a.stride(0), _p(w), w.stride(0), M, N, K, ops.act_code(dt), code, out_ptr, ldo, _p(bias), None, None, 0, 0, 0,
                                       1.0, _st()), what)


def _lnfold(a, w, bias, rowstat, colsum, M, N, K, dt, code, out_ptr, ldo, what):
    _lib.check(_lib.lib().amds_gemm_lnfold(_p(a), a.stride(0), _p(w), w.stride(0), M, N, K, ops.act_code(dt), code, out_ptr, ldo, _p(bias), None, None, None,
                                           _p(rowstat), _p(colsum), _st()), what)


def _launches():
    return _lib.lib().amds_gemm_persist_launches()


@pytest.fixture
def env(monkeypatch):
    for k in (PERSIST, WGS, STREAM):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(WGS, "8")
    return monkeypatch


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N", SHAPES)
def test_tile_walk_equals_one_tile_per_workgroup(gpu, env, M, N, dt):
    """amds_gemm_ex(16) and the amds_gemm_lnfold consumer, BIAS and BIAS_GELU, K = 64 ... 256 (and 1024 once), pitch N and N + 8: same bits as with
    AMDS_GEMM_PERSIST=0, under both poison bytes, bands and padding untouched; the persistent instantiation did run."""
    for K in (64, 128, 192, 256) + ((1024,) if (M, N) == (1300, 768) else ()):
        a0, w0, bias0, rs0, cs0 = _operands(M, N, K, dt, M * 7 + N + K)
        for pad in (0, 8):
            if K == 1024 and pad:
                continue
            for epi, code in EPIS.items():
                tag = (M, N, K, pad, epi, dt)

                def call(pattern):
                    b = Bufs(gpu, pattern)
                    a, w, bias = b.inp(a0, name="A"), b.inp(w0, name="W"), b.inp(bias0, name="bias")
                    rs, cs = b.inp(rs0, name="rowstat"), b.inp(cs0, name="colsum")
                    outs = {k: b.out((M, N), dt, N + pad, k) for k in ("ex_persist", "ex_one_tile", "ln_persist", "ln_one_tile")}
                    n0 = _launches()
                    _gemm_ex(16, a, w, bias, M, N, K, dt, code, _p(outs["ex_persist"]), N + pad, f"gemm_ex 16 {tag}")
                    _lnfold(a, w, bias, rs, cs, M, N, K, dt, code, _p(outs["ln_persist"]), N + pad, f"lnfold {tag}")
                    assert _launches() == n0 + 2, tag
                    env.setenv(PERSIST, "0")
                    _gemm_ex(12, a, w, bias, M, N, K, dt, code, _p(outs["ex_one_tile"]), N + pad, f"gemm_ex 12, switch off {tag}")
                    _lnfold(a, w, bias, rs, cs, M, N, K, dt, code, _p(outs["ln_one_tile"]), N + pad, f"lnfold, switch off {tag}")
                    env.delenv(PERSIST)
                    assert _launches() == n0 + 2, tag
                    return b.result(**outs)

                o = G.run_contract(call)
                assert torch.equal(o["ex_persist"], o["ex_one_tile"]), tag
                assert torch.equal(o["ln_persist"], o["ln_one_tile"]), tag
                assert not torch.equal(o["ex_persist"], o["ln_persist"]), tag          # (the two entries are different computations)


@pytest.mark.parametrize("dt", DTYPES)
def test_column_window_of_a_wider_row(gpu, env, dt):
    """The output is a window of N columns inside rows of 3 N (pointer offset by N columns, ldo = 3 N), as in the K | V launch of the encoder's last
    block: the window equals the one-tile form's and the columns on both sides of it keep their poison."""
    M, N, K = 1300, 768, 128
    a0, w0, bias0, rs0, cs0 = _operands(M, N, K, dt, 11)
    item = 2

    def call(pattern):
        b = Bufs(gpu, pattern)
        a, w, bias = b.inp(a0, name="A"), b.inp(w0, name="W"), b.inp(bias0, name="bias")
        rs, cs = b.inp(rs0, name="rowstat"), b.inp(cs0, name="colsum")
        outs = {k: b.out((M, 3 * N), dt, 3 * N, k) for k in ("ex_persist", "ex_one_tile", "ln_persist", "ln_one_tile")}
        win = {k: _p(v) + N * item for k, v in outs.items()}
        _gemm_ex(16, a, w, bias, M, N, K, dt, _lib.EPI_BIAS_GELU, win["ex_persist"], 3 * N, "window, id 16")
        _lnfold(a, w, bias, rs, cs, M, N, K, dt, _lib.EPI_BIAS, win["ln_persist"], 3 * N, "window, lnfold")
        env.setenv(PERSIST, "0")
        _gemm_ex(12, a, w, bias, M, N, K, dt, _lib.EPI_BIAS_GELU, win["ex_one_tile"], 3 * N, "window, id 12, switch off")
        _lnfold(a, w, bias, rs, cs, M, N, K, dt, _lib.EPI_BIAS, win["ln_one_tile"], 3 * N, "window, lnfold, switch off")
        env.delenv(PERSIST)
        torch.cuda.synchronize()
        for k, v in outs.items():
            outside = torch.cat([v[:, :N], v[:, 2 * N:]], 1).contiguous().view(torch.uint8)
            assert bool((outside == pattern).all()), f"{k}: columns outside the window were written (poison 0x{pattern:02X})"
        return G.Result({k: v[:, N:2 * N] for k, v in outs.items()}, b.handles)

    o = G.run_contract(call)
    assert torch.equal(o["ex_persist"], o["ex_one_tile"])
    assert torch.equal(o["ln_persist"], o["ln_one_tile"])


@pytest.mark.parametrize("dt", DTYPES)
def test_switches(gpu, env, dt):
    """Id 16 = id 12 with the switch unset (both persistent); id 12 with AMDS_GEMM_PERSIST=0 = id 14; AMDS_GEMM_EPI_STREAM=0 gives the same bits and, by
    the library's launch counter, runs no persistent instantiation -- not for id 16 either."""
    M, N, K = 1300, 768, 128
    a0, w0, bias0, _, _ = _operands(M, N, K, dt, 5)
    a, w, bias = a0.to(gpu), w0.to(gpu), bias0.to(gpu)

    def run(cfg):
        out = torch.full((M, N), float("nan"), dtype=dt, device=gpu)
        n0 = _launches()
        _gemm_ex(cfg, a, w, bias, M, N, K, dt, _lib.EPI_BIAS_GELU, _p(out), N, f"cfg {cfg}")
        return out, _launches() - n0

    ref, n = run(14)
    assert n == 0 and bool(torch.isfinite(ref).all())
    for cfg in (16, 12):
        out, n = run(cfg)
        assert n == 1 and torch.equal(out, ref), cfg
    out, n = run(13)
    assert n == 0 and torch.equal(out, ref)
    env.setenv(PERSIST, "0")
    out, n = run(12)
    assert n == 0 and torch.equal(out, ref)
    out, n = run(16)
    assert n == 1 and torch.equal(out, ref)
    env.delenv(PERSIST)
    env.setenv(STREAM, "0")
    for cfg in (16, 12):
        out, n = run(cfg)
        assert n == 0 and torch.equal(out, ref), cfg


@pytest.mark.parametrize("M,N,K", [(1300, 768, 128), (1300, 768, 192), (257, 2304, 256)])
def test_repeated_calls_give_the_same_bits(gpu, env, M, N, K):
    """The tile loop is a new synchronisation structure (slab stage against the next tile's LDS-DMA, prefetched stage against its first reads): 50 calls
    on the same inputs, the output freshly poisoned each time, all bit-equal to the one-tile form; and once each with the grid capped at 16 and 24
    workgroups -- other tile-to-workgroup assignments."""
    dt = torch.float16
    a0, w0, bias0, rs0, cs0 = _operands(M, N, K, dt, 23)
    a, w, bias, rs, cs = (t.to(gpu) for t in (a0, w0, bias0, rs0, cs0))

    def run(lnf, poison):
        out = torch.full((M, N), poison, dtype=dt, device=gpu)
        if lnf:
            _lnfold(a, w, bias, rs, cs, M, N, K, dt, _lib.EPI_BIAS_GELU, _p(out), N, "lnfold")
        else:
            _gemm_ex(16, a, w, bias, M, N, K, dt, _lib.EPI_BIAS_GELU, _p(out), N, "gemm_ex 16")
        return out

    env.setenv(PERSIST, "0")
    ref = {lnf: run(lnf, float("nan")) for lnf in (False, True)}
    env.delenv(PERSIST)
    assert all(bool(torch.isfinite(r).all()) for r in ref.values())
    for lnf in (False, True):
        for it in range(50):
            assert torch.equal(run(lnf, float("nan") if it & 1 else 0.0), ref[lnf]), (lnf, it)
        for cap in ("16", "24"):
            env.setenv(WGS, cap)
            assert torch.equal(run(lnf, float("nan")), ref[lnf]), (lnf, cap)
        env.setenv(WGS, "8")


def test_small_vit_features_equal_with_the_switch_on_and_off(gpu, env):
    """A depth-4 ViT whose LayerNorms are folded into the GEMMs (qkv and fc1 are amds_gemm_lnfold consumers, kernel id 12), 5 tiles in chunks of 3:
    same feature bits with the persistent form, with AMDS_GEMM_PERSIST=0, and with the persistent grid capped at 8 workgroups."""
    from stamp_amd.vit import PRESETS, HipViT, random_vit_state_dict

    cfg = PRESETS["test_tiny_fold"]
    sd = random_vit_state_dict(cfg, seed=2)
    tiles = torch.randint(0, 256, (5, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(gpu)
    model = HipViT(cfg, sd, device=gpu, chunk=3)
    assert model.ln_fold
    capped = model(tiles)
    env.delenv(WGS)
    on = model(tiles)
    env.setenv(PERSIST, "0")
    off = model(tiles)
    env.delenv(PERSIST)
    assert bool(torch.isfinite(on.float()).all())
    assert torch.equal(on, off)
    assert torch.equal(capped, off)
