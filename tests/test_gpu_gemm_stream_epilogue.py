"""The streamed 16-bit epilogue of the production GEMM (gemm_4w16.h, kernel ids 12 / 13) against the one-phase form it replaced, which the
library keeps (kernel id 14; AMDS_GEMM_EPI_STREAM=0 for the entries that name id 12 themselves).

The two forms run the same value arithmetic in the same order and differ only in how a tile's values travel through the LDS to memory, so the
yardstick is the one-phase form in the same library and the bar is torch.equal: no tolerance.  (The one-phase form has its own fp64 bars in
test_gpu_abi_gemm.py / test_gpu_kernels.py.)  Every operand sits in a guarded allocation (tests/guarded.py): poison 0x00 and 0xFF, outputs
bit-identical between the two, finite, bands and pitch padding untouched -- the streamed form stores through a buffer descriptor whose range
ends with the last row of the tile that exists, and these cases put rows past M into every wave's quadrant.

Shapes, the smallest that cross every edge of the new code: M = 1, 255, 257, 513 (a ragged last row tile, one full tile + 1, rows past M in all four
waves' quadrants), N = 256 and 512 (one and two column tiles), K = 64, 128, 192 (1, 2, 3 K tiles: every prologue / last-tile form of the K loop in
front of the epilogue), output pitch N and N + 8, and a column window of a row three times as wide (the K | V launch of the encoder's last block)."""

import pytest
import torch

import guarded as G
from guarded import Bufs, cur_stream as _st, ptr as _p
from stamp_amd import _lib, ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
EPIS = {"BIAS": _lib.EPI_BIAS, "GELU": _lib.EPI_BIAS_GELU}
SWITCH = "AMDS_GEMM_EPI_STREAM"


def _operands(M, N, K, dt, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(dt)
    a[:, 0] += torch.arange(M).to(dt) * 0.01                 # rows differ: a swapped or transposed store cannot pass
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dt)
    w[:, 0] += (torch.arange(N) * 0.003).to(dt)             # ... and so do columns
    bias = torch.randn(N, generator=g)
    rowstat = torch.stack([0.5 + torch.rand(M, generator=g), torch.randn(M, generator=g)], 1).contiguous()      # (rstd, -mean rstd) of some rows
    colsum = torch.randn(N, generator=g)
    return a, w, bias, rowstat, colsum


def _gemm_ex(cfg, a, w, bias, M, N, K, dt, code, out_ptr, ldo, what):
    _lib.check(_lib.lib().amds_gemm_ex(cfg, _p(a), a.stride(0), _p(w), w.stride(0), M, N, K, ops.act_code(dt), code, out_ptr, ldo, _p(bias), None, None, 0, 0, 0,
                                       1.0, _st()), what)


def _lnfold(a, w, bias, rowstat, colsum, M, N, K, dt, code, out_ptr, ldo, what):
    _lib.check(_lib.lib().amds_gemm_lnfold(_p(a), a.stride(0), _p(w), w.stride(0), M, N, K, ops.act_code(dt), code, out_ptr, ldo, _p(bias), None, None, None,
                                           _p(rowstat), _p(colsum), _st()), what)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [1, 255, 257, 513])
def test_streamed_epilogue_equals_one_phase(gpu, monkeypatch, M, dt):
    """amds_gemm_ex BIAS / BIAS_GELU at kernel id 12 against id 14, and the amds_gemm_lnfold consumer (BIAS / BIAS_GELU) with the switch unset
    against AMDS_GEMM_EPI_STREAM=0: same bits, under both poison bytes, bands and padding untouched."""
    monkeypatch.delenv(SWITCH, raising=False)
    for N in (256, 512):
        for K in (64, 128, 192):
            a0, w0, bias0, rs0, cs0 = _operands(M, N, K, dt, M * 7 + N + K)
            for pad in (0, 8):
                for epi, code in EPIS.items():
                    tag = (M, N, K, pad, epi, dt)

                    def call(pattern):
                        b = Bufs(gpu, pattern)
                        a, w, bias = b.inp(a0, name="A"), b.inp(w0, name="W"), b.inp(bias0, name="bias")
                        rs, cs = b.inp(rs0, name="rowstat"), b.inp(cs0, name="colsum")
                        outs = {k: b.out((M, N), dt, N + pad, k) for k in ("ex_stream", "ex_one_phase", "ln_stream", "ln_one_phase")}
                        _gemm_ex(12, a, w, bias, M, N, K, dt, code, _p(outs["ex_stream"]), N + pad, f"gemm_ex 12 {tag}")
                        _gemm_ex(14, a, w, bias, M, N, K, dt, code, _p(outs["ex_one_phase"]), N + pad, f"gemm_ex 14 {tag}")
                        _lnfold(a, w, bias, rs, cs, M, N, K, dt, code, _p(outs["ln_stream"]), N + pad, f"lnfold {tag}")
                        monkeypatch.setenv(SWITCH, "0")
                        _lnfold(a, w, bias, rs, cs, M, N, K, dt, code, _p(outs["ln_one_phase"]), N + pad, f"lnfold, switch off {tag}")
                        monkeypatch.delenv(SWITCH)
                        return b.result(**outs)

                    o = G.run_contract(call)
                    assert torch.equal(o["ex_stream"], o["ex_one_phase"]), tag
                    assert torch.equal(o["ln_stream"], o["ln_one_phase"]), tag
                    assert not torch.equal(o["ex_stream"], o["ln_stream"]), tag          # (the two forms are different computations)


@pytest.mark.parametrize("dt", DTYPES)
def test_switch_turns_ids_12_and_13_back(gpu, monkeypatch, dt):
    """AMDS_GEMM_EPI_STREAM=0 is read at every call and reaches ids 12 and 13 of amds_gemm_ex as well; id 14 does not depend on it."""
    M, N, K = 257, 512, 128
    a0, w0, bias0, _, _ = _operands(M, N, K, dt, 5)
    a, w, bias = a0.to(gpu), w0.to(gpu), bias0.to(gpu)
    monkeypatch.delenv(SWITCH, raising=False)
    got = {}
    for env in (None, "0", "1"):
        if env is not None:
            monkeypatch.setenv(SWITCH, env)
        for cfg in (12, 13, 14):
            out = torch.full((M, N), float("nan"), dtype=dt, device=gpu)
            _gemm_ex(cfg, a, w, bias, M, N, K, dt, _lib.EPI_BIAS_GELU, _p(out), N, f"cfg {cfg} env {env}")
            got[env, cfg] = out
    ref = got[None, 14]
    assert bool(torch.isfinite(ref).all())
    for key, out in got.items():
        assert torch.equal(out, ref), key


@pytest.mark.parametrize("dt", DTYPES)
def test_column_window_of_a_wider_row(gpu, monkeypatch, dt):
    """The output is a window of N columns inside rows of 3 N (pointer offset by N columns, ldo = 3 N), as in the K | V launch of the encoder's last
    block: the window equals the one-phase form's, and the columns on both sides of it keep their poison."""
    M, N, K = 257, 256, 128
    a0, w0, bias0, rs0, cs0 = _operands(M, N, K, dt, 11)
    item = 2
    monkeypatch.delenv(SWITCH, raising=False)

    def call(pattern):
        b = Bufs(gpu, pattern)
        a, w, bias = b.inp(a0, name="A"), b.inp(w0, name="W"), b.inp(bias0, name="bias")
        rs, cs = b.inp(rs0, name="rowstat"), b.inp(cs0, name="colsum")
        outs = {k: b.out((M, 3 * N), dt, 3 * N + 8, k) for k in ("ex_stream", "ex_one_phase", "ln_stream", "ln_one_phase")}
        win = {k: _p(v) + N * item for k, v in outs.items()}
        _gemm_ex(12, a, w, bias, M, N, K, dt, _lib.EPI_BIAS_GELU, win["ex_stream"], 3 * N + 8, "window, id 12")
        _gemm_ex(14, a, w, bias, M, N, K, dt, _lib.EPI_BIAS_GELU, win["ex_one_phase"], 3 * N + 8, "window, id 14")
        _lnfold(a, w, bias, rs, cs, M, N, K, dt, _lib.EPI_BIAS, win["ln_stream"], 3 * N + 8, "window, lnfold")
        monkeypatch.setenv(SWITCH, "0")
        _lnfold(a, w, bias, rs, cs, M, N, K, dt, _lib.EPI_BIAS, win["ln_one_phase"], 3 * N + 8, "window, lnfold, switch off")
        monkeypatch.delenv(SWITCH)
        torch.cuda.synchronize()
        for k, v in outs.items():
            outside = torch.cat([v[:, :N], v[:, 2 * N:]], 1).contiguous().view(torch.uint8)
            assert bool((outside == pattern).all()), f"{k}: columns outside the window were written (poison 0x{pattern:02X})"
        return G.Result({k: v[:, N:2 * N] for k, v in outs.items()}, b.handles)

    o = G.run_contract(call)
    assert torch.equal(o["ex_stream"], o["ex_one_phase"])
    assert torch.equal(o["ln_stream"], o["ln_one_phase"])


def test_small_vit_features_equal_with_the_switch_on_and_off(gpu, monkeypatch):
    """A depth-4 ViT whose LayerNorms are folded into the GEMMs (qkv and fc1 are amds_gemm_lnfold consumers, kernel id 12): same feature bits with the
    streamed epilogue and with AMDS_GEMM_EPI_STREAM=0."""
    from stamp_amd.vit import PRESETS, HipViT, random_vit_state_dict

    cfg = PRESETS["test_tiny_fold"]
    sd = random_vit_state_dict(cfg, seed=2)
    tiles = torch.randint(0, 256, (5, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(gpu)
    model = HipViT(cfg, sd, device=gpu, chunk=3)
    assert model.ln_fold
    monkeypatch.delenv(SWITCH, raising=False)
    on = model(tiles)
    monkeypatch.setenv(SWITCH, "0")
    off = model(tiles)
    monkeypatch.delenv(SWITCH)
    assert bool(torch.isfinite(on.float()).all())
    assert torch.equal(on, off)
    assert torch.equal(on, model(tiles))
