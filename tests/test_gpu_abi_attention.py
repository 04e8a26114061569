"""Bands of the attention entry points (family B of the C-ABI contract tests; tests/guarded.py).

The packed qkv tensor sits in front of a poisoned band: the last, partial key tile of the streaming kernels must not read it (their K / V tiles travel by
buffer-form LDS-DMA, which returns 0 for an out-of-range address instead of faulting -- and would return the poison for an in-range one).  Outputs, lse
and the backward's scratch are poisoned everywhere.  Every case runs under 0x00 and 0xFF: bit-identical and finite outputs, untouched bands, and on the
0x00 run the fp64 bar of the kernel's parity test (test_gpu_kernels.py, test_gpu_train.py, test_gpu_mil_seam.py, test_gpu_vit.py, test_gpu_swin.py)."""
import pytest
import torch

import guarded as G
from stamp_amd import _lib, ops
from guarded import Bufs, act_eps as _eps, cur_stream as _st, ptr as _p

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


def _qkv(B, T, H, dt, seed, hd=64, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B * T, 3 * H * hd, generator=g) * scale).to(dt), g


def _sdpa(qkv, B, T, H, hd=64, mult=None):
    """fp64 softmax(q k^T / sqrt(hd)) v on the already rounded operands; `mult`: a [B, H, T, T] factor on the probabilities (dropout)."""
    q, k, v = qkv.double().reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    p = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, -1)
    if mult is not None:
        p = p * mult
    return (p @ v).transpose(1, 2).reshape(B * T, H * hd)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,T,H", [(1, 63, 1), (1, 65, 1), (3, 129, 4), (2, 1025, 8)])
def test_attention(gpu, dt, B, T, H):
    """amds_attention on both sides of the 64-key tile (test_attention_streaming_any_length: 4 ulp of the act dtype)."""
    lib = _lib.lib()
    qkv0, _ = _qkv(B, T, H, dt, B * 77 + T + H)
    ref = _sdpa(qkv0, B, T, H)

    def call(pattern):
        b = Bufs(gpu, pattern)
        qkv, out = b.inp(qkv0, name="qkv"), b.out((B * T, H * 64), dt, name="out")
        _lib.check(lib.amds_attention(_p(qkv), _p(out), B, T, H, ops.act_code(dt), _st()), "attention")
        return b.result(out=out)

    out = G.run_contract(call)["out"].double().cpu()
    assert (out - ref).abs().max().item() < 4 * _eps(dt) * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,T,H,hd", [(2, 257, 2, 64), (3, 261, 2, 64), (1, 33, 1, 64), (1, 257, 2, 80)])
def test_attention_vit_hd(gpu, dt, B, T, H, hd):
    """amds_attention_vit_hd: the T = 257 kernel, the 256 + R pipeline, the small-T kernel and head dim 80 (test_attention_vit / _head_dim_80: 4 ulp)."""
    lib = _lib.lib()
    qkv0, _ = _qkv(B, T, H, dt, B * 1000 + T + H, hd)
    ref = _sdpa(qkv0, B, T, H, hd)

    def call(pattern):
        b = Bufs(gpu, pattern)
        qkv, out = b.inp(qkv0, name="qkv"), b.out((B * T, H * hd), dt, name="out")
        _lib.check(lib.amds_attention_vit_hd(_p(qkv), _p(out), B, T, H, hd, ops.act_code(dt), _st()), "attention_vit_hd")
        return b.result(out=out)

    out = G.run_contract(call)["out"].double().cpu()
    assert (out - ref).abs().max().item() < 4 * _eps(dt) * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_row(gpu, dt):
    """amds_attention_row at (2, 212, 4), q and out at a padded pitch (test_attention_row_is_the_class_tokens_row_of_the_full_attention: 2 ulp)."""
    lib, (B, T, H) = _lib.lib(), (2, 212, 4)
    D = H * 64
    qkv0, g = _qkv(B, T, H, dt, B * 100 + T + H)
    q0 = (torch.randn(B, D, generator=g) * 1.5).to(dt)
    k, v = (qkv0.double().reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)[i] for i in (1, 2))
    qq = q0.double().reshape(B, H, 1, 64)
    ref = (torch.softmax(qq @ k.transpose(-1, -2) / 8.0, -1) @ v).reshape(B, D)

    def call(pattern):
        b = Bufs(gpu, pattern)
        q, qkv, out = b.inp(q0, D + 8, "q"), b.inp(qkv0, name="qkv"), b.out((B, D), dt, D + 8, "out")
        _lib.check(lib.amds_attention_row(_p(q), D + 8, _p(qkv), _p(out), D + 8, B, T, H, ops.act_code(dt), _st()), "attention_row")
        return b.result(out=out)

    out = G.run_contract(call)["out"].double().cpu()
    assert (out - ref).abs().max().item() < 2 * _eps(dt) * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T,H,hd", [(257, 16, 64), (50, 2, 64), (261, 16, 80)])
def test_attention_cls_f32(gpu, dt, T, H, hd):
    """amds_attention_cls_f32, q and out at a padded pitch (test_attention_cls_f32_matches_fp64: 2e-6 relative L2)."""
    lib, B, D = _lib.lib(), 5, H * hd
    qkv0, g = _qkv(B, T, H, dt, T + hd, hd, scale=1.0)
    q0 = torch.randn(B, D, generator=g)
    q0[1] *= 6.0
    k = qkv0[:, D:2 * D].double().reshape(B, T, H, hd)
    v = qkv0[:, 2 * D:].double().reshape(B, T, H, hd)
    s = torch.einsum("bhd,bthd->bht", q0.double().reshape(B, H, hd), k) / hd ** 0.5
    ref = torch.einsum("bht,bthd->bhd", torch.softmax(s, -1), v).reshape(B, D)

    def call(pattern):
        b = Bufs(gpu, pattern)
        q, qkv, out = b.inp(q0, D + 8, "q"), b.inp(qkv0, name="qkv"), b.out((B, D), torch.float32, D + 8, "out")
        _lib.check(lib.amds_attention_cls_f32(_p(q), D + 8, _p(qkv), _p(out), D + 8, B, T, H, hd, ops.act_code(dt), _st()), "attention_cls_f32")
        return b.result(out=out)

    out = G.run_contract(call)["out"].double().cpu()
    assert ((out - ref).norm() / ref.norm()).item() < 2e-6


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("B,T,H", [(1, 65, 1), (2, 129, 3), (2, 1025, 8)])
def test_attention_train_forward_backward(gpu, dt, p, B, T, H):
    """p = 0: amds_attention_fwd_lse / _bwd; p = 0.25: amds_attention_fwd_train / _bwd_train with the mask the kernels regenerate (test_attention_backward_vs_autograd,
    test_attention_dropout_fwd_bwd_vs_autograd: forward 4 ulp, lse 1e-2, backward 8 ulp against fp64 autograd).  lse, the backward's fp32 scratch and dqkv are
    poisoned on entry."""
    lib, D, seed, sid = _lib.lib(), H * 64, 4242, 21
    qkv0, g = _qkv(B, T, H, dt, B * 100 + T + H, scale=1.0)
    dout0 = torch.randn(B * T, D, generator=g).to(dt)
    mult = None
    if p > 0:
        m = torch.empty(B, H, T, T, dtype=torch.uint8, device=gpu)
        _lib.check(lib.amds_attention_dropout_mask(_p(m), B, H, T, p, seed, sid, _st()), "mask")
        mult = m.cpu().double() * lib.amds_dropout_keep_scale(p)
    x = qkv0.double().requires_grad_(True)
    o = _sdpa(x, B, T, H, mult=mult)
    o.backward(dout0.double())
    q, k = (qkv0.double().reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)[i] for i in (0, 1))
    lref = torch.logsumexp(q @ k.transpose(-1, -2) / 8.0, -1) / torch.log(torch.tensor(2.0, dtype=torch.float64))

    def call(pattern):
        b = Bufs(gpu, pattern)
        qkv, dout = b.inp(qkv0, name="qkv"), b.inp(dout0, name="dout")
        out, lse = b.out((B * T, D), dt, name="out"), b.out((B, H, T), torch.float32, name="lse")
        ws, dqkv = b.out((B, H, T), torch.float32, name="dq_sum_ws"), b.out((B * T, 3 * D), dt, name="dqkv")
        if p > 0:
            _lib.check(lib.amds_attention_fwd_train(_p(qkv), _p(out), _p(lse), B, T, H, ops.act_code(dt), p, seed, sid, _st()), "fwd_train")
            _lib.check(lib.amds_attention_bwd_train(_p(qkv), _p(out), _p(dout), _p(lse), _p(ws), _p(dqkv), B, T, H, ops.act_code(dt), p, seed, sid, _st()), "bwd_train")
        else:
            _lib.check(lib.amds_attention_fwd_lse(_p(qkv), _p(out), _p(lse), B, T, H, ops.act_code(dt), _st()), "fwd_lse")
            _lib.check(lib.amds_attention_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(ws), _p(dqkv), B, T, H, ops.act_code(dt), _st()), "bwd")
        return b.result(out=out, lse=lse, dqkv=dqkv)

    r = {k_: v.double().cpu() for k_, v in G.run_contract(call).items()}
    eps = _eps(dt)
    assert (r["out"] - o.detach()).abs().max().item() < 4 * eps * max(1.0, o.abs().max().item())
    assert (r["lse"] - lref).abs().max().item() < 1e-2
    assert (r["dqkv"] - x.grad).abs().max().item() < 8 * eps * max(1.0, x.grad.abs().max().item())


@pytest.mark.parametrize("B,T,H", [(3, 5, 2), (1, 65, 1)])
def test_attention_alibi_train_forward_backward(gpu, B, T, H):
    """amds_attention_alibi_fwd_train / _bwd (test_alibi_attention_fwd_bwd_vs_autograd: forward 8e-3 relative L2, dq / dk / dv 1.5e-2, d bias_scale 3e-2)."""
    lib, D = _lib.lib(), H * 64
    g = torch.Generator().manual_seed(B * T)
    qkv0 = (torch.randn(B * T, 3 * D, generator=g) * 0.8).bfloat16()
    coords0 = torch.rand(B, T, 2, generator=g) * 4000.0
    coords0[:, 0] = 0.0
    bs0, rm = torch.rand(H, generator=g) * 0.5 + 0.1, torch.rand(H, generator=g) * 500.0 + 1800.0
    dout0 = (torch.randn(B * T, D, generator=g) * 0.5).bfloat16()
    q3 = qkv0.double().reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)
    bsd = bs0.double().clone().requires_grad_(True)
    dist = torch.cdist(coords0.double(), coords0.double())
    w = torch.softmax(q3[0] @ q3[1].transpose(-2, -1) / 8.0, -1) - (dist[:, None] / rm.double().view(1, H, 1, 1)) * bsd.view(1, H, 1, 1)
    ref = (w @ q3[2]).permute(0, 2, 1, 3).reshape(B * T, D)
    ref.backward(dout0.double())
    ref_dqkv = q3.grad.permute(1, 3, 0, 2, 4).reshape(B * T, 3, D)

    def call(pattern):
        b = Bufs(gpu, pattern)
        qkv, coords, dout = b.inp(qkv0, name="qkv"), b.inp(coords0.reshape(B * T, 2), name="coords"), b.inp(dout0, name="dout")
        inv_rm, bs, ds = b.inp(1.0 / rm, name="inv_rm"), b.inp(bs0, name="bias_scale"), b.inp(bs0 / rm, name="dist_scale")
        out, u, osm = (b.out((B * T, D), torch.bfloat16, name=n) for n in ("out", "u", "osm"))
        lse, ws, part = (b.out((B, H, T), torch.float32, name=n) for n in ("lse", "dq_sum_ws", "dbs_part"))
        dqkv = b.out((B * T, 3 * D), torch.bfloat16, name="dqkv")
        _lib.check(lib.amds_attention_alibi_fwd_train(_p(qkv), _p(coords), _p(inv_rm), _p(bs), _p(out), _p(u), _p(osm), _p(lse), B, T, H, _lib.BF16, _st()), "alibi fwd")
        _lib.check(lib.amds_attention_alibi_bwd(_p(qkv), _p(osm), _p(u), _p(dout), _p(lse), _p(coords), _p(bs), _p(ds), _p(ws), _p(part), _p(dqkv), B, T, H, _st()),
                   "alibi bwd")
        return b.result(out=out, dqkv=dqkv, dbs_part=part)

    r = {k_: v.double().cpu() for k_, v in G.run_contract(call).items()}
    rel = lambda a, c: ((a - c).norm() / (c.norm() + 1e-30)).item()  # noqa: E731
    assert rel(r["out"], ref.detach()) < 8e-3
    d = r["dqkv"].reshape(B * T, 3, D)
    for i in range(3):
        assert rel(d[:, i], ref_dqkv[:, i]) < 1.5e-2, i
    assert rel(r["dbs_part"].sum((0, 2)), bsd.grad) < 3e-2


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_attention_row_train_forms(gpu, dt, p):
    """amds_attention_row_fwd_train / _bwd_train at (2, 129, 3), query row 0: only row qrow of every bag of out / lse is declared (the header: the other rows are
    not touched -- they keep the poison, which the bands' check does not mind and the backward must not read); dqkv is complete.  The forward's row against fp64
    with the regenerated mask (4 ulp, the full kernel's bar for that row), the backward against fp64 autograd of that row alone (8 ulp)."""
    lib, (B, T, H), seed, sid = _lib.lib(), (2, 129, 3), 99, 11
    D = H * 64
    qkv0, g = _qkv(B, T, H, dt, 7, scale=1.0)
    dout0 = torch.randn(B * T, D, generator=g).to(dt)
    mult = None
    if p > 0:
        m = torch.empty(B, H, T, T, dtype=torch.uint8, device=gpu)
        _lib.check(lib.amds_attention_dropout_mask(_p(m), B, H, T, p, seed, sid, _st()), "mask")
        mult = m.cpu().double() * lib.amds_dropout_keep_scale(p)
    x = qkv0.double().requires_grad_(True)
    o = _sdpa(x, B, T, H, mult=mult).reshape(B, T, D)[:, 0]
    o.backward(dout0.double().reshape(B, T, D)[:, 0])

    def call(pattern):
        b = Bufs(gpu, pattern)
        qkv, dout = b.inp(qkv0, name="qkv"), b.out((B * T, D), dt, name="dout")
        dout.view(B, T, D)[:, 0] = dout0.to(gpu).view(B, T, D)[:, 0]                 # only the query rows of dout are read: the rest stays poisoned
        out, lse, dqkv = b.out((B * T, D), dt, name="out"), b.out((B, H, T), torch.float32, name="lse"), b.out((B * T, 3 * D), dt, name="dqkv")
        _lib.check(lib.amds_attention_row_fwd_train(_p(qkv), _p(out), _p(lse), B, T, H, 0, ops.act_code(dt), p, seed, sid, _st()), "row_fwd_train")
        _lib.check(lib.amds_attention_row_bwd_train(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), B, T, H, 0, ops.act_code(dt), p, seed, sid, _st()), "row_bwd_train")
        return b.result(out_row=out.view(B, T, D)[:, 0], lse_row=lse[:, :, 0], dqkv=dqkv)

    r = {k_: v.double().cpu() for k_, v in G.run_contract(call).items()}
    assert (r["out_row"] - o.detach()).abs().max().item() < 4 * _eps(dt) * max(1.0, o.abs().max().item())
    assert (r["dqkv"] - x.grad).abs().max().item() < 8 * _eps(dt) * max(1.0, x.grad.abs().max().item())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,T,H", [(2, 129, 3), (3, 65, 1)])
def test_attention_row_alibi_train_forms(gpu, dt, B, T, H):
    """amds_attention_row_alibi_fwd_train / _bwd_train, query row 0 (the class token at (0, 0)): out_0 = sum_k (p_k - bias_scale_h |c_0 - c_k| / running_mean_h) v_k.  Only
    row qrow of every bag of out / u / osm / lse is declared, the rest keeps the poison, and so do the rows of dout the backward does not read; dqkv is complete, dbs is
    [B][H].  Against fp64 autograd of that row alone, the bars of test_mil_vit_train_alibi_class_row_tail_equals_the_full_last_block: 8e-3 relative L2 (out, dq / dk / dv),
    1.6e-2 for the bias_scale vector."""
    lib, D = _lib.lib(), H * 64
    qkv0, g = _qkv(B, T, H, dt, B * T + 11, scale=0.8)
    coords0 = torch.rand(B, T, 2, generator=g) * 4000.0
    coords0[:, 0] = 0.0
    bs0, rm = torch.rand(H, generator=g) * 0.5 + 0.1, torch.rand(H, generator=g) * 500.0 + 1800.0
    dout0 = (torch.randn(B * T, D, generator=g) * 0.5).to(dt)
    q3 = qkv0.double().reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)
    bsd = bs0.double().clone().requires_grad_(True)
    dist0 = coords0.double().norm(dim=-1)                                               # |c_0 - c_k| with the class token at the origin, [B, T]
    w = torch.softmax(q3[0][:, :, :1] @ q3[1].transpose(-2, -1) / 8.0, -1) - (dist0[:, None, None, :] / rm.double().view(1, H, 1, 1)) * bsd.view(1, H, 1, 1)
    ref = (w @ q3[2]).reshape(B, D)
    ref.backward(dout0.double().reshape(B, T, D)[:, 0])
    ref_dqkv = q3.grad.permute(1, 3, 0, 2, 4).reshape(B * T, 3, D)

    def call(pattern):
        b = Bufs(gpu, pattern)
        qkv, coords = b.inp(qkv0, name="qkv"), b.inp(coords0.reshape(B * T, 2), name="coords")
        inv_rm, bs = b.inp(1.0 / rm, name="inv_rm"), b.inp(bs0, name="bias_scale")
        dout = b.out((B * T, D), dt, name="dout")
        dout.view(B, T, D)[:, 0] = dout0.to(gpu).view(B, T, D)[:, 0]
        out, u, osm = (b.out((B * T, D), dt, name=n) for n in ("out", "u", "osm"))
        lse, dqkv, dbs = b.out((B, H, T), torch.float32, name="lse"), b.out((B * T, 3 * D), dt, name="dqkv"), b.out((B, H), torch.float32, name="dbs")
        _lib.check(lib.amds_attention_row_alibi_fwd_train(_p(qkv), _p(coords), _p(inv_rm), _p(bs), _p(out), _p(u), _p(osm), _p(lse), B, T, H, 0, ops.act_code(dt), _st()), "fwd")
        _lib.check(lib.amds_attention_row_alibi_bwd_train(_p(qkv), _p(osm), _p(u), _p(dout), _p(lse), _p(coords), _p(bs), _p(inv_rm), _p(dqkv), _p(dbs), B, T, H, 0,
                                                          ops.act_code(dt), _st()), "bwd")
        return b.result(out_row=out.view(B, T, D)[:, 0], u_row=u.view(B, T, D)[:, 0], osm_row=osm.view(B, T, D)[:, 0], lse_row=lse[:, :, 0], dqkv=dqkv, dbs=dbs)

    r = {k_: v.double().cpu() for k_, v in G.run_contract(call).items()}
    rel = lambda x, y: ((x - y).norm() / (y.norm() + 1e-30)).item()  # noqa: E731
    assert rel(r["out_row"], ref.detach()) < 8e-3
    d = r["dqkv"].reshape(B * T, 3, D)
    for i in range(3):
        assert rel(d[:, i], ref_dqkv[:, i]) < 8e-3, i
    assert rel(r["dbs"].sum(0), bsd.grad) < 1.6e-2


_BIG_T = 16384          # row kernels: LDS (T + 1032) * 4 = 69 664 bytes, ALiBi row forward (2 T + 2056) * 4 = 139 296: past the 64 KB a kernel gets without an opt-in
_big_mask_row = {}


def _big_mask_row0(gpu, p, seed, sid):
    """Row 0 of the [1, 1, T, T] attention dropout mask at _BIG_T (the whole tensor is written on the device, 268 MB of u8; one row comes back), once per rate."""
    if p not in _big_mask_row:
        m = torch.empty(1, 1, _BIG_T, _BIG_T, dtype=torch.uint8, device=gpu)
        _lib.check(_lib.lib().amds_attention_dropout_mask(_p(m), 1, 1, _BIG_T, p, seed, sid, _st()), "mask")
        _big_mask_row[p] = m[0, 0, 0].cpu().double() * _lib.lib().amds_dropout_keep_scale(p)
        del m
    return _big_mask_row[p]


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_row_forms_past_64k_of_lds(gpu, dt):
    """The one-query kernels at B = 1, H = 1, T = 16384, where their dynamic LDS request passes 64 KB and the launch depends on the per-device opt-in:
    amds_attention_row_varlen with one bag of 16 383 tiles bit-equal to amds_attention_row on the same rows; amds_attention_row_fwd_train / _bwd_train at p = 0 and
    0.25; amds_attention_row_alibi_fwd_train / _bwd_train.  Reference: fp64 autograd of the ONE row, softmax(q_0 K^T / 8) times the regenerated mask row, then @ V
    (the full T x T product would be 2 GB of doubles).  Bars of the small-shape tests above: 4 ulp forward row, 8 ulp dqkv; ALiBi 8e-3 / 1.6e-2 relative L2."""
    lib, T, seed, sid = _lib.lib(), _BIG_T, 99, 11
    D, code = 64, ops.act_code(dt)
    qkv0, g = _qkv(1, T, 1, dt, 16384 + 7, scale=1.0)
    dout_row = torch.randn(D, generator=g).to(dt)

    # ---- ragged form == fixed-pitch form, bit for bit
    offs0 = torch.tensor([0, T - 1], dtype=torch.int32)
    need = lib.amds_attention_varlen_workspace_bytes(1, T - 1)

    def call_varlen(pattern):
        b = Bufs(gpu, pattern)
        qkv, offs, ws = b.inp(qkv0, name="qkv"), b.inp(offs0, name="offsets"), b.out((need,), torch.uint8, name="ws")
        q = b.inp(qkv0[:1, :D], D + 8, "q")
        o_var, o_row = b.out((1, D), dt, D + 8, name="out varlen"), b.out((1, D), dt, D + 8, name="out row")
        _lib.check(lib.amds_attention_row_varlen(_p(q), D + 8, _p(qkv), _p(offs), _p(o_var), D + 8, 1, T - 1, T - 1, 1, code, _p(ws), need, _st()), "row_varlen")
        _lib.check(lib.amds_attention_row(_p(q), D + 8, _p(qkv), _p(o_row), D + 8, 1, T, 1, code, _st()), "row")
        return b.result(varlen=o_var, row=o_row)

    r = G.run_contract(call_varlen)
    assert torch.equal(r["varlen"], r["row"])
    print(f"big-LDS row forms {dt}:", end=" ")

    def row_ref(mult):
        x = qkv0.double().requires_grad_(True)
        w = torch.softmax(x[:1, :D] @ x[:, D:2 * D].T / 8.0, -1)
        o = ((w if mult is None else w * mult) @ x[:, 2 * D:]).reshape(D)
        o.backward(dout_row.double())
        return o.detach(), x.grad

    o0, _ = row_ref(None)
    err = (r["row"].double().cpu().reshape(D) - o0).abs().max().item()
    print(f"row fwd {err / _eps(dt):.3f} ulp", end="; ")
    assert err < 4 * _eps(dt) * max(1.0, o0.abs().max().item())

    # ---- training forms, without and with dropout
    for p in (0.0, 0.25):
        o, dref = row_ref(_big_mask_row0(gpu, p, seed, sid) if p > 0 else None)

        def call_train(pattern):
            b = Bufs(gpu, pattern)
            qkv, dout = b.inp(qkv0, name="qkv"), b.out((T, D), dt, name="dout")
            dout[0] = dout_row.to(gpu)                                                   # only the query row of dout is read: the rest stays poisoned
            out, lse, dqkv = b.out((T, D), dt, name="out"), b.out((1, 1, T), torch.float32, name="lse"), b.out((T, 3 * D), dt, name="dqkv")
            _lib.check(lib.amds_attention_row_fwd_train(_p(qkv), _p(out), _p(lse), 1, T, 1, 0, code, p, seed, sid, _st()), "row_fwd_train")
            _lib.check(lib.amds_attention_row_bwd_train(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), 1, T, 1, 0, code, p, seed, sid, _st()), "row_bwd_train")
            return b.result(out_row=out[0], lse_row=lse[:, :, 0], dqkv=dqkv)

        rt = {k_: v.double().cpu() for k_, v in G.run_contract(call_train).items()}
        ef, eb = (rt["out_row"] - o).abs().max().item(), (rt["dqkv"] - dref).abs().max().item()
        print(f"p={p}: fwd {ef / _eps(dt):.3f} ulp, dqkv {eb / (_eps(dt) * max(1.0, dref.abs().max().item())):.3f} ulp", end="; ")
        assert ef < 4 * _eps(dt) * max(1.0, o.abs().max().item())
        assert eb < 8 * _eps(dt) * max(1.0, dref.abs().max().item())

    # ---- ALiBi row forms (the class token at the origin)
    qa0, g = _qkv(1, T, 1, dt, 16384 + 11, scale=0.8)
    coords0 = torch.rand(T, 2, generator=g) * 4000.0
    coords0[0] = 0.0
    bs0, rm = torch.rand(1, generator=g) * 0.5 + 0.1, torch.rand(1, generator=g) * 500.0 + 1800.0
    da_row = (torch.randn(D, generator=g) * 0.5).to(dt)
    x = qa0.double().requires_grad_(True)
    bsd = bs0.double().clone().requires_grad_(True)
    w = torch.softmax(x[:1, :D] @ x[:, D:2 * D].T / 8.0, -1) - (coords0.double().norm(dim=-1)[None, :] / rm.double()) * bsd
    ref = (w @ x[:, 2 * D:]).reshape(D)
    ref.backward(da_row.double())

    def call_alibi(pattern):
        b = Bufs(gpu, pattern)
        qkv, coords = b.inp(qa0, name="qkv"), b.inp(coords0, name="coords")
        inv_rm, bs = b.inp(1.0 / rm, name="inv_rm"), b.inp(bs0, name="bias_scale")
        dout = b.out((T, D), dt, name="dout")
        dout[0] = da_row.to(gpu)
        out, u, osm = (b.out((T, D), dt, name=n) for n in ("out", "u", "osm"))
        lse, dqkv, dbs = b.out((1, 1, T), torch.float32, name="lse"), b.out((T, 3 * D), dt, name="dqkv"), b.out((1, 1), torch.float32, name="dbs")
        _lib.check(lib.amds_attention_row_alibi_fwd_train(_p(qkv), _p(coords), _p(inv_rm), _p(bs), _p(out), _p(u), _p(osm), _p(lse), 1, T, 1, 0, code, _st()), "fwd")
        _lib.check(lib.amds_attention_row_alibi_bwd_train(_p(qkv), _p(osm), _p(u), _p(dout), _p(lse), _p(coords), _p(bs), _p(inv_rm), _p(dqkv), _p(dbs), 1, T, 1, 0, code,
                                                          _st()), "bwd")
        return b.result(out_row=out[0], u_row=u[0], osm_row=osm[0], lse_row=lse[:, :, 0], dqkv=dqkv, dbs=dbs)

    ra = {k_: v.double().cpu() for k_, v in G.run_contract(call_alibi).items()}
    rel = lambda a, c: ((a - c).norm() / (c.norm() + 1e-30)).item()  # noqa: E731
    d3, g3 = ra["dqkv"].reshape(T, 3, D), x.grad.reshape(T, 3, D)
    rels = [rel(ra["out_row"], ref.detach())] + [rel(d3[:, i], g3[:, i]) for i in range(3)] + [rel(ra["dbs"].sum(0), bsd.grad)]
    print("alibi rel L2 out / dq / dk / dv / dbs " + " ".join(f"{v:.2e}" for v in rels))
    assert rels[0] < 8e-3
    for i in range(3):
        assert rels[1 + i] < 8e-3, i
    assert rels[4] < 1.6e-2


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_masked(gpu, dt):
    """amds_attention_masked at (3, 129, 4), mask_heads 3 (one zero-padded head): blocked(q, k) = (pad[q] & pad[k]) | (q > 0 & k == 0) with the pad row of bag
    (b * mask_heads + h) % B, restated from the header in fp64; the streaming kernel's bar (4 ulp): same kernel family, same roundings."""
    lib, (B, T, H, MH) = _lib.lib(), (3, 129, 4, 3)
    D = H * 64
    qkv0, g = _qkv(B, T, H, dt, 31)
    qkv0.view(B * T, 3, H, 64)[:, :, MH:] = 0                                        # heads past mask_heads are zero padding
    pad0 = (torch.rand(B, T, generator=g) > 0.5).to(torch.uint8)
    pad0[:, 0] = 0
    q, k, v = qkv0.double().reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    idx = (torch.arange(B)[:, None] * MH + torch.arange(H)[None, :]) % B
    pr = pad0.bool()[idx]                                                            # [B, H, T]
    blocked = (pr[..., :, None] & pr[..., None, :])
    blocked[..., 1:, 0] = True
    ref = (torch.softmax(s.masked_fill(blocked, float("-inf")), -1) @ v).transpose(1, 2).reshape(B * T, D)[:, :MH * 64]

    def call(pattern):
        b = Bufs(gpu, pattern)
        qkv, pad, out = b.inp(qkv0, name="qkv"), b.inp(pad0, name="pad"), b.out((B * T, D), dt, name="out")
        _lib.check(lib.amds_attention_masked(_p(qkv), _p(pad), _p(out), B, T, H, MH, ops.act_code(dt), _st()), "attention_masked")
        return b.result(out=out)

    out = G.run_contract(call)["out"].double().cpu()
    assert (out[:, :MH * 64] - ref).abs().max().item() < 4 * _eps(dt) * max(1.0, ref.abs().max().item())
    assert bool((out[:, MH * 64:] == 0).all())


def test_attention_varlen_forms(gpu):
    """The three varlen entries with offsets [0, 1, 78, 378] (token rows 2, 78, 301): every bag against fp64 on its own rows (the fixed-pitch kernels' bars: 4 ulp,
    ALiBi 8e-3 relative L2, the row form 2 ulp); the per-call table lives in a poisoned workspace of exactly the requested size."""
    lib, H, dt = _lib.lib(), 4, torch.float16
    tiles = [1, 77, 300]
    n, total, mx = len(tiles), sum(tiles), max(tiles)
    M, D = total + n, H * 64
    g = torch.Generator().manual_seed(9)
    qkv0 = (torch.randn(M, 3 * D, generator=g) * 0.5).half()
    coords0, hs0 = torch.rand(M, 2, generator=g) * 1000, torch.rand(H, generator=g) * 1e-3
    q0 = (torch.randn(n, D, generator=g) * 0.5).half()
    offs0 = torch.tensor([0, 1, 78, 378], dtype=torch.int32)
    need = lib.amds_attention_varlen_workspace_bytes(n, total)

    def call(pattern):
        b = Bufs(gpu, pattern)
        qkv, coords, hs, q, offs = b.inp(qkv0, name="qkv"), b.inp(coords0, name="coords"), b.inp(hs0, name="head_scale"), b.inp(q0, D + 8, "q"), b.inp(offs0, name="offsets")
        outs = {}
        for name in ("plain", "alibi", "row"):
            ws = b.out((need,), torch.uint8, name=f"ws {name}")
            if name == "plain":
                o = b.out((M, D), dt, name="out")
                rc = lib.amds_attention_varlen(_p(qkv), _p(offs), _p(o), n, total, mx, H, _lib.F16, _p(ws), need, _st())
            elif name == "alibi":
                o = b.out((M, D), torch.bfloat16, name="out alibi")
                rc = lib.amds_attention_alibi_varlen(_p(qkv), _p(coords), _p(hs), _p(offs), _p(o), n, total, mx, H, _lib.F16, _p(ws), need, _st())
            else:
                o = b.out((n, D), dt, D + 8, name="out row")
                rc = lib.amds_attention_row_varlen(_p(q), D + 8, _p(qkv), _p(offs), _p(o), D + 8, n, total, mx, H, _lib.F16, _p(ws), need, _st())
            _lib.check(rc, name)
            outs[name] = o
        return b.result(**outs)

    r = {k_: v.double().cpu() for k_, v in G.run_contract(call).items()}
    for i, t in enumerate(tiles):
        r0, T = int(offs0[i]) + i, t + 1
        sl = qkv0[r0:r0 + T]
        ref = _sdpa(sl, 1, T, H)
        assert (r["plain"][r0:r0 + T] - ref).abs().max().item() < 4 * _eps(dt) * max(1.0, ref.abs().max().item()), i
        _, k, v = sl.double().reshape(1, T, 3, H, 64).permute(2, 0, 3, 1, 4)
        dist = torch.cdist(coords0[r0:r0 + T].double(), coords0[r0:r0 + T].double())
        refa = ref - ((hs0.double().view(1, H, 1, 1) * dist[None, None]) @ v).transpose(1, 2).reshape(T, D)
        assert ((r["alibi"][r0:r0 + T] - refa).norm() / refa.norm()).item() < 8e-3, i
        refr = (torch.softmax(q0[i].double().reshape(1, H, 1, 64) @ k.transpose(-1, -2) / 8.0, -1) @ v).reshape(D)
        assert (r["row"][i] - refr).abs().max().item() < 2 * _eps(dt) * max(1.0, refr.abs().max().item()), i


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("grid,heads,shift", [(14, 12, 3), (7, 24, 0), (14, 12, 0)])
def test_window_attention(gpu, dt, grid, heads, shift):
    """amds_window_attention at grids 14 and 7, qkv and out at padded pitches (test_window_attention: 2e-3 / 1.2e-2 relative L2)."""
    from stamp_amd.swin import rel_bias_lane_table, shift_mask_bits
    from test_gpu_swin import _window_attention_ref
    lib, B, dim = _lib.lib(), 2, heads * 32
    g = torch.Generator().manual_seed(grid * 10 + shift)
    qkv0 = (torch.randn(B * grid * grid, 3 * dim, generator=g) * 1.5).to(dt)
    table = torch.randn(169, heads, generator=g)
    ref = _window_attention_ref(qkv0.float(), table, B, grid, heads, shift)
    lane0, bits0 = rel_bias_lane_table(table), shift_mask_bits()
    for pad in (0, 8):
        def call(pattern):
            b = Bufs(gpu, pattern)
            qkv, lane, bits = b.inp(qkv0, 3 * dim + pad, "qkv"), b.inp(lane0, name="bias_lane"), b.inp(bits0, name="mask_bits")
            out = b.out((B * grid * grid, dim), dt, dim + pad, "out")
            _lib.check(lib.amds_window_attention(_p(qkv), 3 * dim + pad, _p(out), dim + pad, _p(lane), _p(bits), B, grid, dim, heads, shift, ops.act_code(dt), _st()), "window")
            return b.result(out=out)

        out = G.run_contract(call)["out"].double().cpu()
        assert ((out - ref).norm() / ref.norm()).item() < (2e-3 if dt == torch.float16 else 1.2e-2), pad


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,T,H", [(1, 65, 1), (3, 129, 2)])
def test_attention_alibi_inference_forms(gpu, masked, B, T, H):
    """amds_attention_alibi and amds_attention_alibi_masked (the header's statement of vision_tranformer.py:62-70, :363-372 in fp64: softmax over all keys, blocked
    products (pad[q] & pad[k]) | (q > 0 & k == 0) zeroed afterwards, no distance term on the class token's row and column); bf16 output, the ALiBi forward's bar
    (8e-3 relative L2, test_alibi_attention_fwd_bwd_vs_autograd)."""
    lib, D, dt = _lib.lib(), H * 64, torch.float16
    qkv0, g = _qkv(B, T, H, dt, B * T + 3, scale=0.8)
    coords0 = torch.rand(B, T, 2, generator=g) * 4000.0
    coords0[:, 0] = 0.0
    hs0 = (torch.rand(H, generator=g) * 0.5 + 0.1) / (torch.rand(H, generator=g) * 500.0 + 1800.0)
    pad0 = (torch.rand(B, T, generator=g) > 0.5).to(torch.uint8)
    pad0[:, 0] = 0
    q, k, v = qkv0.double().reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    dist = torch.cdist(coords0.double(), coords0.double())[:, None] * hs0.double().view(1, H, 1, 1)
    w = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
    if masked:
        dist[..., 0, :] = 0
        dist[..., :, 0] = 0
        pr = pad0.bool()[:, None]
        blocked = (pr[..., :, None] & pr[..., None, :]).expand(B, H, T, T).clone()
        blocked[..., 1:, 0] = True
        w = (w - dist).masked_fill(blocked, 0.0)
    else:
        w = w - dist
    ref = (w @ v).transpose(1, 2).reshape(B * T, D)

    def call(pattern):
        b = Bufs(gpu, pattern)
        qkv, coords, hs, out = b.inp(qkv0, name="qkv"), b.inp(coords0.reshape(B * T, 2), name="coords"), b.inp(hs0, name="head_scale"), b.out((B * T, D), torch.bfloat16, name="out")
        if masked:
            pad = b.inp(pad0, name="pad")
            rc = lib.amds_attention_alibi_masked(_p(qkv), _p(coords), _p(hs), _p(pad), _p(out), B, T, H, _lib.F16, _st())
        else:
            rc = lib.amds_attention_alibi(_p(qkv), _p(coords), _p(hs), _p(out), B, T, H, _lib.F16, _st())
        _lib.check(rc, "alibi")
        return b.result(out=out)

    out = G.run_contract(call)["out"].double().cpu()
    assert ((out - ref).norm() / ref.norm()).item() < 8e-3
