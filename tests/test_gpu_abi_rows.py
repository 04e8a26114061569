"""Bands and pitch of the row kernels (family B of the C-ABI contract tests; tests/guarded.py): LayerNorm and its training forms, column sums, transposes,
the element-wise dropout sites, TransMIL's small kernels, gathers and pools.  Inputs carry the poison byte in their bands and pitch padding, outputs and
workspaces everywhere; every case runs under 0x00 and 0xFF (bit-identical, finite, bands untouched) and the 0x00 run meets an fp64 bar.

Bars: where a kernel has a parity test of its own its bar is restated (named in the docstring).  The fp32 kernels that are only reached through the
whole-model chains have none; theirs is the rounding bound of the arithmetic the header states, computed from the REFERENCE's operands: a sum of n fp32 terms
evaluated in any order is within n * 2^-23 * sum|terms| of the exact sum (`_sum_bar`), a single fp32 result within 2^-23 of its magnitude, a value rounded once
to bf16 within 2^-8 of its magnitude.

The kernels of train.hip and dropout.hip (LayerNorm training forms, column sums, transposes, the dropout sites) are held to per-element bars, on every launch and
with masks from an independent restatement of the rule, by tests/test_gpu_train_rows.py; the tensor-wide bars restated below stay as this file's contract check."""
import ctypes as C

import pytest
import torch

import guarded as G
from stamp_amd import _lib, ops
from guarded import Bufs, act_eps as _eps, cur_stream as _st, ptr as _p

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _sum_bar(n_terms, abs_sum):
    return (n_terms + 2) * 2.0 ** -23 * float(abs_sum)


def _run(gpu, body):
    """body(b: Bufs) -> dict of outputs; -> the 0x00 run's outputs on the CPU."""
    def call(pattern):
        b = Bufs(gpu, pattern)
        return b.result(**body(b))
    return {k: v.cpu() for k, v in G.run_contract(call).items()}


def _mask(gpu, n, p, seed, sid):
    m = torch.empty(n, dtype=torch.uint8, device=gpu)
    _lib.check(_lib.lib().amds_dropout_mask(_p(m), n, p, seed, sid, _st()), "dropout_mask")
    return m.cpu().double() * _lib.lib().amds_dropout_keep_scale(p)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odt", [torch.float16, torch.bfloat16, F32])
@pytest.mark.parametrize("rows,cols,stride", [(33, 1280, 1288), (257, 1024, 1024), (5, 128, 7 * 128), (3, 8192, 8192)])
def test_layernorm(gpu, odt, rows, cols, stride):
    """amds_layernorm with a row stride above the width, and in the class-row form (5 rows, stride T * D = 7 * 128: the rows between are other tokens, poisoned
    here) (test_layernorm: one ulp of the act dtype, 1.6e-5 for fp32, of the range)."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(rows * 7 + cols)
    x0, w0, b0 = torch.randn(rows, cols, generator=g) * 3 + 1.5, 1 + 0.3 * torch.randn(cols, generator=g), 0.2 * torch.randn(cols, generator=g)
    ref = torch.nn.functional.layer_norm(x0.double(), (cols,), w0.double(), b0.double(), 1e-6)

    def body(b):
        x, w, bb = b.inp(x0, stride, "x"), b.inp(w0, name="gamma"), b.inp(b0, name="beta")
        y = b.out((rows, cols), odt, cols + 8, "y")
        _lib.check(lib.amds_layernorm(_p(x), stride, _p(w), _p(bb), _p(y), cols + 8, rows, cols, 1e-6, ops._DT[odt], _st()), "layernorm")
        return dict(y=y)

    y = _run(gpu, body)["y"].double()
    assert (y - ref).abs().max().item() / ref.abs().max().item() < (2e-6 * 8 if odt == F32 else _eps(odt))


@pytest.mark.parametrize("rows,cols,pad,p", [(70, 128, 8, 0.25), (1025, 512, 0, 0.0), (333, 256, 64, 0.5)])
def test_layernorm_training_forms(gpu, rows, cols, pad, p):
    """amds_layernorm_train / _train_copy, amds_layernorm_bwd / _bwd_cast / _bwd_partials on pitched rows (test_layernorm_train_and_bwd: y 1e-5, dx 2e-5, parameter
    gradients 1e-3 of their range; the 16-bit copy of dx: the dropout site's multiplier times dx, rounded once to bf16).  Per-element bars for y, mean, rstd, dx, the
    parameter gradients and the copy: tests/test_gpu_train_rows.py::test_layernorm_train / test_layernorm_bwd."""
    lib, ld, seed, sid = _lib.lib(), cols + pad, 77, 13
    g = torch.Generator().manual_seed(rows)
    x0 = torch.randn(rows, cols, generator=g) * 2 + 0.5
    gamma0, beta0 = 1 + 0.2 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)
    dy0, skip0 = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    xd, gd, bd = x0.double().requires_grad_(True), gamma0.double().requires_grad_(True), beta0.double().requires_grad_(True)
    yref = torch.nn.functional.layer_norm(xd, (cols,), gd, bd, 1e-5)
    yref.backward(dy0.double())
    mult = _mask(gpu, rows * cols, p, seed, sid).view(rows, cols) if p > 0 else 1.0
    nb = lib.amds_layernorm_bwd_workspace_bytes(rows, cols)
    nchunk = (rows + 63) // 64

    def body(b):
        x, gam, bet, dy = b.inp(x0, ld, "x"), b.inp(gamma0, name="gamma"), b.inp(beta0, name="beta"), b.inp(dy0, ld, "dy")
        y, mean, rstd = b.out((rows, cols), F32, ld, "y"), b.out((rows,), F32, name="mean"), b.out((rows,), F32, name="rstd")
        _lib.check(lib.amds_layernorm_train(_p(x), ld, _p(gam), _p(bet), _p(y), ld, _p(mean), _p(rstd), rows, cols, 1e-5, _lib.F32, _st()), "ln_train")
        y2, mean2, rstd2, xc = b.out((rows, cols), torch.bfloat16, ld, "y2"), b.out((rows,), F32, name="mean2"), b.out((rows,), F32, name="rstd2"), b.out((rows, cols), F32, ld, "x_copy")
        _lib.check(lib.amds_layernorm_train_copy(_p(x), ld, _p(gam), _p(bet), _p(y2), ld, _p(mean2), _p(rstd2), rows, cols, 1e-5, _lib.BF16, _p(xc), ld, cols, _st()),
                   "ln_train_copy")
        outs = dict(y=y, mean=mean, rstd=rstd, y2=y2, mean2=mean2, rstd2=rstd2, x_copy=xc)
        for form in ("bwd", "cast", "partials"):
            dx = b.out((rows, cols), F32, ld, f"dx {form}")
            dx.copy_(skip0)
            ws = b.out((max(nb, 1),), torch.uint8, name=f"ws {form}")
            if form == "partials":
                dg, db = b.out((nchunk, cols), F32, name="dgamma_part"), b.out((nchunk, cols), F32, name="dbeta_part")
            else:
                dg, db = b.out((cols,), F32, name=f"dgamma {form}"), b.out((cols,), F32, name=f"dbeta {form}")
            d16 = b.out((rows, cols), torch.bfloat16, ld, f"dx16 {form}")
            if form == "bwd":
                rc = lib.amds_layernorm_bwd(_p(dy), ld, _p(x), ld, _p(mean), _p(rstd), _p(gam), _p(dx), ld, 1, _p(dg), _p(db), 0, rows, cols, _p(ws), nb, _st())
            elif form == "cast":
                rc = lib.amds_layernorm_bwd_cast(_p(dy), ld, _p(x), ld, _p(mean), _p(rstd), _p(gam), _p(dx), ld, 1, _p(dg), _p(db), 0, rows, cols, _p(ws), nb, _p(d16), ld, p,
                                                 seed, sid, _st())
            else:
                rc = lib.amds_layernorm_bwd_partials(_p(dy), ld, _p(x), ld, _p(mean), _p(rstd), _p(gam), _p(dx), ld, 1, _p(dg), _p(db), rows, cols, _p(d16), ld, p, seed, sid,
                                                     _st())
            _lib.check(rc, form)
            outs.update({f"dx_{form}": dx, f"dg_{form}": dg, f"db_{form}": db})
            if form != "bwd":
                outs[f"dx16_{form}"] = d16
        return outs

    o = _run(gpu, body)
    assert (o["y"].double() - yref.detach()).abs().max() < 1e-5
    assert (o["y2"].double() - yref.detach()).abs().max() < 2 ** -7 * yref.abs().max().item()          # bf16 output: test_layernorm's bar
    assert torch.equal(o["mean"], o["mean2"]) and torch.equal(o["rstd"], o["rstd2"]) and torch.equal(o["x_copy"], x0)
    dxref = skip0.double() + xd.grad
    for form in ("bwd", "cast", "partials"):
        assert (o[f"dx_{form}"].double() - dxref).abs().max() < 2e-5, form
        dg, db = (o[f"{k}_{form}"].double().sum(0) if form == "partials" else o[f"{k}_{form}"].double() for k in ("dg", "db"))
        assert (dg - gd.grad).abs().max() < 1e-3 * max(1.0, gd.grad.abs().max().item()), form
        assert (db - bd.grad).abs().max() < 1e-3 * max(1.0, bd.grad.abs().max().item()), form
        if form != "bwd":
            want = dxref * mult
            assert (o[f"dx16_{form}"].double() - want).abs().max() < 2.0 ** -8 * want.abs().max().item() + 2e-5 * 2, form


# ---- column sums, transposes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, F32])
@pytest.mark.parametrize("M,N,pad", [(777, 300, 4), (4100, 130, 0), (64, 2, 2)])
def test_colsum_family(gpu, dt, M, N, pad):
    """amds_colsum, amds_colsum_partials + a kind-1 entry of amds_colsum_multi, a kind-0 entry (fp32, M <= 2048), amds_sum_partials_multi (test_colsum_multi_is_colsum_bit_for_bit:
    2e-2 max(1, sqrt(M / 1000)), the routes bit-identical).  Per-column bars (M + 2) 2^-23 sum|x|, integer grids bit-equal to fp64, and amds_sum_partials_multi
    bit for bit amds_colsum up to 2048 rows: tests/test_gpu_train_rows.py::test_colsum / test_sum_partials_multi_is_colsum_bit_for_bit."""
    lib, ld = _lib.lib(), N + pad
    g = torch.Generator().manual_seed(M + N)
    x0 = torch.randn(M, N, generator=g).to(dt)
    ref = x0.double().sum(0)
    nb = lib.amds_colsum_workspace_bytes(M, N)
    S, cnt = 3, 4 * ((N + 3) // 4)
    parts0 = torch.randn(S, cnt, generator=g)

    def body(b):
        x, ws, out = b.inp(x0, ld, "x"), b.out((max(nb, 4),), torch.uint8, name="ws"), b.out((N,), F32, name="out")
        _lib.check(lib.amds_colsum(_p(x), ld, _p(out), M, N, ops._DT[dt], 0, _p(ws), nb, _st()), "colsum")
        part, out1 = b.out((max(nb, 4 * N),), torch.uint8, name="part"), b.out((N,), F32, name="out kind 1")
        nchunk = C.c_int(0)
        _lib.check(lib.amds_colsum_partials(_p(x), ld, _p(part), M, N, ops._DT[dt], C.byref(nchunk), _st()), "colsum_partials")
        entries = [_lib.ColsumEntry(_p(part), _p(out1), N, nchunk.value, N, 1)]
        outs = dict(out=out, out1=out1)
        if dt == F32 and M <= 2048:
            out0 = b.out((N,), F32, name="out kind 0")
            entries.append(_lib.ColsumEntry(_p(x), _p(out0), ld, M, N, 0))
            outs["out0"] = out0
        _lib.check(lib.amds_colsum_multi((_lib.ColsumEntry * len(entries))(*entries), len(entries), _st()), "colsum_multi")
        pin, pout = b.inp(parts0, name="parts"), b.out((cnt,), F32, name="sum of partials")
        _lib.check(lib.amds_sum_partials_multi((C.c_void_p * 1)(_p(pin)), (C.c_void_p * 1)(_p(pout)), (C.c_long * 1)(cnt), 1, S, _st()), "sum_partials_multi")
        outs["psum"] = pout
        return outs

    o = _run(gpu, body)
    for k in ("out", "out1", "out0"):
        if k in o:
            assert torch.equal(o[k], o["out"]) and (o[k].double() - ref).abs().max() < 2e-2 * max(1.0, (M / 1000) ** 0.5), k
    assert (o["psum"].double() - parts0.double().sum(0)).abs().max() < _sum_bar(S, parts0.abs().sum(0).max())


@pytest.mark.parametrize("R,Cc,ld", [(640, 2048, 704), (777, 300, 832)])
def test_transpose16(gpu, R, Cc, ld):
    """amds_transpose16 into a padded destination pitch, vector and scalar path (test_transpose_vector_path / test_transpose_colsum: a copy, bit for bit).  The
    destination's columns past R are the caller's: they keep the poison."""
    lib = _lib.lib()
    x0 = torch.randn(R, Cc + 64, generator=torch.Generator().manual_seed(R + Cc)).bfloat16()[:, 64:]

    def body(b):
        x, t = b.inp(x0, Cc + 64, "src"), b.out((Cc, R), torch.bfloat16, ld, "dst")
        _lib.check(lib.amds_transpose16(_p(x), Cc + 64, _p(t), ld, R, Cc, _st()), "transpose16")
        return dict(t=t)

    assert torch.equal(_run(gpu, body)["t"], x0.t())


def test_cast_transpose_multi(gpu):
    """amds_cast_transpose_multi: two matrices, pitched copies and transposed copies, one without a transposed copy (the values are the fp32 -> 16-bit rounding:
    bit for bit torch's cast)."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(3)
    shapes = [(128, 64, torch.bfloat16, True), (64, 192, torch.float16, True), (64, 64, torch.bfloat16, False)]
    srcs = [torch.randn(r, c, generator=g) for r, c, _, _ in shapes]

    def body(b):
        arr, outs = (_lib.CastEntry * len(shapes))(), {}
        for j, ((r, c, dt, tr), s0) in enumerate(zip(shapes, srcs)):
            s, d = b.inp(s0, c + 8, f"src{j}"), b.out((r, c), dt, c + 8, f"dst{j}")
            dtp = b.out((c, r), dt, r + 8, f"dst_t{j}") if tr else None
            arr[j] = _lib.CastEntry(_p(s), c + 8, _p(d), c + 8, _p(dtp), r + 8 if tr else 0, r, c, ops.act_code(dt))
            outs[f"d{j}"] = d
            if tr:
                outs[f"t{j}"] = dtp
        _lib.check(lib.amds_cast_transpose_multi(arr, len(shapes), _st()), "cast_transpose_multi")
        return outs

    o = _run(gpu, body)
    for j, ((r, c, dt, tr), s0) in enumerate(zip(shapes, srcs)):
        assert torch.equal(o[f"d{j}"], s0.to(dt)) and (not tr or torch.equal(o[f"t{j}"], s0.to(dt).t()))


def test_cast_pad(gpu):
    """amds_cast_pad writes the padding itself: zeros up to ld_dst (the GEMMs' precondition on padded K), nothing behind it."""
    lib, (rows, cols, ld_src, ld_dst) = _lib.lib(), (37, 100, 104, 128)
    s0 = torch.randn(rows, cols, generator=torch.Generator().manual_seed(1))

    def body(b):
        s, d = b.inp(s0, ld_src, "src"), b.out((rows, ld_dst), torch.float16, name="dst")
        _lib.check(lib.amds_cast_pad(_p(s), ld_src, _p(d), ld_dst, rows, cols, _lib.F16, _st()), "cast_pad")
        return dict(d=d)

    d = _run(gpu, body)["d"]
    assert torch.equal(d[:, :cols], s0.half()) and bool((d[:, cols:] == 0).all())


# ---- the element-wise dropout sites -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_dropout_sites(gpu, p):
    """amds_dropout_add / _cast_bwd, amds_gelu_dropout_fwd / _bwd and the four *_rows forms (rows r * row_mul of the full tensor), pitched; the multipliers are
    the ones amds_dropout_mask writes for (seed, stream_id).  fp32 results: one fp32 rounding of the exact value (GELU: test_gelu_fwd_bwd's 1e-6 / 1e-5 times the
    keep scale); 16-bit results: rounded once more.  The masks against a restatement of the rule, every dtype route and per-element bars:
    tests/test_gpu_train_rows.py::test_act_dropout / test_dropout_sites / test_rows_forms."""
    lib, (rows, cols, pad, seed, sid, mul) = _lib.lib(), (37, 264, 8, 5, 3, 9)
    ld = cols + pad
    g = torch.Generator().manual_seed(11)
    y0, x0, z0 = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g) * 2
    ks = lib.amds_dropout_keep_scale(p) if p > 0 else 1.0
    full = _mask(gpu, rows * mul * cols, p, seed, sid).view(rows * mul, cols) if p > 0 else torch.ones(rows * mul, cols, dtype=torch.float64)
    m_flat, m_rows = full[:rows], full[::mul]
    zb = z0.bfloat16()
    zd = z0.double().requires_grad_(True)
    torch.nn.functional.gelu(zd).backward(y0.double())
    zbd = zb.double().requires_grad_(True)
    torch.nn.functional.gelu(zbd).backward(y0.bfloat16().double())

    def body(b):
        y, x, z = b.inp(y0, ld, "y"), b.inp(x0, ld, "x_in"), b.inp(z0, name="z")
        o = {}
        o["add"] = b.out((rows, cols), F32, ld, "x_out")
        _lib.check(lib.amds_dropout_add(_p(y), ld, _p(x), ld, _p(o["add"]), ld, rows, cols, p, seed, sid, _st()), "dropout_add")
        o["cast"] = b.out((rows, cols), torch.bfloat16, ld, "dy16")
        _lib.check(lib.amds_dropout_cast_bwd(_p(y), ld, _p(o["cast"]), ld, rows, cols, _lib.BF16, p, seed, sid, _st()), "dropout_cast_bwd")
        o["add_rows"] = b.out((rows, cols), F32, ld, "x_out rows")
        _lib.check(lib.amds_dropout_add_rows(_p(y), ld, _p(x), ld, _p(o["add_rows"]), ld, rows, cols, mul, p, seed, sid, _st()), "dropout_add_rows")
        o["cast_rows"] = b.out((rows, cols), torch.bfloat16, ld, "dy16 rows")
        _lib.check(lib.amds_dropout_cast_bwd_rows(_p(y), ld, _p(o["cast_rows"]), ld, rows, cols, mul, p, seed, sid, _st()), "dropout_cast_bwd_rows")
        o["gelu"], o["dgelu"] = b.out((rows, cols), F32, name="u"), b.out((rows, cols), F32, name="dz")
        yc = b.inp(y0, name="du")
        _lib.check(lib.amds_gelu_dropout_fwd(_p(z), _p(o["gelu"]), rows * cols, _lib.F32, _lib.F32, p, seed, sid, _st()), "gelu_dropout_fwd")
        _lib.check(lib.amds_gelu_dropout_bwd(_p(z), _p(yc), _p(o["dgelu"]), rows * cols, _lib.F32, _lib.F32, _lib.F32, p, seed, sid, _st()), "gelu_dropout_bwd")
        z16, du16 = b.inp(zb, ld, "z16"), b.inp(y0.bfloat16(), ld, "du16")
        o["gelu_rows"], o["dgelu_rows"] = b.out((rows, cols), torch.bfloat16, ld, "u rows"), b.out((rows, cols), torch.bfloat16, ld, "dz rows")
        _lib.check(lib.amds_gelu_dropout_fwd_rows(_p(z16), ld, _p(o["gelu_rows"]), ld, rows, cols, mul, p, seed, sid, _st()), "gelu_dropout_fwd_rows")
        _lib.check(lib.amds_gelu_dropout_bwd_rows(_p(z16), ld, _p(du16), ld, _p(o["dgelu_rows"]), ld, rows, cols, mul, p, seed, sid, _st()), "gelu_dropout_bwd_rows")
        return o

    o = {k: v.double() for k, v in _run(gpu, body).items()}
    u32, u16 = 2.0 ** -23, 2.0 ** -8
    for key, m in (("add", m_flat), ("add_rows", m_rows)):
        want = x0.double() + m * y0.double()
        assert (o[key] - want).abs().max() <= 2 * u32 * want.abs().max(), key
    for key, m in (("cast", m_flat), ("cast_rows", m_rows)):
        want = m * y0.double()
        assert (o[key] - want).abs().max() <= u16 * want.abs().max(), key
    assert (o["gelu"] - m_flat * torch.nn.functional.gelu(z0.double())).abs().max() < 1e-6 * ks
    assert (o["dgelu"] - m_flat * zd.grad).abs().max() < 1e-5 * ks
    want = m_rows * torch.nn.functional.gelu(zb.double())
    assert (o["gelu_rows"] - want).abs().max() <= u16 * want.abs().max() + 1e-6 * ks
    want = m_rows * zbd.grad
    assert (o["dgelu_rows"] - want).abs().max() <= u16 * want.abs().max() + 1e-5 * ks


# ---- TransMIL's small fp32 kernels ---------------------------------------------------------------------------------------------------------------
def test_transmil_small_kernels(gpu):
    """amds_landmark_mean / _bwd, amds_dwconv_seq / _row / _wgrad on head slices of a packed qkv [b][np][3 C] (the addressing of tests/chains/transmil.py), amds_softmax_rows
    / _bwd, amds_ppeg / _wgrad on an 8 x 8 grid: each against fp64 within the rounding bound of its sum (module docstring)."""
    lib, (b_, H, np_, d, m, taps) = _lib.lib(), (2, 8, 70, 8, 35, 33)
    Cd, l, e4 = H * d, 2, 4
    sb, sh, ld = np_ * 3 * Cd, d, 3 * Cd
    g = torch.Generator().manual_seed(21)
    qkv0 = torch.randn(b_, np_, 3 * Cd, generator=g)
    w0, merged0 = torch.randn(H, taps, generator=g) * 0.2, torch.randn(b_, np_, Cd, generator=g)
    q = qkv0[..., :Cd].reshape(b_, np_, H, d).permute(0, 2, 1, 3).double()                                       # [b, H, np, d]
    v = qkv0[..., 2 * Cd:].reshape(b_, np_, H, d).permute(0, 2, 1, 3).double()
    lm_ref = q.reshape(b_, H, m, l, d).sum(3) * 0.25
    vpad = torch.nn.functional.pad(v, (0, 0, taps // 2, taps // 2))
    win = vpad.unfold(2, taps, 1)                                                                                # [b, H, np, d, taps]
    conv = (win * w0.double().view(1, H, 1, 1, taps)).sum(-1)
    conv_abs = (win.abs() * w0.double().abs().view(1, H, 1, 1, taps)).sum(-1)
    mh = merged0.reshape(b_, np_, H, d).permute(0, 2, 1, 3).double()
    dw_ref = torch.einsum("bhtc,bhtck->hk", mh, win)
    dw_abs = torch.einsum("bhtc,bhtck->hk", mh.abs(), win.abs())
    sm0, dsm0 = torch.randn(37, m, generator=g) * 3, torch.randn(37, m, generator=g)
    pr = torch.softmax(sm0.double(), -1)
    dlm0 = torch.randn(b_, H, m, d, generator=g)
    Bp, side = 2, 8
    px0, pdy0 = torch.randn(Bp, 1 + side * side, Cd, generator=g), torch.randn(Bp, 1 + side * side, Cd, generator=g)
    pw = [torch.randn(Cd, k * k, generator=g) * 0.1 for k in (7, 5, 3)]
    pb = [torch.randn(Cd, generator=g) * 0.1 for _ in range(3)]
    img = px0[:, 1:].double().reshape(Bp, side, side, Cd).permute(0, 3, 1, 2)
    pref, pabs = img.clone(), img.abs()
    for w_, b__, k in zip(pw, pb, (7, 5, 3)):
        pref = pref + torch.nn.functional.conv2d(img, w_.double().view(Cd, 1, k, k), b__.double(), padding=k // 2, groups=Cd)
        pabs = pabs + torch.nn.functional.conv2d(img.abs(), w_.double().abs().view(Cd, 1, k, k), b__.double().abs(), padding=k // 2, groups=Cd)
    dyimg = pdy0[:, 1:].double().reshape(Bp, side, side, Cd).permute(0, 3, 1, 2)
    xwin = torch.nn.functional.pad(img, (3, 3, 3, 3)).unfold(2, 7, 1).unfold(3, 7, 1)                              # [B, C, i, j, r, q]
    corr_ref = torch.cat([torch.einsum("bcij,bcijrq->rqc", dyimg, xwin).reshape(49, Cd), dyimg.sum((0, 2, 3))[None]])
    corr_abs = torch.cat([torch.einsum("bcij,bcijrq->rqc", dyimg.abs(), xwin.abs()).reshape(49, Cd), dyimg.abs().sum((0, 2, 3))[None]])
    nbw, nbp = lib.amds_dwconv_seq_wgrad_workspace_bytes(b_, H, taps), lib.amds_ppeg_wgrad_workspace_bytes(Bp, Cd)

    def body(b):
        qkv, w, merged_in = b.inp(qkv0.reshape(b_ * np_, 3 * Cd), name="qkv"), b.inp(w0, name="conv_w"), b.inp(merged0.reshape(b_ * np_, Cd), name="dmerged")
        vp = qkv.data_ptr() + 2 * Cd * e4
        o = {}
        o["lm"] = b.out((b_ * H * m, d), F32, name="landmarks")
        _lib.check(lib.amds_landmark_mean(_p(qkv), sb, sh, ld, _p(o["lm"]), b_, H, m, l, d, 0.25, _st()), "landmark_mean")
        o["conv"] = b.out((b_ * np_, Cd), F32, name="merged")
        o["conv"].copy_(merged0.reshape(b_ * np_, Cd))
        _lib.check(lib.amds_dwconv_seq(vp, sb, sh, ld, _p(w), _p(o["conv"]), np_ * Cd, d, Cd, b_, H, np_, d, taps, _st()), "dwconv_seq")
        o["conv_row"] = b.out((b_, Cd), F32, name="merged row")
        o["conv_row"].zero_()
        _lib.check(lib.amds_dwconv_seq_row(vp, sb, sh, ld, _p(w), _p(o["conv_row"]), Cd, d, b_, H, np_, d, taps, np_ - 1, _st()), "dwconv_seq_row")
        ws, o["dw"] = b.out((max(nbw, 1),), torch.uint8, name="wgrad ws"), b.out((H, taps), F32, name="dw")
        _lib.check(lib.amds_dwconv_seq_wgrad(_p(merged_in), np_ * Cd, d, Cd, vp, sb, sh, ld, _p(o["dw"]), b_, H, np_, d, taps, _p(ws), nbw, _st()), "dwconv_seq_wgrad")
        dlm = b.inp(dlm0.reshape(-1, d), name="dlandmarks")
        o["dqkv"] = b.out((b_ * np_, 3 * Cd), F32, name="dqkv")
        o["dqkv"].zero_()
        _lib.check(lib.amds_landmark_mean_bwd(_p(dlm), _p(o["dqkv"]), sb, sh, ld, b_, H, m, l, d, 0.25, 1, _st()), "landmark_mean_bwd")
        o["p"] = b.out((37, m), F32, name="softmax")
        o["p"].copy_(sm0)
        _lib.check(lib.amds_softmax_rows(_p(o["p"]), 37, m, _st()), "softmax_rows")
        o["dp"] = b.out((37, m), F32, name="dsoftmax")
        o["dp"].copy_(dsm0)
        _lib.check(lib.amds_softmax_rows_bwd(_p(o["p"]), _p(o["dp"]), 37, m, _st()), "softmax_rows_bwd")
        px, pdy = b.inp(px0.reshape(-1, Cd), name="ppeg x"), b.inp(pdy0.reshape(-1, Cd), name="ppeg dy")
        wts = [b.inp(t, name="ppeg w") for t in pw]
        bs = [b.inp(t, name="ppeg b") for t in pb]
        o["ppeg"] = b.out((Bp * (1 + side * side), Cd), F32, name="ppeg y")
        _lib.check(lib.amds_ppeg(_p(px), _p(o["ppeg"]), _p(wts[0]), _p(bs[0]), _p(wts[1]), _p(bs[1]), _p(wts[2]), _p(bs[2]), Bp, side, side, Cd, _st()), "ppeg")
        pws, o["corr"] = b.out((max(nbp, 1),), torch.uint8, name="ppeg ws"), b.out((50, Cd), F32, name="dcorr")
        _lib.check(lib.amds_ppeg_wgrad(_p(px), _p(pdy), _p(o["corr"]), Bp, side, side, Cd, _p(pws), nbp, _st()), "ppeg_wgrad")
        return o

    o = {k: v.double() for k, v in _run(gpu, body).items()}
    assert (o["lm"].view(b_, H, m, d) - lm_ref).abs().max() <= _sum_bar(l, q.abs().reshape(b_, H, m, l, d).sum(3).max() * 0.25)
    got = o["conv"].view(b_, np_, H, d).permute(0, 2, 1, 3)
    assert (got - (mh + conv)).abs().max() <= _sum_bar(taps + 1, (mh.abs() + conv_abs).max())
    assert (o["conv_row"].view(b_, H, d) - conv[:, :, np_ - 1]).abs().max() <= _sum_bar(taps, conv_abs.max())
    assert (o["dw"] - dw_ref).abs().max() <= _sum_bar(b_ * np_ * d, dw_abs.max())
    dq = o["dqkv"][:, :Cd].view(b_, np_, H, d).permute(0, 2, 1, 3)
    want = (dlm0.double() * 0.25).unsqueeze(3).expand(b_, H, m, l, d).reshape(b_, H, np_, d)
    assert (dq - want).abs().max() <= 2.0 ** -23 * want.abs().max() and bool((o["dqkv"][:, Cd:] == 0).all())
    assert (o["p"] - pr).abs().max() <= _sum_bar(m, 1.0) + 2.0 ** -21          # exp in fp32: a few ulp of a value <= 1
    dpr = pr * (dsm0.double() - (pr * dsm0.double()).sum(-1, keepdim=True))
    assert (o["dp"] - dpr).abs().max() <= _sum_bar(m, (pr * dsm0.double().abs()).sum(-1).max() + dsm0.abs().max()) + 2.0 ** -21 * dsm0.abs().max().item()
    y = o["ppeg"].view(Bp, 1 + side * side, Cd)
    assert torch.equal(y[:, 0].float(), px0[:, 0])
    assert (y[:, 1:].reshape(Bp, side, side, Cd).permute(0, 3, 1, 2) - pref).abs().max() <= _sum_bar(49 + 25 + 9 + 4, pabs.max())
    assert (o["corr"] - corr_ref).abs().max() <= _sum_bar(Bp * side * side, corr_abs.max())


# ---- gathers, pools, activations ---------------------------------------------------------------------------------------------------------------
def test_gather_topk_pool_quick_gelu(gpu):
    """amds_gather_rows (f16 -> f32, pitched, zero rows behind the indices), amds_topk_rows_mean, amds_mean_pool / _bwd, amds_quick_gelu_inplace on pitched rows."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(31)
    src0, idx0 = torch.randn(50, 264, generator=g).half(), torch.randperm(50, generator=g)[:20]
    sc0, rows0 = torch.randn(300, generator=g), torch.randn(300, 96, generator=g)
    x0, dy0 = torch.randn(3, 77, 40, generator=g).half(), torch.randn(3, 40, generator=g)
    u0 = (torch.randn(37, 72, generator=g) * 3).half()
    top = torch.topk(sc0, 5).indices

    def body(b):
        src, idx, o = b.inp(src0, 272, "src"), b.inp(idx0, name="idx"), {}
        o["bag"] = b.out((32, 264), F32, 272, "bag")
        _lib.check(lib.amds_gather_rows(_p(src), 272, _p(idx), 20, _p(o["bag"]), 272, 32, 264, _lib.F16, _lib.F32, _st()), "gather_rows")
        sc, rows = b.inp(sc0, name="score"), b.inp(rows0, 104, "rows")
        o["idx"], o["mean"] = b.out((5,), torch.int32, name="idx_out"), b.out((96,), F32, name="mean_out")
        _lib.check(lib.amds_topk_rows_mean(_p(sc), 300, 5, _p(rows), 104, 96, _lib.F32, _p(o["idx"]), _p(o["mean"]), _st()), "topk_rows_mean")
        x, dy = b.inp(x0.reshape(-1, 40), name="x"), b.inp(dy0, name="dy")
        o["pool"], o["dpool"] = b.out((3, 40), F32, name="pooled"), b.out((3 * 77, 40), F32, name="dx")
        _lib.check(lib.amds_mean_pool(_p(x), _p(o["pool"]), 3, 77, 40, _lib.F16, _st()), "mean_pool")
        _lib.check(lib.amds_mean_pool_bwd(_p(dy), _p(o["dpool"]), 3, 77, 40, _st()), "mean_pool_bwd")
        o["u"] = b.out((37, 72), torch.float16, 80, "u")
        o["u"].copy_(u0)
        _lib.check(lib.amds_quick_gelu_inplace(_p(o["u"]), 80, 37, 72, _lib.F16, _st()), "quick_gelu")
        return o

    o = _run(gpu, body)
    assert torch.equal(o["bag"][:20], src0[idx0].float()) and bool((o["bag"][20:] == 0).all())            # a copy + zero rows: bit for bit
    assert torch.equal(o["idx"].long(), top)
    want = rows0[top].double().mean(0)
    assert (o["mean"].double() - want).abs().max() <= _sum_bar(5, rows0[top].abs().sum(0).max() / 5)
    want = x0.double().mean(1)
    assert (o["pool"].double() - want).abs().max() <= _sum_bar(77, x0.double().abs().sum(1).max() / 77)
    want = (dy0.double() / 77)[:, None].expand(3, 77, 40).reshape(-1, 40)
    assert (o["dpool"].double() - want).abs().max() <= 2.0 ** -23 * want.abs().max()
    want = u0.double() * torch.sigmoid(1.702 * u0.double())
    assert (o["u"].double() - want).abs().max() <= 2.0 ** -10 * want.abs().max()                           # one fp16 ulp of the range (the BIAS epilogue's bar)
