"""tests/nystrom_oracle.py pinned to independent evaluations, with no kernel: each reference against torch.nn.functional, each backward against fp64 autograd of
its forward, PPEG and the pinv start against oracle/transmil.py, the tie rule on a hand-built case, and -- for EVERY integer-grid case test_gpu_nystrom_kernels.py
runs -- that all sums stay below 2^24 in units of the grid, the condition under which fp32 is exact in any order (asserted from the references' abs_sum)."""
import pytest
import torch
import torch.nn.functional as F

import nystrom_oracle as O
from oracle import transmil as OT

F64 = torch.float64
TINY = 1e-12          # fp64 references of O(1) .. O(100) values against each other


def _close(a, b, tol=TINY):
    scale = max(1.0, float(b.abs().max()))
    assert a.shape == b.shape and float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---- forwards against torch.nn.functional ----------------------------------------------------------------------------------------------------------------
def test_softmax_and_its_backward():
    x = torch.randn(5, 37, generator=_g(1), dtype=F64) * 3
    p, ab = O.softmax_rows(x)
    _close(p, F.softmax(x, -1))
    assert torch.equal(p, ab)
    xr = x.clone().requires_grad_(True)
    dp = torch.randn(5, 37, generator=_g(2), dtype=F64)
    (F.softmax(xr, -1) * dp).sum().backward()
    val, ab = O.softmax_rows_bwd(p, dp)
    _close(val, xr.grad)
    assert bool((ab >= val.abs() - 1e-15).all())


def test_landmark_mean_and_its_backward():
    b, H, m, l, d = 2, 3, 7, 3, 6
    qkv = torch.randn(b, m * l, 3 * H * d, generator=_g(3), dtype=F64)
    for which in (0, 1, 2):
        val, _ = O.landmark_mean(qkv, which, H, d, m, l, 0.125)
        x = qkv[..., which * H * d:(which + 1) * H * d].reshape(b, m, l, H, d)          # written the other way round: split the rows first, the heads second
        _close(val, x.sum(2).permute(0, 2, 1, 3) * 0.125)
    dout = torch.randn(b, H, m, d, generator=_g(4), dtype=F64)
    q = qkv.clone().requires_grad_(True)
    (O.landmark_mean(q, 1, H, d, m, l, 0.125)[0] * dout).sum().backward()
    dx0 = torch.randn(b, m * l, 3 * H * d, generator=_g(5), dtype=F64)
    _close(O.landmark_mean_bwd(dout, dx0, 1, H, d, m, l, 0.125, 1)[0], dx0 + q.grad)
    got = O.landmark_mean_bwd(dout, dx0, 1, H, d, m, l, 0.125, 0)[0]
    blk = slice(H * d, 2 * H * d)
    _close(got[..., blk], q.grad[..., blk])
    assert torch.equal(got[..., :H * d], dx0[..., :H * d]) and torch.equal(got[..., 2 * H * d:], dx0[..., 2 * H * d:])


@pytest.mark.parametrize("taps", [1, 3, 33])
def test_dwconv_seq_row_and_wgrad(taps):
    b, H, n, d = 2, 3, 19, 5
    v = torch.randn(b, H, n, d, generator=_g(6), dtype=F64)
    w = torch.randn(H, taps, generator=_g(7), dtype=F64)
    out0 = torch.randn(b, H, n, d, generator=_g(8), dtype=F64)

    def conv(v_, w_):          # channels = (head, column), every column of a head with that head's taps
        inp = v_.permute(0, 1, 3, 2).reshape(b, H * d, n)
        return F.conv1d(inp, w_.repeat_interleave(d, 0).view(H * d, 1, taps), padding=taps // 2, groups=H * d).reshape(b, H, d, n).permute(0, 1, 3, 2)

    val, ab = O.dwconv_seq(v, w, out0)
    _close(val, out0 + conv(v, w))
    _close(ab, out0.abs() + conv(v.abs(), w.abs()))
    for row in (0, n // 2, n - 1):
        r0 = out0[:, :, 0]
        _close(O.dwconv_seq_row(v, w, r0, row)[0], r0 + conv(v, w)[:, :, row])
    dout = torch.randn(b, H, n, d, generator=_g(9), dtype=F64)
    wr = w.clone().requires_grad_(True)
    (conv(v, wr) * dout).sum().backward()
    _close(O.dwconv_seq_wgrad(dout, v, taps)[0], wr.grad)


@pytest.mark.parametrize("Hh,Ww", [(1, 1), (2, 3), (7, 7), (3, 11)])
def test_ppeg_and_its_wgrad(Hh, Ww):
    B, C = 2, 5
    x, dy, ws, bs, _ = O.ppeg_inputs(B, Hh, Ww, C, "real")
    x, dy, ws, bs = x.double(), dy.double(), [w.double() for w in ws], [b.double() for b in bs]
    val, ab = O.ppeg(x, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], Hh, Ww)
    img = x[:, 1:].reshape(B, Hh, Ww, C).permute(0, 3, 1, 2)

    def f(ws_, bs_, img_):
        y = img_
        for w_, b_, k in zip(ws_, bs_, (7, 5, 3)):
            y = y + F.conv2d(img_, w_.view(C, 1, k, k), b_, padding=k // 2, groups=C)
        return y.permute(0, 2, 3, 1).reshape(B, Hh * Ww, C)

    _close(val[:, 1:], f(ws, bs, img))
    _close(ab[:, 1:], f([w.abs() for w in ws], [b.abs() for b in bs], img.abs()))
    assert torch.equal(val[:, 0], x[:, 0])
    sd = {"p.proj.weight": ws[0].view(C, 1, 7, 7), "p.proj.bias": bs[0], "p.proj1.weight": ws[1].view(C, 1, 5, 5), "p.proj1.bias": bs[1],
          "p.proj2.weight": ws[2].view(C, 1, 3, 3), "p.proj2.bias": bs[2]}
    _close(val, OT.ppeg(x, sd, "p.", Hh, Ww))
    # the tap-correlation table = the gradients of the three kernels: w7's in full, w5 / w3 its central 5 x 5 / 3 x 3, the biases its last row
    wr, br = [w.clone().requires_grad_(True) for w in ws], [b.clone().requires_grad_(True) for b in bs]
    (f(wr, br, img) * dy[:, 1:]).sum().backward()
    corr, _ = O.ppeg_wgrad(x, dy, Hh, Ww)
    t = corr[:49].reshape(7, 7, C)
    _close(t.reshape(49, C).T, wr[0].grad)
    _close(t[1:6, 1:6].reshape(25, C).T, wr[1].grad)
    _close(t[2:5, 2:5].reshape(9, C).T, wr[2].grad)
    for b_ in br:
        _close(corr[49], b_.grad)


def test_pinv_init_against_the_model_oracle_and_by_groups():
    x = O.pinv_inputs(35, "real").double()
    z, _ = O.pinv_init(x, 6)
    _close(z, OT.pinv_iter(x, iters=0), 1e-13)
    for group in (2, 1):
        zg, _ = O.pinv_init(x, group)
        for k in range(0, 6, group):
            _close(zg[k:k + group], O.pinv_init(x[k:k + group], group)[0], 1e-13)
    ax = x.abs()
    assert int(ax.sum(-1).reshape(-1).argmax()) // 35 == 1 and int(ax.sum(-2).reshape(-1).argmax()) // 35 == 4          # planted in different matrices


@pytest.mark.parametrize("family", ["grid", "real"])
def test_pinv_init_bwd_closed_form_is_the_autograd_gradient(family):
    x, dz, dx0 = (t.double() for t in O.pinv_bwd_inputs(40, family))
    xr = x.clone().requires_grad_(True)
    (O.pinv_init(xr, 3)[0] * dz).sum().backward()
    p = O.pinv_init_bwd_parts(x, dz, dx0)
    _close(p["value"], dx0 + xr.grad, 1e-13)
    assert (p["row"], p["col"]) == (2 * 40 + 40 // 3, 40 // 2) and p["row_margin"] >= 1e-3 and p["col_margin"] >= 1e-3
    assert bool((p["abs_sum"] >= p["value"].abs() * (1 - 1e-12)).all()) and bool((p["largest"] <= p["abs_sum"] * (1 + 1e-12)).all())


def test_pinv_init_bwd_tie_goes_to_the_first_index():
    x, dz, dx0, row, col = O.pinv_bwd_tie_inputs(32)
    n = 32
    assert torch.equal(x[1, 5], x[2, 3]) and torch.equal(x[0, :, 7], x[0, :, 9])
    rs, cs = x.sum(-1).reshape(-1), x.sum(-2).reshape(-1)
    assert int((rs == rs.max()).sum()) == 2 and int((cs == cs.max()).sum()) == 2
    p = O.pinv_init_bwd_parts(x, dz, dx0)
    assert (p["row"], p["col"]) == (row, col) == (n + 5, 7) and p["row_margin"] == 0.0 and p["col_margin"] == 0.0
    # by hand: only row (1, 5) and column (0, 7) carry the ds terms
    s = 9.0 * n * n
    ds = -float((dz.double().transpose(-1, -2) * x.double()).sum()) / s ** 2
    want = dx0.double() + dz.double().transpose(-1, -2) / s
    want[1, 5] += ds * 3 * n
    want[0, :, 7] += ds * 3 * n
    _close(p["value"], want, 1e-14)


# ---- the bars of the real family are bars: torch's own fp32 softmax sits far inside them --------------------------------------------------------------------
@pytest.mark.parametrize("cols", [256, 1280, 2048])
def test_softmax_bar_holds_for_an_fp32_softmax(cols):
    x, _ = O.softmax_inputs(8, cols, "real")
    p, _ = O.softmax_rows(x)
    ratio = (F.softmax(x, -1).double() - p).abs() / O.softmax_rows_bar(x)
    assert float(ratio.max()) <= 0.5, float(ratio.max())          # (measured 0.08: the row sum is a tree, not a chain)
    pf, dp, _ = O.softmax_bwd_inputs(8, cols, "real")
    val, _ = O.softmax_rows_bwd(pf, dp)
    got = pf * (dp - (pf * dp).sum(-1, keepdim=True))
    # the bar's 2^-149 is what the FORMAT asks for, nothing more: without it this plain fp32 evaluation misses the relative bar, and only at subnormal results
    over = (got.double() - val).abs() > O.softmax_rows_bwd_bar(pf, dp) - 2.0 ** -149
    assert bool((val[over].abs() < 2.0 ** -126).all()) and (cols == 256 or bool(over.any()))
    assert float(((got.double() - val).abs() / O.softmax_rows_bwd_bar(pf, dp)).max()) <= 0.5          # (measured 0.28, at the spike: dp_j - s cancels)


# ---- every integer-grid case of the GPU file is exact in fp32 ------------------------------------------------------------------------------------------------
def _exact(abs_sum, unit=1.0):
    assert float((abs_sum / unit).max()) < O.EXACT, float((abs_sum / unit).max())


def _on_grid(val, unit=1.0):
    q = val / unit
    assert torch.equal(q, q.round())


def test_grid_softmax_cases_are_exact():
    for cols in O.SOFTMAX_COLS:
        for rows in O.SOFTMAX_ROWS:
            x, unit = O.softmax_inputs(rows, cols, "grid")
            p, ab = O.softmax_rows(x)
            _exact(ab, unit.double())
            assert bool(((p == unit.double()) | (p == 0)).all()) and bool((p.sum(-1) == 1).all())          # 1 / k or 0, k a power of two
            pf, dp, unit = O.softmax_bwd_inputs(rows, cols, "grid")
            val, ab = O.softmax_rows_bwd(pf, dp)
            _exact(ab, unit)
            _on_grid(val, unit)


def test_grid_landmark_cases_are_exact():
    b, H = O.LANDMARK_B, O.LANDMARK_H
    for m, l, d in O.LANDMARK_CASES:
        qkv, dout, dx0, scale, unit = O.landmark_inputs(m, l, d, "grid")
        val, ab = O.landmark_mean(qkv, 0, H, d, m, l, scale)
        _exact(ab, unit)
        _on_grid(val, unit)
        val, ab = O.landmark_mean_bwd(dout, dx0, 0, H, d, m, l, scale, 1)
        _exact(ab, unit)
        _on_grid(val, unit)


def test_grid_dwconv_cases_are_exact():
    H = O.DWCONV_H
    for n, d, taps in O.DWCONV_WIN_CASES + O.DWCONV_GENERIC_CASES + O.WGRAD_WIN_CASES + O.WGRAD_GENERIC_CASES + tuple((n, d, 33) for n, d in O.DWCONV_ROW_CASES):
        qkv, w, merged, unit = O.dwconv_inputs(n, d, taps, "grid")
        v, mh = O.head_slice(qkv, 2, H, d), O.head_slice(merged, 0, H, d)
        val, ab = O.dwconv_seq(v, w, mh)
        _exact(ab, unit)
        _on_grid(val, unit)
        val, ab = O.dwconv_seq_wgrad(mh, v, taps)
        _exact(ab, unit)
        _on_grid(val, unit)


def test_grid_ppeg_cases_are_exact():
    for Hh, Ww in O.PPEG_WGRAD_GRIDS:
        for C, B in ((max(O.PPEG_C), max(O.PPEG_B)), (max(O.PPEG_WGRAD_C), max(O.PPEG_WGRAD_B))):          # the sums grow with B only; C is a batch dimension
            x, dy, ws, bs, unit = O.ppeg_inputs(B, Hh, Ww, C, "grid")
            val, ab = O.ppeg(x, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], Hh, Ww)
            _exact(ab, unit)
            _on_grid(val, unit)
            val, ab = O.ppeg_wgrad(x, dy, Hh, Ww)
            _exact(ab, unit)
            _on_grid(val, unit)


def test_grid_pinv_cases_are_exact():
    """The sums of |x| and their product s are integers below 2^24: the kernel's s is exact and what is left is the reciprocal and one product (pinv_init), or the
    counted roundings of test_gpu_nystrom_kernels.py's bar (pinv_init_bwd)."""
    for n in O.PINV_N:
        ax = O.pinv_inputs(n, "grid").double().abs()
        assert float(ax.sum(-1).max() * ax.sum(-2).max()) < O.EXACT
        assert int(ax.sum(-1).reshape(-1).argmax()) // n == 1 or n < 32          # (tiny matrices: wherever the maxima fall)
    for n in O.PINV_BWD_N:
        x, dz, dx0 = O.pinv_bwd_inputs(n, "grid")
        p = O.pinv_init_bwd_parts(x, dz, dx0)
        assert p["s"] < O.EXACT and p["dot_abs"] < O.EXACT
        assert (p["row"], p["col"]) == (2 * n + n // 3, n // 2) and p["row_margin"] >= 1e-3 and p["col_margin"] >= 1e-3
    x, dz, dx0, _, _ = O.pinv_bwd_tie_inputs(32)
    p = O.pinv_init_bwd_parts(x, dz, dx0)
    assert p["s"] < O.EXACT and p["dot_abs"] < O.EXACT


def test_real_pinv_bwd_cases_have_unique_maxima():
    for n in O.PINV_BWD_N:
        x, dz, dx0 = O.pinv_bwd_inputs(n, "real")
        assert bool((x > 0).all())
        p = O.pinv_init_bwd_parts(x, dz, dx0)
        assert (p["row"], p["col"]) == (2 * n + n // 3, n // 2) and p["row_margin"] >= 1e-3 and p["col_margin"] >= 1e-3, (n, p["row_margin"], p["col_margin"])
