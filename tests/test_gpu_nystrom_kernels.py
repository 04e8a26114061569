"""Every dispatch variant of the Nystrom / TransMIL fp32 kernels (stamp_amd/csrc/transmil.hip) against fp64, through the C ABI, element by element.

References, inputs and bars: tests/nystrom_oracle.py (pinned on the CPU by test_cpu_nystrom_oracle.py).  Two families per kernel:

* grid -- integer operands whose every partial sum is exact in fp32 (asserted on the CPU for every case below): the kernel must equal fp64 BIT FOR BIT.  Behind a
  division the bar is a counted number of roundings of the element's largest term L, in units of 2^-23 L:
    amds_pinv_init      2: s = rmax * cmax is exact, 1 / s rounds once, x * (1 / s) once -- 2 * 2^-24 = 1 unit; 2 units allowed.
    amds_pinv_init_bwd  8: s exact; dz / s 1 rounding; ds * cmax and ds * rmax 3 each (s * s, the quotient, the product); the three additions g + t2, + t3, dx + g
                        round results of at most 2 L, 3 L, 4 L -- (1 + 3 + 3 + 2 + 3 + 4) * 2^-24 L = 8 * 2^-23 L.
* real -- Gaussian operands at the model's magnitudes and the softmax edge rows, |got - ref| <= (n_terms + 2) * 2^-23 * abs_sum PER ELEMENT (the bound of
  test_gpu_abi_rows.py's `_sum_bar`, no longer taken at the tensor's maximum); the softmax bars are nystrom_oracle.softmax_rows_bar / _bwd_bar.
  n_terms: landmark_mean l, _bwd 2; dwconv_seq taps + 1, _row taps + 1, _wgrad outer * n * d; ppeg 49 + 25 + 9 + 4, ppeg_wgrad B * Hh * Ww; pinv_init n (the two
  maxima are sums of n terms: 2 n * 2^-24); pinv_init_bwd nmat * n^2 + 4 n (the dot product over all matrices, s^2 from four sums of n terms).

Outputs sit between two 64-float bands of a marker value that must survive the call.  Each check prints `nystrom| kernel | variant | family | case | error / bar`
under -s, and the module ends with the worst figure per kernel, variant and family: profiles/nystrom_kernel_errors.txt is that table from one run.

Which case reaches which kernel (transmil.hip line of the condition; every hipLaunchKernelGGL of the entry points below is named once):

  amds_softmax_rows / _bwd (:1496-1507 / :1213-1224; cols % 4 == 0, cols <= 2048, 16-byte aligned -> one wave per row, else a workgroup per row)
    cols 4, 252, 256          softmax_rows_wave_kernel<1> / softmax_rows_bwd_wave_kernel<1>      :1499 / :1216
    cols 260, 512             <2>                                                                 :1500 / :1217
    cols 516, 1024            <4>                                                                 :1501 / :1218
    cols 1028, 1280           <5>                                                                 :1502 / :1219
    cols 1284, 2048           <8>                                                                 :1503 / :1220
    cols 2052, 35, 1; cols 256 on a pointer one float off     softmax_rows_kernel / softmax_rows_bwd_kernel      :1507 / :1224
    rows 1, 5, 8: four rows per workgroup (:561 / :853), 5 leaves a partial one
  amds_landmark_mean / _bwd (:1515 / :1232; d, ld, strides multiples of 4 and 16-byte aligned)
    (m, l, d) (1,1,4), (35,2,8), (256,5,64)      landmark_mean4_kernel / landmark_mean_bwd4_kernel      :1516 / :1233
    (7,3,6) (d and ld no multiple of 4); (35,2,8) one float off      landmark_mean_kernel / landmark_mean_bwd_kernel      :1519 / :1236
  amds_pinv_init / _grouped (:1531-1533, then :1538)
    n 4, 32, 252, 256         absmax_kernel<2>         :1531
    n 260, 512, 1024          absmax_kernel<8>         :1532
    n 35, 1028                absmax_any_kernel        :1533
    every n                   transpose_scale_kernel   :1538      (nmat, group) (6,6), (6,2), (6,1): one, three, six pairs of maxima
  amds_pinv_init_bwd (:1355-1358, then :1362)
    n 32, 256 (+ the tie case, n 32)      pinv_init_bwd_stats_kernel<2>      :1356
    n 288, 1024                           pinv_init_bwd_stats_kernel<8>      :1357
    n 40, 1056                            pinv_init_bwd_stats_any_kernel     :1358
    every n                               pinv_init_bwd_apply_kernel         :1362
  amds_dwconv_seq (:1573)
    taps 33, n 1 .. 300 x d 8, 64, 72      dwconv_seq_win_kernel<33, 32> (128 positions x 64 channels per workgroup)      :1575
    taps 1, 3, 31, 35; taps 33 in the child (AMDS_DWCONV_WIN=0)      dwconv_seq_kernel      :1580
  amds_dwconv_seq_row      dwconv_seq_row_kernel      :1590
  amds_dwconv_seq_wgrad (:1251)
    taps 33, n 1 .. 200 x d 8 .. 130       dwconv_seq_wgrad_win_kernel<33, 16> (16 positions x 4 waves)      :1252
    taps 31, d 8, 64, 256; taps 33 d 8 in the child       dwconv_seq_wgrad_kernel, 256 % d == 0 branch (:913)      :1256
    taps 31, d 24, 72, 320; taps 33 d 72, 130 in the child      dwconv_seq_wgrad_kernel, flat branch (:917)      :1256
  amds_ppeg      ppeg_kernel      :1599      grids below the 7 x 7 window (1x1 .. 4x4), at it, above it, oblong; C 4, 64 (partial block), 257, 320 (two blocks)
  amds_ppeg_wgrad (:1274)
    every grid, + Ww 15, 16, 17, 33 at Hh 2 (runs of 16 columns); B 3 leaves a chunk of one bag      ppeg_wgrad_win_kernel<16>      :1275
    the child (AMDS_DWCONV_WIN=0)       ppeg_wgrad_kernel      :1278
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import nystrom_oracle as O
from stamp_amd import _lib

pytestmark = pytest.mark.gpu
F32 = torch.float32
BAND, MARK = 64, 24301.5
FAMILIES = ("grid", "real")
_WORST: dict = {}


# ---- operands ----------------------------------------------------------------------------------------------------------------------------------------------
def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, gpu, offset=0):
    """t on the device; `offset` floats off the allocation's (256-byte) alignment."""
    buf = torch.empty(t.numel() + offset, dtype=F32, device=gpu)
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * offset) % 16
    return v


class _Out:
    """An output (pre-filled with t) between two bands of MARK; `cpu()` checks the bands and returns the interior."""

    def __init__(self, t, gpu, offset=0):
        self.buf = torch.full((2 * BAND + t.numel() + offset,), MARK, dtype=F32, device=gpu)
        self.lo, self.hi = BAND + offset, BAND + offset + t.numel()
        self.view = self.buf[self.lo:self.hi].view(t.shape)
        self.view.copy_(t)
        assert self.view.data_ptr() % 16 == (4 * offset) % 16

    def ptr(self):
        return self.view.data_ptr()

    def cpu(self):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        assert bool((host[:self.lo] == MARK).all()) and bool((host[self.hi:] == MARK).all()), "the call wrote outside its output"
        return host[self.lo:self.hi].view(self.view.shape).clone()


def _ws(gpu, nbytes):
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=gpu)


def _judge(kernel, variant, family, case, got, ref, bar=None):
    """bar None: bit for bit.  Prints the figure, keeps the worst per (kernel, variant, family), then asserts."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{kernel} {variant} {case}: shape or non-finite output"
    err = (got - ref).abs()
    if bar is None:
        ratio = 0.0 if bool((err == 0).all()) else float("inf")
        where = "" if ratio == 0.0 else f"{int((err != 0).sum())} element(s) differ, first at flat index {int((err != 0).reshape(-1).nonzero()[0])}, largest difference {float(err.max()):.6g}"
    else:
        r = torch.where(err == 0, torch.zeros_like(err), err / bar)
        ratio = float(r.max())
        i = int(r.reshape(-1).argmax())
        where = f"flat index {i}: got {float(got.reshape(-1)[i])!r} want {float(ref.reshape(-1)[i])!r}, error {float(err.reshape(-1)[i]):.6g}"
    print(f"nystrom| {kernel} | {variant} | {family} | {case} | {ratio:.3f}")
    key = (kernel, variant, family)
    if key not in _WORST or ratio > _WORST[key][0]:
        _WORST[key] = (ratio, case)
    assert ratio <= 1.0, f"{kernel} [{variant}] {family} {case}: error / bar = {ratio:.4g}; {where}"


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nnystrom-worst| kernel | variant | family | worst error / bar | at case")
    for (kernel, variant, family), (ratio, case) in sorted(_WORST.items()):
        print(f"nystrom-worst| {kernel} | {variant} | {family} | {ratio:.3f} | {case}")


# ---- the calls (shared with the child process) -----------------------------------------------------------------------------------------------------------------
def run_dwconv_seq(gpu, qkv, w, merged, n, d, taps):
    lib, b, H = _lib.lib(), O.DWCONV_B, O.DWCONV_H
    Cd = H * d
    q, wd, out = _dev(qkv, gpu), _dev(w, gpu), _Out(merged, gpu)
    _lib.check(lib.amds_dwconv_seq(q.data_ptr() + 2 * Cd * 4, n * 3 * Cd, d, 3 * Cd, wd.data_ptr(), out.ptr(), n * Cd, d, Cd, b, H, n, d, taps, _st()), "dwconv_seq")
    return O.head_slice(out.cpu(), 0, H, d)


def run_dwconv_seq_wgrad(gpu, qkv, merged, n, d, taps):
    lib, b, H = _lib.lib(), O.DWCONV_B, O.DWCONV_H
    Cd = H * d
    q, g, out = _dev(qkv, gpu), _dev(merged, gpu), _Out(torch.full((H, taps), MARK), gpu)
    nb = lib.amds_dwconv_seq_wgrad_workspace_bytes(b, H, taps)
    ws = _ws(gpu, nb)
    _lib.check(lib.amds_dwconv_seq_wgrad(g.data_ptr(), n * Cd, d, Cd, q.data_ptr() + 2 * Cd * 4, n * 3 * Cd, d, 3 * Cd, out.ptr(), b, H, n, d, taps, ws.data_ptr(), nb,
                                         _st()), "dwconv_seq_wgrad")
    return out.cpu()


def run_ppeg_wgrad(gpu, x, dy, B, Hh, Ww, C):
    lib = _lib.lib()
    xd, gd, out = _dev(x, gpu), _dev(dy, gpu), _Out(torch.full((50, C), MARK), gpu)
    nb = lib.amds_ppeg_wgrad_workspace_bytes(B, C)
    ws = _ws(gpu, nb)
    _lib.check(lib.amds_ppeg_wgrad(xd.data_ptr(), gd.data_ptr(), out.ptr(), B, Hh, Ww, C, ws.data_ptr(), nb, _st()), "ppeg_wgrad")
    return out.cpu()


# ---- softmax ---------------------------------------------------------------------------------------------------------------------------------------------
def _softmax_variant(cols, offset):
    if cols % 4 or cols > 2048 or offset % 4:
        return "block"
    return "wave<%d>" % next(nv for nv in (1, 2, 4, 5, 8) if cols <= 256 * nv)


def _softmax_case(gpu, rows, cols, offset):
    lib, variant = _lib.lib(), _softmax_variant(cols, offset)
    case = f"rows={rows} cols={cols}" + (" +1 float" if offset else "")
    for family in FAMILIES:
        x, _ = O.softmax_inputs(rows, cols, family)
        out = _Out(x, gpu, offset)
        _lib.check(lib.amds_softmax_rows(out.ptr(), rows, cols, _st()), "softmax_rows")
        _judge("amds_softmax_rows", variant, family, case, out.cpu(), O.softmax_rows(x)[0], None if family == "grid" else O.softmax_rows_bar(x))
        p, dp, _ = O.softmax_bwd_inputs(rows, cols, family)
        pd, out = _dev(p, gpu, offset), _Out(dp, gpu, offset)
        _lib.check(lib.amds_softmax_rows_bwd(pd.data_ptr(), out.ptr(), rows, cols, _st()), "softmax_rows_bwd")
        _judge("amds_softmax_rows_bwd", variant, family, case, out.cpu(), O.softmax_rows_bwd(p, dp)[0], None if family == "grid" else O.softmax_rows_bwd_bar(p, dp))
        assert torch.equal(pd.cpu(), p)


@pytest.mark.parametrize("cols", O.SOFTMAX_COLS)
def test_softmax_rows(gpu, cols):
    for rows in O.SOFTMAX_ROWS:
        _softmax_case(gpu, rows, cols, 0)


def test_softmax_rows_unaligned(gpu):
    _softmax_case(gpu, 5, 256, 1)


# ---- landmark means --------------------------------------------------------------------------------------------------------------------------------------
def _landmark_case(gpu, m, l, d, offset):
    lib, b, H = _lib.lib(), O.LANDMARK_B, O.LANDMARK_H
    Cd, n = H * d, m * l
    sb, sh, ld = n * 3 * Cd, d, 3 * Cd
    variant = "float4" if d % 4 == 0 and ld % 4 == 0 and offset % 4 == 0 and (Cd * 4) % 16 == 0 else "scalar"
    case = f"m={m} l={l} d={d}" + (" +1 float" if offset else "")
    for family in FAMILIES:
        qkv, dout, dx0, scale, _ = O.landmark_inputs(m, l, d, family)
        q, out = _dev(qkv, gpu, offset), _Out(torch.full((b, H, m, d), MARK), gpu, offset)
        _lib.check(lib.amds_landmark_mean(q.data_ptr() + Cd * 4, sb, sh, ld, out.ptr(), b, H, m, l, d, scale, _st()), "landmark_mean")          # k's slices
        ref, ab = O.landmark_mean(qkv, 1, H, d, m, l, scale)
        _judge("amds_landmark_mean", variant, family, case, out.cpu(), ref, None if family == "grid" else O.sum_bar(l, ab))
        for acc in (0, 1):
            g, out = _dev(dout, gpu, offset), _Out(dx0, gpu, offset)
            _lib.check(lib.amds_landmark_mean_bwd(g.data_ptr(), out.ptr() + Cd * 4, sb, sh, ld, b, H, m, l, d, scale, acc, _st()), "landmark_mean_bwd")
            ref, ab = O.landmark_mean_bwd(dout, dx0, 1, H, d, m, l, scale, acc)
            _judge("amds_landmark_mean_bwd", variant, family, f"{case} accumulate={acc}", out.cpu(), ref, None if family == "grid" else O.sum_bar(2, ab))


@pytest.mark.parametrize("m,l,d", O.LANDMARK_CASES)
def test_landmark_mean(gpu, m, l, d):
    _landmark_case(gpu, m, l, d, 0)


def test_landmark_mean_unaligned(gpu):
    _landmark_case(gpu, 35, 2, 8, 1)


# ---- the pinv start ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", O.PINV_N)
def test_pinv_init(gpu, n):
    lib = _lib.lib()
    variant = "absmax<2>" if n % 4 == 0 and n <= 256 else "absmax<8>" if n % 4 == 0 and n <= 1024 else "absmax_any"
    for family in FAMILIES:
        x = O.pinv_inputs(n, family)
        xd = _dev(x, gpu)
        for nmat, group in O.PINV_GROUPS:
            out, scratch = _Out(torch.full((nmat, n, n), MARK), gpu), _Out(torch.full((2 * (nmat // group),), MARK), gpu)
            _lib.check(lib.amds_pinv_init_grouped(xd.data_ptr(), out.ptr(), nmat, n, group, scratch.ptr(), _st()), "pinv_init_grouped")
            got = out.cpu()
            scratch.cpu()
            ref, ab = O.pinv_init(x, group)
            _judge("amds_pinv_init_grouped", variant, family, f"n={n} nmat={nmat} group={group}", got, ref, 2 * O.EPS * ab if family == "grid" else O.sum_bar(n, ab))
            if group == nmat:
                out, scratch = _Out(torch.full((nmat, n, n), MARK), gpu), _Out(torch.full((2,), MARK), gpu)
                _lib.check(lib.amds_pinv_init(xd.data_ptr(), out.ptr(), nmat, n, scratch.ptr(), _st()), "pinv_init")
                assert torch.equal(out.cpu(), got), "amds_pinv_init and amds_pinv_init_grouped(group = nmat) differ"
        assert torch.equal(xd.cpu(), x)


def _pinv_bwd_variant(n):
    return "stats<2>" if n % 32 == 0 and n <= 256 else "stats<8>" if n % 32 == 0 and n <= 1024 else "stats_any"


def _pinv_bwd_call(gpu, x, dz, dx0):
    lib = _lib.lib()
    nmat, n, _ = x.shape
    xd, gd, out = _dev(x, gpu), _dev(dz, gpu), _Out(dx0, gpu)
    nb = lib.amds_pinv_init_bwd_workspace_bytes(nmat)
    ws = _ws(gpu, nb)
    _lib.check(lib.amds_pinv_init_bwd(xd.data_ptr(), gd.data_ptr(), out.ptr(), nmat, n, ws.data_ptr(), nb, _st()), "pinv_init_bwd")
    return out.cpu()


@pytest.mark.parametrize("n", O.PINV_BWD_N)
def test_pinv_init_bwd(gpu, n):
    for family in FAMILIES:
        x, dz, dx0 = O.pinv_bwd_inputs(n, family)
        p = O.pinv_init_bwd_parts(x, dz, dx0)
        assert p["row_margin"] >= 1e-3 and p["col_margin"] >= 1e-3 and bool((x > 0).all())          # fp32 and fp64 then pick the same row and column
        bar = 8 * O.EPS * p["largest"] if family == "grid" else O.sum_bar(x.numel() + 4 * n, p["abs_sum"])
        _judge("amds_pinv_init_bwd", _pinv_bwd_variant(n), family, f"n={n} nmat={x.shape[0]}", _pinv_bwd_call(gpu, x, dz, dx0), p["value"], bar)


def test_pinv_init_bwd_tie(gpu):
    """Two bit-identical maximal rows and columns: the ds terms land on the FIRST of each, and only there."""
    x, dz, dx0, row, col = O.pinv_bwd_tie_inputs(32)
    p = O.pinv_init_bwd_parts(x, dz, dx0)
    assert (p["row"], p["col"]) == (row, col)
    got = _pinv_bwd_call(gpu, x, dz, dx0)
    _judge("amds_pinv_init_bwd", "stats<2>", "grid", "n=32 nmat=3 tie", got, p["value"], 8 * O.EPS * p["largest"])
    # the ds terms are far above the bar: the second row / column of each pair must not carry them
    plain = dx0.double() + dz.double().transpose(-1, -2) / p["s"]
    moved = (got.double() - plain).abs() > 8 * O.EPS * p["largest"]
    want = torch.zeros_like(moved)
    want.view(3 * 32, 32)[row] = True
    want[col // 32, :, col % 32] = True
    assert torch.equal(moved, want)


# ---- the sequence convolution ------------------------------------------------------------------------------------------------------------------------------------
def _dwconv_case(gpu, n, d, taps, variant):
    H = O.DWCONV_H
    for family in FAMILIES:
        qkv, w, merged, _ = O.dwconv_inputs(n, d, taps, family)
        ref, ab = O.dwconv_seq(O.head_slice(qkv, 2, H, d), w, O.head_slice(merged, 0, H, d))
        _judge("amds_dwconv_seq", variant, family, f"n={n} d={d} taps={taps}", run_dwconv_seq(gpu, qkv, w, merged, n, d, taps), ref,
               None if family == "grid" else O.sum_bar(taps + 1, ab))


@pytest.mark.parametrize("n", sorted({c[0] for c in O.DWCONV_WIN_CASES}))
def test_dwconv_seq_window(gpu, n):
    for n_, d, taps in O.DWCONV_WIN_CASES:
        if n_ == n:
            _dwconv_case(gpu, n, d, taps, "window<33,32>")


@pytest.mark.parametrize("taps", sorted({c[2] for c in O.DWCONV_GENERIC_CASES}))
def test_dwconv_seq_generic(gpu, taps):
    for n, d, taps_ in O.DWCONV_GENERIC_CASES:
        if taps_ == taps:
            _dwconv_case(gpu, n, d, taps, "generic")


@pytest.mark.parametrize("n,d", O.DWCONV_ROW_CASES)
def test_dwconv_seq_row(gpu, n, d):
    lib, b, H, taps = _lib.lib(), O.DWCONV_B, O.DWCONV_H, 33
    Cd = H * d
    for family in FAMILIES:
        qkv, w, merged, _ = O.dwconv_inputs(n, d, taps, family)
        out0 = merged[:, 0].reshape(b, H, d)
        q, wd = _dev(qkv, gpu), _dev(w, gpu)
        for row in sorted({0, n // 2, n - 1}):
            out = _Out(out0, gpu)
            _lib.check(lib.amds_dwconv_seq_row(q.data_ptr() + 2 * Cd * 4, n * 3 * Cd, d, 3 * Cd, wd.data_ptr(), out.ptr(), Cd, d, b, H, n, d, taps, row, _st()), "dwconv_seq_row")
            ref, ab = O.dwconv_seq_row(O.head_slice(qkv, 2, H, d), w, out0, row)
            _judge("amds_dwconv_seq_row", "row", family, f"n={n} d={d} row={row}", out.cpu(), ref, None if family == "grid" else O.sum_bar(taps + 1, ab))


def _wgrad_case(gpu, n, d, taps, variant):
    b, H = O.DWCONV_B, O.DWCONV_H
    for family in FAMILIES:
        qkv, _, merged, _ = O.dwconv_inputs(n, d, taps, family)
        ref, ab = O.dwconv_seq_wgrad(O.head_slice(merged, 0, H, d), O.head_slice(qkv, 2, H, d), taps)
        _judge("amds_dwconv_seq_wgrad", variant, family, f"n={n} d={d} taps={taps}", run_dwconv_seq_wgrad(gpu, qkv, merged, n, d, taps), ref,
               None if family == "grid" else O.sum_bar(b * n * d, ab))


@pytest.mark.parametrize("n", sorted({c[0] for c in O.WGRAD_WIN_CASES}))
def test_dwconv_seq_wgrad_window(gpu, n):
    for n_, d, taps in O.WGRAD_WIN_CASES:
        if n_ == n:
            _wgrad_case(gpu, n, d, taps, "window<33,16>")


@pytest.mark.parametrize("d", sorted({c[1] for c in O.WGRAD_GENERIC_CASES}))
def test_dwconv_seq_wgrad_generic(gpu, d):
    for n, d_, taps in O.WGRAD_GENERIC_CASES:
        if d_ == d:
            _wgrad_case(gpu, n, d, taps, "generic 256%d==0" if 256 % d == 0 else "generic flat")


# ---- PPEG ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hh,Ww", O.PPEG_GRIDS)
def test_ppeg(gpu, Hh, Ww):
    lib = _lib.lib()
    for C in O.PPEG_C:
        for B in O.PPEG_B:
            for family in FAMILIES:
                x, _, ws, bs, _ = O.ppeg_inputs(B, Hh, Ww, C, family)
                xd, wd, bd = _dev(x, gpu), [_dev(t, gpu) for t in ws], [_dev(t, gpu) for t in bs]
                out = _Out(torch.full(x.shape, MARK), gpu)
                _lib.check(lib.amds_ppeg(xd.data_ptr(), out.ptr(), wd[0].data_ptr(), bd[0].data_ptr(), wd[1].data_ptr(), bd[1].data_ptr(), wd[2].data_ptr(),
                                         bd[2].data_ptr(), B, Hh, Ww, C, _st()), "ppeg")
                got = out.cpu()
                ref, ab = O.ppeg(x, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], Hh, Ww)
                assert torch.equal(got[:, 0], x[:, 0]), "the class row is a copy"
                _judge("amds_ppeg", "ppeg_kernel", family, f"{Hh}x{Ww} C={C} B={B}", got, ref, None if family == "grid" else O.sum_bar(49 + 25 + 9 + 4, ab))


@pytest.mark.parametrize("Hh,Ww", O.PPEG_WGRAD_GRIDS)
def test_ppeg_wgrad(gpu, Hh, Ww):
    for C in O.PPEG_WGRAD_C:
        for B in O.PPEG_WGRAD_B:
            for family in FAMILIES:
                x, dy, _, _, _ = O.ppeg_inputs(B, Hh, Ww, C, family)
                ref, ab = O.ppeg_wgrad(x, dy, Hh, Ww)
                _judge("amds_ppeg_wgrad", "window<16>", family, f"{Hh}x{Ww} C={C} B={B}", run_ppeg_wgrad(gpu, x, dy, B, Hh, Ww, C), ref,
                       None if family == "grid" else O.sum_bar(B * Hh * Ww, ab))


# ---- the generic forms behind AMDS_DWCONV_WIN=0 (read once per process: a child) ------------------------------------------------------------------------------------
CHILD_SEQ = ((129, 72, 33), (17, 8, 33))
CHILD_WGRAD = ((65, 8, 33), (65, 72, 33), (16, 130, 33))
CHILD_PPEG = ((3, 3, 11, 70), (1, 2, 2, 257), (2, 2, 17, 130), (1, 1, 1, 4))          # (B, Hh, Ww, C)


def child_main(out_dir):
    """Runs in the child: the three kernels on integer-grid inputs -> <out_dir>/generic.npz."""
    gpu, out = torch.device("cuda:0"), {}
    for i, (n, d, taps) in enumerate(CHILD_SEQ):
        qkv, w, merged, _ = O.dwconv_inputs(n, d, taps, "grid")
        out[f"seq{i}"] = run_dwconv_seq(gpu, qkv, w, merged, n, d, taps).numpy()
    for i, (n, d, taps) in enumerate(CHILD_WGRAD):
        qkv, _, merged, _ = O.dwconv_inputs(n, d, taps, "grid")
        out[f"wgrad{i}"] = run_dwconv_seq_wgrad(gpu, qkv, merged, n, d, taps).numpy()
    for i, (B, Hh, Ww, C) in enumerate(CHILD_PPEG):
        x, dy, _, _, _ = O.ppeg_inputs(B, Hh, Ww, C, "grid")
        out[f"ppeg{i}"] = run_ppeg_wgrad(gpu, x, dy, B, Hh, Ww, C).numpy()
    np.savez(os.path.join(out_dir, "generic.npz"), **out)


def test_generic_forms_in_a_child_process(gpu, tmp_path):
    """AMDS_DWCONV_WIN=0 selects dwconv_seq_kernel and dwconv_seq_wgrad_kernel at taps = 33 and ppeg_wgrad_kernel: on integer grids they equal the fp64 reference bit for
    bit, and therefore the window kernels' results (test_dwconv_seq_window, test_dwconv_seq_wgrad_window, test_ppeg_wgrad hold those to the same reference)."""
    tests = str(Path(__file__).resolve().parent)
    code = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import test_gpu_nystrom_kernels as T; T.child_main(sys.argv[3])"
    subprocess.run([sys.executable, "-c", code, str(Path(tests).parent), tests, str(tmp_path)], check=True, env=dict(os.environ, AMDS_DWCONV_WIN="0"), timeout=300)
    z, H = np.load(tmp_path / "generic.npz"), O.DWCONV_H
    for i, (n, d, taps) in enumerate(CHILD_SEQ):
        qkv, w, merged, _ = O.dwconv_inputs(n, d, taps, "grid")
        ref, _ = O.dwconv_seq(O.head_slice(qkv, 2, H, d), w, O.head_slice(merged, 0, H, d))
        _judge("amds_dwconv_seq", "generic (AMDS_DWCONV_WIN=0)", "grid", f"n={n} d={d} taps={taps}", torch.from_numpy(z[f"seq{i}"]), ref)
    for i, (n, d, taps) in enumerate(CHILD_WGRAD):
        qkv, _, merged, _ = O.dwconv_inputs(n, d, taps, "grid")
        ref, _ = O.dwconv_seq_wgrad(O.head_slice(merged, 0, H, d), O.head_slice(qkv, 2, H, d), taps)
        _judge("amds_dwconv_seq_wgrad", ("generic 256%d==0" if 256 % d == 0 else "generic flat") + " (AMDS_DWCONV_WIN=0)", "grid", f"n={n} d={d} taps={taps}",
               torch.from_numpy(z[f"wgrad{i}"]), ref)
    for i, (B, Hh, Ww, C) in enumerate(CHILD_PPEG):
        x, dy, _, _, _ = O.ppeg_inputs(B, Hh, Ww, C, "grid")
        _judge("amds_ppeg_wgrad", "generic (AMDS_DWCONV_WIN=0)", "grid", f"{Hh}x{Ww} C={C} B={B}", torch.from_numpy(z[f"ppeg{i}"]), O.ppeg_wgrad(x, dy, Hh, Ww)[0])
