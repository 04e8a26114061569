"""Every dispatch variant of the fp32 batched product -- `amds_bgemm_f32`, `amds_bgemm_f32_dual` (stamp_amd/csrc/transmil.hip) and `amds_linear_f32` (gap.hip) -- against
fp64, through the C ABI, element by element.

References, inputs, bars and the case list: tests/bgemm_oracle.py (pinned on the CPU by test_cpu_bgemm_oracle.py, which also asserts that the cases below reach
every hipLaunchKernelGGL of `bgemm_f32_at` and `gemm_f32`).  Four operand families:

* grid  -- integers in [-4, 4], alpha in {1, -0.5, 2}, integer diag / bias / old C: every partial sum exact in fp32 and in the bf16 `hi` plane alone.  BIT FOR BIT
           equal to fp64 at "highest" and at "high".
* lo    -- one operand integers in [-4096, 4096] (hi + lo == a exactly, lo nonzero for ~80 %), the other in [-4, 4], then the roles swapped ("lo-swapped"); K <= 128.
           Bit for bit at both precisions: the family that sees a wrong lo image of `bgemm_x3_kernel` or a wrong split of `bgemm_f32_big_kernel<.., X3 = 1>`.
* real  -- Gaussian, A's rows scaled by 2^-3 .. 2^3, per element |got - ref| <= bar:
             "highest" (and every kernel that does not split):  (K + 5) * 2^-23 * abs_sum                                (bgemm_oracle.bar_highest)
             "high" on a splitting kernel, K <= 128:           (3 * 2^-16 + 3 (K + 2) * 2^-24) * abs_sum               (bgemm_oracle.bar_high)
           and at "high" the project's stated 2e-5 relative L2 per batch as well.  abs_sum = |alpha| sum_k |a||b| + |diag delta_mn| + |bias_n| + |old C|.
* chain -- ("highest") Gaussian operands with odd significands against the in-order fp32 fused-multiply-add chain over k, bit for bit, on one case per exact kernel; the
           oracle asserts that no step of any chain case is an fp32 tie of its fp64 emulation.

Outputs sit between two 64-float bands of a marker; the columns of a row beyond N (ldc > N) and every other float of the buffer that is no element of the product hold
the marker too, and all of it must survive the call.  Each check prints `bgemm| kernel | variant | family | case | error / bar` under -s (0.000 = bit-equal), and the
module ends with the worst figure per kernel, variant and family: profiles/bgemm_f32_kernel_errors.txt is that table from one run.

Which case group reaches which kernel (transmil.hip line of the launch; `bgemm_oracle.dispatch` restates the conditions of :1402-1481):

  fallback    M, N < 96, or K / pitch / stride / pointer not float4-loadable (:1402, :1406)
                (1,1,1) (64,64,32) (63,65,33) (95,95,31) (130,70,50); (128,128,32) with lda = K + 1, with A one float off, with a batch stride of 6 floats
                                                                    bgemm_f32_kernel<1 | 0>                                    :1482 | :1483
                "high" gives the bits of "highest" here (no split below the tiled kernels)
  boundary    K = 32, aligned: (95,95) -> fallback; (96,8) (96,64) -> 256 x 64; (8,96) (64,96) -> 64 x 256; (96,96) (97,65) (65,97) -> 128 x 128        (:1406, :1408)
  big-whole   one whole tile (128,128) (256,64) (64,256) x A B^T, A B, A^T B^T, A^T B:
                K = 16, 48    unchecked float4 loop (:276)          bgemm_f32_big_kernel<TB,TA,WM,WN,0> "highest"              :1435
                K = 4, 20, 36 checked float4 loop (:277, :186/:194)  bgemm_f32_big_kernel<TB,TA,WM,WN,1> "high" (K % 32 != 0)   :1433
  big-ragged  (129,127) (257,63) (255,64) (63,257), K = 20, diag 7 and 0, pitches rounded up to 4: edge tiles, the edge store forms (:302, :305)
  big-elem    A^T with a pitch that is no multiple of 4: (5,7,3) (130,70,50) (70,5,3) (5,70,3), (128,128,32) with lda = M + 1: element loader (vec = 0, :187/:195)
  x3          "high", whole tiles, K % 32 == 0 (:1447): the three shapes x four layouts x accumulate 0 | 1, K = 32 (one stage) and 96 (both LDS stages, odd count);
              (256,256) (512,64) (64,512); (128,128,1280): a long exact chain
                                                                    bgemm_x3_kernel<TB,TA,WM,WN,false,ACC>                     :1454 | :1451
              ("highest": the unchecked loop of the tiled kernel, :1435)
  epilogue    alpha {1, -0.5} x diag {0, 7} x bias {none, given} x accumulate {0, 1} on the fallback (63,65,33), a ragged (129,127,20) and an interior (128,128,16)
              tiled product and the x3 shape (128,128,32); every other case carries one mixed combination
  batch       (outer, inner) = (2, 3) q k^T on head slices of a packed [b][n][3 C] tensor; B shared through zero strides; C as a column window of a wider row;
              1, 3, 7, 8, 9, 13 tiles (and 4 x those) for the XCD re-mapping (:140-148, :351-359), distinct operands per slot and identical ones (all outputs bit-identical)
  dual        (128,128,32) (256,256,32)  bgemm_x3_kernel<0,0,2,2,true> "high" :1420, bgemm_f32_big_kernel<0,0,2,2,0,true> "highest" :1426;   K = 48 "high" and the
              ragged (130,70,52)  bgemm_f32_big_kernel<0,0,2,2,1,true> :1423;   B^T, A^T, (256,64,64): two calls (:1414-1416);   (40,40,40): the fallback twice
              (:1486 | :1487).  Each output per element, and its bits against two single calls.
  chain       the fallback on a pointer one float off, (128,128,256), the dual kernel; the fallback's (130,70,50) and the twelve tiled instances' K = 48 cases carry the
              chain family as well
  amds_linear_f32 (mil_small.hip:174 -> gemm_f32, gap.hip:73)        gemm_f32_kernel<1 | 0>                                     gap.hip:77 | :78
              M {1,63,64,65,130} x N {1,2,64,65} x K {1,3,6,32,33} and (130,512,768); K = 6: rows only 8-byte aligned under the float4 loader (gap.hip:39)
  child       AMDS_BGEMM_XCD=0 AMDS_BGEMM_X3_LDS=0 (read once per process): big-whole, x3 and batch again, grid and lo: launch order, the in-register split on aligned shapes
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import bgemm_oracle as O
from stamp_amd import _lib, ops

pytestmark = pytest.mark.gpu
F32 = torch.float32
BAND, MARK = 64, O.MARK
_WORST: dict = {}
_RECORDS: list = []


# ---- buffers -------------------------------------------------------------------------------------------------------------------------------------------------
def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, gpu, offset=0):
    """the flat fp32 array a on the device, `offset` floats off the allocation's (256-byte) alignment"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    buf = torch.empty(t.numel() + offset, dtype=F32, device=gpu)
    v = buf[offset:]
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * offset) % 16
    return v


class _Out:
    """A flat output buffer (pre-filled with c0: old values at the product's elements, MARK elsewhere) between two bands of MARK; `cpu()` checks the bands."""

    def __init__(self, c0, gpu):
        n = int(c0.size)
        self.buf = torch.full((2 * BAND + n,), MARK, dtype=F32, device=gpu)
        self.view = self.buf[BAND:BAND + n]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(c0, dtype=np.float32)))
        assert self.view.data_ptr() % 16 == 0

    def ptr(self, first=0):
        return self.view.data_ptr() + 4 * first

    def cpu(self):
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        assert bool((host[:BAND] == MARK).all()) and bool((host[-BAND:] == MARK).all()), "the call wrote outside its output"
        return host[BAND:-BAND].copy()


def _elements(flat, g, what):
    """the product's elements [outer, inner, M, N] out of the flat output; everything else of the buffer must still hold the marker"""
    idx = O.c_index(g)
    rest = np.ones(flat.size, dtype=bool)
    rest[idx.reshape(-1)] = False
    assert bool((flat[rest] == MARK).all()), f"{what}: wrote between the rows or batches of its output ({int((flat[rest] != MARK).sum())} floats)"
    return flat[idx]


def _judge(kernel, variant, family, case, got, ref, bar=None):
    """bar None: bit for bit.  Prints the figure, keeps the worst per (kernel, variant, family), then asserts."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and bool(np.isfinite(got).all()), f"{kernel} {variant} {case}: shape or non-finite output"
    err = np.abs(got - ref)
    if bar is None:
        ratio = 0.0 if bool((err == 0).all()) else float("inf")
        where = "" if ratio == 0.0 else (f"{int((err != 0).sum())} element(s) differ, first at {tuple(int(i) for i in np.argwhere(err != 0)[0])}, "
                                         f"largest difference {float(err.max()):.6g}")
    else:
        r = np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300))
        ratio = float(r.max())
        i = np.unravel_index(int(r.argmax()), r.shape)
        where = f"at {tuple(int(j) for j in i)}: got {float(got[i])!r} want {float(ref[i])!r}, error {float(err[i]):.6g}"
    print(f"bgemm| {kernel} | {variant} | {family} | {case} | {ratio:.3f}")
    key = (kernel, variant, family)
    if key not in _WORST or ratio > _WORST[key][0]:
        _WORST[key] = (ratio, case)
    _RECORDS.append((kernel, variant, family, case, ratio))
    assert ratio <= 1.0, f"{kernel} [{variant}] {family} {case}: error / bar = {ratio:.4g}; {where}"


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nbgemm-worst| kernel | variant | family | worst error / bar | at case")
    for (kernel, variant, family), (ratio, case) in sorted(_WORST.items()):
        print(f"bgemm-worst| {kernel} | {variant} | {family} | {ratio:.3f} | {case}")


# ---- the calls (shared with the child process) -----------------------------------------------------------------------------------------------------------------
def call_bgemm(gpu, g, op):
    """one amds_bgemm_f32 call on the flat buffers of `op`; -> (return code, flat output)"""
    A, B = _dev(op["A"], gpu, g.misA), _dev(op["B"], gpu, g.misB)
    bias = None if op["bias"] is None else _dev(op["bias"], gpu)
    out = _Out(op["c0"], gpu)
    rc = _lib.lib().amds_bgemm_f32(A.data_ptr() + 4 * g.a0, g.lda, g.sAo, g.sAi, B.data_ptr() + 4 * g.b0, g.ldb, g.sBo, g.sBi, g.flags, out.ptr(g.c0), g.ldc, g.sCo, g.sCi,
                                   g.outer, g.inner, g.M, g.N, g.K, op["alpha"], op["diag"], None if bias is None else bias.data_ptr(), op["accumulate"], _st())
    flat = out.cpu()
    assert np.array_equal(A.cpu().numpy(), op["A"]) and np.array_equal(B.cpu().numpy(), op["B"]), "an operand was written"
    return rc, flat


def call_dual(gpu, g, op, alpha2, diag2, second="own"):
    """one amds_bgemm_f32_dual call; second: "own" buffer, "same" (C2 == C) or "null" -> (return code, flat C, flat C2)"""
    A, B = _dev(op["A"], gpu, g.misA), _dev(op["B"], gpu, g.misB)
    o1, o2 = _Out(op["c0"], gpu), _Out(op["c0"], gpu)
    p2 = {"own": o2.ptr(g.c0), "same": o1.ptr(g.c0), "null": None}[second]
    rc = _lib.lib().amds_bgemm_f32_dual(A.data_ptr() + 4 * g.a0, g.lda, g.sAo, g.sAi, B.data_ptr() + 4 * g.b0, g.ldb, g.sBo, g.sBi, g.flags, o1.ptr(g.c0), p2, g.ldc, g.sCo, g.sCi,
                                        g.outer, g.inner, g.M, g.N, g.K, op["alpha"], op["diag"], alpha2, diag2, _st())
    return rc, o1.cpu(), o2.cpu()


def _label(launches):
    l = launches[0]
    name, args = l.kernel.split("<")
    return name, "<" + args + (" " + "+".join(sorted(l.loaders)) if l.loaders else "") + (" x2 launches" if len(launches) > 1 else "")


def _bar(case, precision, launches, family, ab):
    if family != "real":
        return None
    return O.bar_high(case.g.K, ab) if precision == "high" and any(O.is_split(l) for l in launches) else O.bar_highest(case.g.K, ab)


def _reference(case, family, op):
    """(value, abs_sum); the chain family's value is the fp32 chain"""
    ref, ab = O.reference(case, family, op)
    if family == "chain":
        ref, ties = O.chain(op["A"], op["B"], case.g)
        assert ties == 0
    return ref, ab


def run_case(gpu, case, precision, families=None, x3_lds=True, tag=""):
    """Every family of one amds_bgemm_f32 case at one precision (already set); -> {family: the product's elements}."""
    g, launches, out = case.g, case.launches(precision, x3_lds), {}
    kernel, variant = _label(launches)
    for family in case.families(precision, x3_lds):
        if families is not None and family not in families:
            continue
        op = O.operands(case, family)
        rc, flat = call_bgemm(gpu, g, op)
        _lib.check(rc, "bgemm_f32")
        what = f"{case.name} @{precision}{tag}"
        got = _elements(flat, g, what)
        ref, ab = _reference(case, family, op)
        _judge(kernel, variant + tag, family, what, got, ref, _bar(case, precision, launches, family, ab))
        if family == "real" and precision == "high":
            assert float(O.rel_l2(got, ref).max()) <= 2e-5, f"{what}: relative L2 {float(O.rel_l2(got, ref).max()):.3g} per batch"
        if case.name.endswith("identical"):
            assert bool((got == got[:1, :1]).all()), f"{what}: identical operands in every batch slot, different outputs"
        out[family] = got
    return out


def _run_group(gpu, group):
    for case in O.cases(group):
        if case.dual:          # test_bgemm_f32_dual
            continue
        got = {}
        for precision in O.PRECISIONS:
            with ops.float32_matmul_precision(precision):
                got[precision] = run_case(gpu, case, precision)
        if not any(O.is_split(l) for l in case.launches("high")):          # the fallback has no "high" form: the bits of "highest"
            for family, v in got["high"].items():
                assert np.array_equal(v, got["highest"][family]), f"{case.name} {family}: \"high\" changed the bits of a kernel that does not split"


@pytest.mark.parametrize("group", [g for g in O.GROUPS if g != "dual"])
def test_bgemm_f32(gpu, group):
    _run_group(gpu, group)


# ---- the two outputs of one product ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in O.CASES if c.dual])
def test_bgemm_f32_dual(gpu, name):
    (case,) = [c for c in O.CASES if c.name == name]
    g, (alpha2, diag2) = case.g, case.dual
    for precision in O.PRECISIONS:
        with ops.float32_matmul_precision(precision):
            launches = case.launches(precision)
            kernel, variant = _label(launches)
            for family in case.families(precision):
                op = O.operands(case, family)
                assert op["bias"] is None and not op["accumulate"]
                rc, f1, f2 = call_dual(gpu, g, op, alpha2, diag2)
                _lib.check(rc, "bgemm_f32_dual")
                what = f"{case.name} @{precision}"
                op2 = dict(op, alpha=alpha2, diag=diag2)
                for which, flat, o in (("C", f1, op), ("C2", f2, op2)):
                    got = _elements(flat, g, what)
                    ref, ab = _reference(case, family, o)
                    _judge(kernel, variant + " dual " + which, family, what, got, ref, _bar(case, precision, launches, family, ab))
                    rc, single = call_bgemm(gpu, g, o)
                    _lib.check(rc, "bgemm_f32")
                    assert np.array_equal(single, flat), f"{what} {family}: {which} of the dual call and the single call differ"


@pytest.mark.parametrize("second", ["same", "null"])
def test_bgemm_f32_dual_refuses_a_missing_or_aliased_second_output(gpu, second):
    case = next(c for c in O.CASES if c.dual)
    op = O.operands(case, "grid")
    rc, f1, f2 = call_dual(gpu, case.g, op, -1.0, 7.0, second)
    assert rc != 0 and np.array_equal(f1, op["c0"]) and np.array_equal(f2, op["c0"]), "refused calls write nothing"


# ---- rows depend on M only through the row class ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", O.ROW_CLASS_PAIRS, ids=lambda p: f"{p[0][0]}-{p[1][0]}x{p[0][1]}x{p[0][2]}")
def test_rows_are_the_same_bits_inside_a_row_class(gpu, pair):
    (M, N, K), (M2, _, _) = pair
    assert O.row_class(M) == O.row_class(M2) and M < M2
    for tb in (1, 0):
        small, large = O.Case("rowclass", f"{M}x{N}x{K} tb={tb}", O.geo(M, N, K, 0, tb), O.MIX_B), O.Case("rowclass", f"{M2}x{N}x{K} tb={tb}", O.geo(M2, N, K, 0, tb), O.MIX_B)
        for precision in O.PRECISIONS:
            assert [l.kernel for l in small.launches(precision)] == [l.kernel for l in large.launches(precision)]
            with ops.float32_matmul_precision(precision):
                for family in ("real", "lo"):
                    op2 = O.operands(large, family)
                    op = dict(op2, A=op2["A"][:small.g.nA].copy(), c0=np.full(small.g.nC, MARK, dtype=np.float32))          # the first M rows of the same operands
                    rows = []
                    for case, o in ((small, op), (large, op2)):
                        rc, flat = call_bgemm(gpu, case.g, o)
                        _lib.check(rc, "bgemm_f32")
                        got = _elements(flat, case.g, case.name)
                        ref, ab = O.reference(case, family, o)
                        launches = case.launches(precision)
                        _judge(*_label(launches), family, f"{case.name} @{precision}", got, ref, _bar(case, precision, launches, "real", ab) if family == "real" else None)
                        rows.append(got[0, 0, :M])
                    assert np.array_equal(rows[0], rows[1]), f"rows 0 .. {M - 1} of M = {M} and M = {M2} differ ({family}, {precision}, tb={tb})"


# ---- amds_linear_f32 -------------------------------------------------------------------------------------------------------------------------------------------
def call_linear(gpu, M, N, K, op, relu, null=None, out=None):
    x, w = _dev(op["A"], gpu), _dev(op["B"], gpu)
    bias = None if op["bias"] is None else _dev(op["bias"], gpu)
    out = out or _Out(np.full(max(M, 1) * N, MARK, dtype=np.float32), gpu)
    p = dict(x=x.data_ptr(), w=w.data_ptr(), out=out.ptr())
    if null:
        p[null] = None
    rc = _lib.lib().amds_linear_f32(p["x"], p["w"], None if bias is None else bias.data_ptr(), p["out"], M, N, K, relu, _st())
    return rc, out.cpu()


def _linear_case(gpu, M, N, K):
    for family, relu, bias in O.LINEAR_FORMS:
        case = O.linear_case(M, N, K, family, relu, bias)
        op = O.linear_operands(case, family, relu)
        rc, flat = call_linear(gpu, M, N, K, op, relu)
        _lib.check(rc, "linear_f32")
        got = flat.reshape(1, 1, M, N)
        ref, ab, pre = O.linear_reference(case, family, op, relu)
        if family == "grid":
            O.assert_exact(ab)
            if relu:
                assert pre[0, 0, 0, 0] == 0 and (N == 1 or pre[0, 0, 0, N - 1] == -3), "the planted zero and negative in front of the activation"
        if family == "chain":
            ref, ties = O.chain(op["A"], op["B"], case.g)
            assert ties == 0
        _judge("gemm_f32_kernel", f"<{relu}>", family, f"{M}x{N}x{K} bias={int(bias)}", got, ref, O.bar_highest(K, ab) if family == "real" else None)


@pytest.mark.parametrize("M", O.LINEAR_M)
def test_linear_f32(gpu, M):
    for N in O.LINEAR_N:
        for K in O.LINEAR_K:
            _linear_case(gpu, M, N, K)


def test_linear_f32_wide(gpu):
    _linear_case(gpu, *O.LINEAR_BIG)


def test_linear_f32_ignores_the_matmul_precision(gpu):
    case = O.linear_case(130, 65, 33, "real", 0, True)
    op = O.linear_operands(case, "real", 0)
    _, a = call_linear(gpu, 130, 65, 33, op, 0)
    with ops.float32_matmul_precision("high"):
        _, b = call_linear(gpu, 130, 65, 33, op, 0)
    assert np.array_equal(a, b)


def test_linear_f32_empty_and_refused_calls_write_nothing(gpu):
    case = O.linear_case(5, 3, 6, "grid", 0, True)
    op = O.linear_operands(case, "grid", 0)
    untouched = np.full(15, MARK, dtype=np.float32)
    rc, flat = call_linear(gpu, 0, 3, 6, op, 0, out=_Out(untouched, gpu))
    assert rc == 0 and np.array_equal(flat, untouched), "M = 0 is an empty call"
    for null in ("x", "w", "out"):
        rc, flat = call_linear(gpu, 5, 3, 6, op, 0, null=null)
        assert rc != 0 and np.array_equal(flat, untouched), f"null {null}"
    for M, N, K in ((-1, 3, 6), (5, 0, 6), (5, 3, 0), (5, -3, 6)):
        rc, flat = call_linear(gpu, M, N, K, op, 0, out=_Out(untouched, gpu))
        assert rc != 0 and np.array_equal(flat, untouched), (M, N, K)


# ---- one chain, three kernels -----------------------------------------------------------------------------------------------------------------------------------
def test_chain_is_the_same_bits_through_three_kernels(gpu):
    """(64,64,64): amds_linear_f32, the fallback (A one float off) and bgemm_f32_big_kernel<1,0,2,2,0> (as the first 64 x 64 block of (128,128,64)) all give the
    in-order fmaf chain, hence each other's bits."""
    big = O.Case("chain3", "128x128x64 ABt first block", O.geo(128, 128, 64), chain=True, seed=1)
    small = O.Case("chain3", "64x64x64 ABt A+1float", O.geo(64, 64, 64, misA=1), chain=True, seed=1)
    assert [l.kernel for l in big.launches("highest")] == ["bgemm_f32_big_kernel<1,0,2,2,0>"] and [l.kernel for l in small.launches("highest")] == ["bgemm_f32_kernel<1>"]
    opb = O.operands(big, "chain")
    ops_ = dict(opb, A=opb["A"][:64 * 64].copy(), B=opb["B"][:64 * 64].copy(), c0=np.full(64 * 64, MARK, dtype=np.float32))
    want, ties = O.chain(ops_["A"], ops_["B"], small.g)
    wantb, tiesb = O.chain(opb["A"], opb["B"], big.g)
    assert ties == 0 and tiesb == 0 and np.array_equal(wantb[0, 0, :64, :64], want[0, 0])
    with ops.float32_matmul_precision("highest"):
        rc, lin = call_linear(gpu, 64, 64, 64, ops_, 0)
        _lib.check(rc, "linear_f32")
        _judge("gemm_f32_kernel", "<0>", "chain", "64x64x64 shared chain", lin.reshape(64, 64), want[0, 0])
        rc, flat = call_bgemm(gpu, small.g, ops_)
        _lib.check(rc, "bgemm_f32")
        _judge(*_label(small.launches("highest")), "chain", "64x64x64 shared chain", _elements(flat, small.g, small.name), want)
        rc, flat = call_bgemm(gpu, big.g, opb)
        _lib.check(rc, "bgemm_f32")
        _judge(*_label(big.launches("highest")), "chain", "128x128x64 shared chain", _elements(flat, big.g, big.name), wantb)


# ---- launch order and the in-register split on aligned shapes: AMDS_BGEMM_XCD=0 AMDS_BGEMM_X3_LDS=0 (read once per process: a child) -----------------------------------
CHILD_FAMILIES = ("grid", "lo", "lo-swapped")
CHILD_TAG = " (XCD=0 X3_LDS=0)"


def _child_checks():
    return sum(1 for group in O.CHILD_GROUPS for case in O.cases(group) for p in O.PRECISIONS for f in case.families(p, x3_lds=False) if f in CHILD_FAMILIES)


def child_main(out_dir):
    """Runs in the child: the grid and lo families of the whole-tile and batching cases, judged bit for bit here -> <out_dir>/child.json"""
    gpu = torch.device("cuda:0")
    for group in O.CHILD_GROUPS:
        for case in O.cases(group):
            for precision in O.PRECISIONS:
                with ops.float32_matmul_precision(precision):
                    run_case(gpu, case, precision, CHILD_FAMILIES, x3_lds=False, tag=CHILD_TAG)
    with open(os.path.join(out_dir, "child.json"), "w") as f:
        json.dump(_RECORDS, f)


def test_launch_order_and_register_split_in_a_child_process(gpu, tmp_path):
    """With AMDS_BGEMM_X3_LDS=0 the aligned "high" products run bgemm_f32_big_kernel<.., X3 = 1> (its unchecked loop), with AMDS_BGEMM_XCD=0 every tiled kernel
    takes its tile from the launch order: on the integer families both equal fp64 bit for bit, and therefore the default path's results."""
    tests = Path(__file__).resolve().parent
    env = dict(os.environ, AMDS_BGEMM_XCD="0", AMDS_BGEMM_X3_LDS="0", PYTHONPATH=os.pathsep.join([str(tests.parent), str(tests)]))
    done = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(tmp_path)], env=env, timeout=300)
    if done.returncode != 0:
        pytest.fail(f"the child process ended with status {done.returncode}")
    records = json.loads((tmp_path / "child.json").read_text())
    assert len(records) == _child_checks() and len(records) > 300
    for kernel, variant, family, case, ratio in records:
        assert ratio == 0.0 and "x3_kernel" not in kernel and variant.endswith(CHILD_TAG)
        key = (kernel, variant, family)
        if key not in _WORST or ratio > _WORST[key][0]:
            _WORST[key] = (ratio, case)


if __name__ == "__main__":
    child_main(sys.argv[1])
