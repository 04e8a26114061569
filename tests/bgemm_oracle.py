"""Plain fp64 reference of the fp32 batched product behind `amds_bgemm_f32`, `amds_bgemm_f32_dual` and `amds_linear_f32` (stamp_amd/csrc/transmil.hip,
gap.hip), its rounding bars, the inputs of the direct tests and a restatement of the kernel choice (test_cpu_bgemm_oracle.py pins this file;
test_gpu_bgemm_kernels.py holds the kernels to it).  numpy / torch on the CPU; nothing here shares code with the kernels.

    C[zo, zi] = alpha * op(A[zo, zi]) op(B[zo, zi]) + diag * I + bias[n] (+ the old C when accumulate)

A product is described by a `Geo`: the flat buffers' pitches (`lda`, `ldb`, `ldc`), the element strides of the two batch levels (`sAo`, `sAi`, ...: 0 = a shared
operand), the offset of the first element in its buffer (`a0`, `b0`, `c0`: a head slice of a packed row, a column window) and how many floats the buffer sits off a
16-byte boundary (`misA`, ...).  `product` gathers the operands out of the FLAT buffers with exactly these numbers -- the ones that go to the C call -- so a stride
mistake in a test cannot cancel one in a kernel.

Operand families (`operands(case, family)`):

* grid  -- integers in [-4, 4] in A, B, bias and the old C, alpha in {1, -0.5, 2}, an integer diag.  Every product and partial sum is a multiple of 1/2 below
           2^24 * 1/2 (`assert_exact`: abs_sum < 2^24), so exact in fp32 in any order, fused or not; and every operand IS its bf16 `hi` (lo = 0), so the same holds
           for the three-MFMA product of "high".  The device must equal fp64 bit for bit at both precisions.
* lo    -- one operand integers in [-4096, 4096], the other in [-4, 4] (family "lo-swapped": roles exchanged), K <= 128.  bf16 keeps 8 significant bits: hi = the integer
           rounded to 8 bits, lo = a - hi is an integer of at most 4 bits, so hi + lo == a exactly and most lo are nonzero (`lo_fraction`); the small operand's lo is
           0, so lo * lo vanishes and hi * hi, lo * hi, hi * lo are exact.  abs_sum < 2^24 is asserted: bit for bit at both precisions.  A lo fragment taken from the
           wrong place, or a wrong split, changes integers.
* real  -- Gaussian, A's rows scaled by 2^k, k in [-3, 3]; judged per element by `bar_highest` / `bar_high`.
* chain -- Gaussian, alpha = 1 and no epilogue terms, against `chain`: the in-order fp32 fused-multiply-add chain over k = 0 .. K - 1 ("highest" only).
           `chain` cannot judge a step whose fp64 sum is an fp32 tie and every chain case must have none, no element excluded.  Plain Gaussian fp32 values meet
           about one tie per 10^6 steps: values with trailing zero bits give products that end exactly on the half-way bit.  So the lowest significand bit of every
           chain operand is set (a change of at most one ulp): a product of two odd 24-bit significands is odd in its last bit, far below the half-way bit, and a
           tie is left only where the fp64 sum itself rounds (2^-29 per step).  The remaining cases with a tie carry another `seed`.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np
import torch

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -23
EXACT = 2.0 ** 24
MARK = 24301.5            # what the unwritten parts of an output buffer hold
PRECISIONS = ("highest", "high")


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Geo:
    M: int
    N: int
    K: int
    transa: int = 0          # A stored [K][M]
    transb: int = 1          # B stored [N][K]
    outer: int = 1
    inner: int = 1
    lda: int = 0
    ldb: int = 0
    ldc: int = 0
    sAo: int = 0
    sAi: int = 0
    sBo: int = 0
    sBi: int = 0
    sCo: int = 0
    sCi: int = 0
    a0: int = 0
    b0: int = 0
    c0: int = 0
    misA: int = 0
    misB: int = 0
    nA: int = 0
    nB: int = 0
    nC: int = 0

    @property
    def Z(self):
        return self.outer * self.inner

    @property
    def flags(self):
        return self.transb | (self.transa << 1)


_TIGHT = object()


def geo(M, N, K, transa=0, transb=1, outer=1, inner=1, lda=None, ldb=None, ldc=None, sAo=_TIGHT, sAi=_TIGHT, sBo=_TIGHT, sBi=_TIGHT, sCo=_TIGHT, sCi=_TIGHT,
        a0=0, b0=0, c0=0, misA=0, misB=0, nC=0):
    """A Geo with the defaults of densely stacked matrices; the buffers are exactly as long as the last element read or written needs (nC: at least that)."""
    lda = lda or (M if transa else K)
    ldb = ldb or (K if transb else N)
    ldc = ldc or N
    ra, ca = (K, M) if transa else (M, K)
    rb, cb = (N, K) if transb else (K, N)
    sAi = ra * lda if sAi is _TIGHT else sAi
    sAo = inner * sAi if sAo is _TIGHT else sAo
    sBi = rb * ldb if sBi is _TIGHT else sBi
    sBo = inner * sBi if sBo is _TIGHT else sBo
    sCi = M * ldc if sCi is _TIGHT else sCi
    sCo = inner * sCi if sCo is _TIGHT else sCo
    nA = a0 + (outer - 1) * sAo + (inner - 1) * sAi + (ra - 1) * lda + ca
    nB = b0 + (outer - 1) * sBo + (inner - 1) * sBi + (rb - 1) * ldb + cb
    nCx = c0 + (outer - 1) * sCo + (inner - 1) * sCi + (M - 1) * ldc + N
    return Geo(M, N, K, transa, transb, outer, inner, lda, ldb, ldc, sAo, sAi, sBo, sBi, sCo, sCi, a0, b0, c0, misA, misB, nA, nB, max(nC, nCx))


def _batch(g, so, si):
    zo = np.arange(g.outer, dtype=np.int64).reshape(-1, 1, 1, 1)
    zi = np.arange(g.inner, dtype=np.int64).reshape(1, -1, 1, 1)
    return zo * so + zi * si


def a_index(g):
    """flat index of op(A)[zo, zi, m, k]"""
    m, k = np.arange(g.M, dtype=np.int64).reshape(1, 1, -1, 1), np.arange(g.K, dtype=np.int64).reshape(1, 1, 1, -1)
    return g.a0 + _batch(g, g.sAo, g.sAi) + (k * g.lda + m if g.transa else m * g.lda + k)


def b_index(g):
    """flat index of op(B)[zo, zi, k, n]"""
    k, n = np.arange(g.K, dtype=np.int64).reshape(1, 1, -1, 1), np.arange(g.N, dtype=np.int64).reshape(1, 1, 1, -1)
    return g.b0 + _batch(g, g.sBo, g.sBi) + (n * g.ldb + k if g.transb else k * g.ldb + n)


def c_index(g):
    m, n = np.arange(g.M, dtype=np.int64).reshape(1, 1, -1, 1), np.arange(g.N, dtype=np.int64).reshape(1, 1, 1, -1)
    return g.c0 + _batch(g, g.sCo, g.sCi) + m * g.ldc + n


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------------
def _terms(A, B, g, alpha, diag, bias, c_old, accumulate, absolute):
    f = np.abs if absolute else (lambda x: x)
    a = f(np.asarray(A, dtype=F64)[a_index(g)])
    b = f(np.asarray(B, dtype=F64)[b_index(g)])
    v = f(np.float64(alpha)) * np.matmul(a, b)
    if diag:
        v = v + f(np.float64(diag)) * np.eye(g.M, g.N)
    if bias is not None:
        v = v + f(np.asarray(bias, dtype=F64))[:g.N]
    if accumulate:
        v = v + f(np.asarray(c_old, dtype=F64)[c_index(g)])
    return v


def product(A, B, g, alpha=1.0, diag=0.0, bias=None, c_old=None, accumulate=0):
    """fp64 [outer, inner, M, N] from the flat buffers A, B (and the flat old C when accumulate); transa / transb and every pitch and stride are g's."""
    return _terms(A, B, g, alpha, diag, bias, c_old, accumulate, False)


def abs_sum(A, B, g, alpha=1.0, diag=0.0, bias=None, c_old=None, accumulate=0):
    """|alpha| sum_k |a||b| + |diag delta_mn| + |bias_n| + |c_old|, per element"""
    return _terms(A, B, g, alpha, diag, bias, c_old, accumulate, True)


def bar_highest(K, ab):
    """Exact-fp32 products: K fp32 fused multiply-adds, then alpha * acc, + diag, + bias and + old C -- at most K + 3 roundings, each of a partial result no larger
    than abs_sum, i.e. (K + 3) * 2^-24 * abs_sum to first order.  The bar is the project's `_sum_bar` form (tests/test_gpu_abi_rows.py), (n_terms + 2) * 2^-23 *
    abs_sum with n_terms = K + 3: twice the first-order bound, which covers the second-order terms and the fp64 reference's own 2^-53 K."""
    return (K + 5) * EPS * ab


def bar_high(K, ab):
    """bf16 x 3 products.  u = 2^-8 is bf16's unit roundoff (8 significant bits, round to nearest).  hi = bf16(a) misses a by at most u |a|; lo = bf16(a - hi) misses
    that remainder by at most u * u |a|: hi + lo = a (1 + e), |e| <= u^2 = 2^-16 -- one such factor per operand, 2 * 2^-16 |a||b| per term.  The product the kernels
    drop, lo_a * lo_b, is at most u |a| * u |b| = 2^-16 |a||b|.  Together 3 * 2^-16 * sum_k |a||b|.  What is kept -- lo hi, hi lo, hi hi -- are exact products
    of 8-bit numbers accumulated in fp32: 3 K accumulations, plus the epilogue's (alpha, diag, bias, old C: 3 more after the first), each rounding a partial result of
    at most abs_sum by 2^-24: 3 (K + 2) * 2^-24 * abs_sum."""
    return (3 * 2.0 ** -16 + 3 * (K + 2) * 2.0 ** -24) * ab


def rel_l2(got, ref):
    """relative L2 error per batch [outer, inner] (the project's stated 2e-5 for "high")"""
    d = np.asarray(got, dtype=F64) - ref
    return np.sqrt((d * d).sum((-1, -2)) / np.maximum((ref * ref).sum((-1, -2)), 1e-300))


def chain(A, B, g):
    """The in-order fp32 fused-multiply-add chain acc <- fma(a_k, b_k, acc), k = 0 .. K - 1, from acc = 0: ([outer, inner, M, N] fp32, ties).  One step is
    float32(float64(a) * float64(b) + float64(acc)): the product of two fp32 numbers is exact in fp64 (48 bits), the sum is rounded to fp64 and then to fp32.  That
    double rounding differs from the single rounding of a true fmaf only when the fp64 sum lies exactly half way between two fp32 numbers (its low 29 mantissa bits
    equal 1 << 28); `ties` counts such sums -- a chain case must have none."""
    a = np.asarray(A, dtype=F32)[a_index(g)].astype(F64)
    b = np.asarray(B, dtype=F32)[b_index(g)].astype(F64)
    acc = np.zeros((g.outer, g.inner, g.M, g.N), dtype=F32)
    ties = 0
    for k in range(g.K):
        s = a[..., :, k:k + 1] * b[..., k:k + 1, :] + acc.astype(F64)
        ties += int(((s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)).sum())
        acc = s.astype(F32)
    return acc, ties


def split_bf16(x):
    """fp32 -> (hi, lo) as the kernels split: hi = bf16(x), lo = bf16(x - hi), both returned as fp32"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F32))
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi.numpy(), lo.numpy()


def emulate_high(A, B, g, drop_lo_a=False):
    """The three-term sum of "high" with fp32 accumulation, k by k: acc += lo_a hi_b; acc += hi_a lo_b; acc += hi_a hi_b (each product of two 8-bit numbers is exact in
    fp32, each addition rounds): [outer, inner, M, N] fp32.  drop_lo_a: the mutant whose lo plane of A reads as zero."""
    ah, al = split_bf16(np.asarray(A, dtype=F32)[a_index(g)])
    bh, bl = split_bf16(np.asarray(B, dtype=F32)[b_index(g)])
    if drop_lo_a:
        al = np.zeros_like(al)
    acc = np.zeros((g.outer, g.inner, g.M, g.N), dtype=F32)
    for k in range(g.K):
        ka, kb = (Ellipsis, slice(None), slice(k, k + 1)), (Ellipsis, slice(k, k + 1), slice(None))
        acc = acc + al[ka] * bh[kb]
        acc = acc + ah[ka] * bl[kb]
        acc = acc + ah[ka] * bh[kb]
    assert acc.dtype == F32
    return acc


ROW_CLASS_PAIRS = (((256, 64, 64), (512, 64, 64)), ((128, 64, 64), (384, 64, 64)), ((100, 128, 64), (130, 128, 64)))          # (M, N, K) and (M', N, K)


def row_class(M):
    """`amds::bgemm_f32_row_class` (transmil.hip): what the kernel choice takes from the row count"""
    return int(M >= 96) | int(M <= 64) << 1 | int(M % 64 == 0) << 2 | int(M % 128 == 0) << 3 | int(M % 256 == 0) << 4


# ---- which kernel a call reaches: bgemm_f32_at (transmil.hip:1394-1491) and gemm_f32 (gap.hip:73-81), restated -----------------------------------------------------------
@dataclass(frozen=True)
class Launch:
    kernel: str              # name and template arguments
    line: int                # of the hipLaunchKernelGGL
    loaders: frozenset = frozenset()        # of its tiles: "fast" (unchecked float4), "vec4" (checked float4), "elem"
    stores: frozenset = frozenset()         # "inside" | "edge", + "+diag" with a nonzero diag
    tiles: int = 1

    @property
    def leaf(self):
        return (self.line, self.kernel)


# the hipLaunchKernelGGL sites of bgemm_f32_at in source order, (line, text of the kernel's name there), and gemm_f32's
LAUNCH_SITES = ((1420, "bgemm_x3_kernel<0, 0, 2, 2, true>"), (1423, "bgemm_f32_big_kernel<0, 0, 2, 2, 1, true>"), (1426, "bgemm_f32_big_kernel<0, 0, 2, 2, 0, true>"),
                (1433, "bgemm_f32_big_kernel<TB, TA, WM_, WN_, 1>"), (1435, "bgemm_f32_big_kernel<TB, TA, WM_, WN_, 0>"),
                (1451, "bgemm_x3_kernel<TB, TA, WM_, WN_, false, true>"), (1454, "bgemm_x3_kernel<TB, TA, WM_, WN_, false, false>"),
                (1482, "bgemm_f32_kernel<1>"), (1483, "bgemm_f32_kernel<0>"), (1486, "bgemm_f32_kernel<1>"), (1487, "bgemm_f32_kernel<0>"))
LINEAR_LAUNCH_SITES = ((77, "gemm_f32_kernel<1>"), (78, "gemm_f32_kernel<0>"))


def vec_ok(g):
    return (g.K % 4 == 0 and g.lda % 4 == 0 and g.ldb % 4 == 0 and g.sAo % 4 == 0 and g.sAi % 4 == 0 and g.sBo % 4 == 0 and g.sBi % 4 == 0
            and (g.misA + g.a0) % 4 == 0 and (g.misB + g.b0) % 4 == 0)


def tile_shape(g):
    """(index, BM, BN): 1 = 256 x 64 (N <= 64 < M), 2 = 64 x 256 (M <= 64 < N), 0 = 128 x 128"""
    s = 1 if (g.N <= 64 and g.M > 64) else 2 if (g.M <= 64 and g.N > 64) else 0
    return s, (128, 256, 64)[s], (128, 64, 256)[s]


def dispatch(g, precision, diag=0.0, accumulate=0, dual=None, x3_lds=True):
    """The launches of one amds_bgemm_f32 (dual = (alpha2, diag2): amds_bgemm_f32_dual) call, in order."""
    v, x3 = vec_ok(g), precision != "highest"
    tb, ta = g.transb, g.transa
    if ta or (v and (g.M >= 96 or g.N >= 96)):
        s, bm, bn = tile_shape(g)
        wm, wn = ((2, 2), (4, 1), (1, 4))[s]
        if dual and (tb or ta or s != 0):
            return dispatch(g, precision, diag, 0, None, x3_lds) + dispatch(g, precision, dual[1], 0, None, x3_lds)
        gy, gx = -(-g.M // bm), -(-g.N // bn)
        tiles = gx * gy * g.Z
        whole = v and g.M % bm == 0 and g.N % bn == 0 and g.K % 32 == 0
        loaders, stores = set(), set()
        for by in range(gy):
            for bx in range(gx):
                interior = by * bm + bm <= g.M and bx * bn + bn <= g.N
                loaders.add("fast" if v and interior and g.K % 16 == 0 else "vec4" if v else "elem")
                stores.add(("inside" if interior else "edge") + ("+diag" if diag != 0 else ""))
        loaders, stores = frozenset(loaders), frozenset(stores)
        if dual:
            if x3 and v and g.M % 128 == 0 and g.N % 128 == 0 and g.K % 32 == 0:
                return [Launch("bgemm_x3_kernel<0,0,2,2,true,false>", 1420, frozenset({"x3"}), stores, tiles)]
            if x3:
                return [Launch("bgemm_f32_big_kernel<0,0,2,2,1,true>", 1423, loaders, stores, tiles)]
            return [Launch("bgemm_f32_big_kernel<0,0,2,2,0,true>", 1426, loaders, stores, tiles)]
        if x3 and x3_lds and whole:
            return [Launch(f"bgemm_x3_kernel<{tb},{ta},{wm},{wn},false,{'true' if accumulate else 'false'}>", 1451 if accumulate else 1454, frozenset({"x3"}), stores, tiles)]
        return [Launch(f"bgemm_f32_big_kernel<{tb},{ta},{wm},{wn},{1 if x3 else 0}>", 1433 if x3 else 1435, loaders, stores, tiles)]
    tiles = -(-g.M // 64) * -(-g.N // 64) * g.Z
    first = [Launch(f"bgemm_f32_kernel<{tb}>", 1482 if tb else 1483, tiles=tiles)]
    return first + ([Launch(f"bgemm_f32_kernel<{tb}>", 1486 if tb else 1487, tiles=tiles)] if dual else [])


def dispatch_linear(relu):
    return [Launch(f"gemm_f32_kernel<{1 if relu else 0}>", 77 if relu else 78)]


def all_leaves(precision):
    """Every hipLaunchKernelGGL of bgemm_f32_at (and, at "highest", of gemm_f32) that the precision can reach."""
    x3 = precision != "highest"
    out = {(1482, "bgemm_f32_kernel<1>"), (1483, "bgemm_f32_kernel<0>"), (1486, "bgemm_f32_kernel<1>"), (1487, "bgemm_f32_kernel<0>")}
    for tb in (0, 1):
        for ta in (0, 1):
            for wm, wn in ((2, 2), (4, 1), (1, 4)):
                out.add((1433 if x3 else 1435, f"bgemm_f32_big_kernel<{tb},{ta},{wm},{wn},{1 if x3 else 0}>"))
                if x3:
                    out.add((1451, f"bgemm_x3_kernel<{tb},{ta},{wm},{wn},false,true>"))
                    out.add((1454, f"bgemm_x3_kernel<{tb},{ta},{wm},{wn},false,false>"))
    if x3:
        out |= {(1420, "bgemm_x3_kernel<0,0,2,2,true,false>"), (1423, "bgemm_f32_big_kernel<0,0,2,2,1,true>")}
    else:
        out |= {(1426, "bgemm_f32_big_kernel<0,0,2,2,0,true>"), (77, "gemm_f32_kernel<1>"), (78, "gemm_f32_kernel<0>")}
    return out


def is_split(launch):
    """the kernel takes its operands as hi + lo bf16"""
    k = launch.kernel
    return k.startswith("bgemm_x3_kernel") or (k.startswith("bgemm_f32_big_kernel") and k.split("<")[1].split(",")[4].rstrip(">") == "1")


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Epi:
    alpha: float = 1.0
    diag: float = 0.0
    bias: bool = False
    acc: int = 0

    def __str__(self):
        return f"alpha={self.alpha:g} diag={self.diag:g} bias={int(self.bias)} acc={self.acc}"


MIX_A = Epi(-0.5, 7.0, True, 1)
MIX_B = Epi(2.0, 0.0, True, 0)
PLAIN = Epi()
EPILOGUES = tuple(Epi(a, d, b, c) for a in (1.0, -0.5) for d in (0.0, 7.0) for b in (False, True) for c in (0, 1))


@dataclass(frozen=True)
class Case:
    group: str
    name: str
    g: Geo
    epi: Epi = PLAIN
    chain: bool = False                    # also runs the chain family (at "highest")
    dual: tuple | None = None              # (alpha2, diag2) of amds_bgemm_f32_dual
    seed: int = 0

    def families(self, precision, x3_lds=True):
        """grid everywhere, real too (at "high" on a splitting kernel: K <= 128); lo where "high" reaches a kernel that splits (and then at both precisions); chain where flagged, at "highest"."""
        split = any(is_split(l) for l in dispatch(self.g, "high", self.epi.diag, self.epi.acc, self.dual, x3_lds))
        f = ["grid"]
        if precision == "highest" or not split or self.g.K <= 128:          # bar_high separates a lost lo plane from rounding only at small K
            f.append("real")
        if split and self.g.K <= 128:
            f += ["lo", "lo-swapped"]
        if self.chain and precision == "highest":
            f.append("chain")
        return tuple(f)

    def launches(self, precision, x3_lds=True):
        return dispatch(self.g, precision, self.epi.diag, self.epi.acc, self.dual, x3_lds)


LAYOUTS = ((0, 1), (0, 0), (1, 1), (1, 0))          # (transa, transb)
WHOLE = ((128, 128), (256, 64), (64, 256))          # one tile of each shape


def _r4(x):
    return (x + 3) // 4 * 4


def _lay(ta, tb):
    return f"{'At' if ta else 'A'}{'Bt' if tb else 'B'}"


def _build_cases():
    c = []

    def add(group, name, g, epi=PLAIN, **kw):
        c.append(Case(group, name, g, epi, **kw))

    # the 64 x 64 fallback: products below 96 x 96, or not float4-loadable
    for tb in (1, 0):
        t = f"tb={tb}"
        for i, (M, N, K) in enumerate(((1, 1, 1), (64, 64, 32), (63, 65, 33), (95, 95, 31), (130, 70, 50))):
            add("fallback", f"{M}x{N}x{K} {t}", geo(M, N, K, 0, tb), (MIX_A, MIX_B)[i & 1], chain=(M, N, K) == (130, 70, 50))
        add("fallback", f"128x128x32 lda=K+1 {t}", geo(128, 128, 32, 0, tb, lda=33), MIX_A)
        add("fallback", f"128x128x32 A+1float {t}", geo(128, 128, 32, 0, tb, misA=1), MIX_B)
        add("fallback", f"128x128x32 Z=3 sAi=6 {t}", geo(128, 128, 32, 0, tb, inner=3, sAi=6), MIX_A)
    # the choice boundaries at 95 / 96 / 97 and 64 / 65
    for i, (M, N) in enumerate(((95, 95), (96, 8), (96, 64), (8, 96), (64, 96), (96, 96), (97, 65), (65, 97))):
        for tb in (1, 0):
            add("boundary", f"{M}x{N}x32 tb={tb}", geo(M, N, 32, 0, tb, ldb=None if tb else _r4(N)), (MIX_A, MIX_B)[i & 1])
    # the tiled kernel: whole tiles (unchecked loop at K % 16 == 0, checked float4 loop otherwise), ragged tiles, element loader
    for ta, tb in LAYOUTS:
        L = _lay(ta, tb)
        for M, N in WHOLE:
            for K, epi in ((16, MIX_B), (48, MIX_A), (4, MIX_A), (20, MIX_B), (36, MIX_A)):
                add("big-whole", f"{M}x{N}x{K} {L}", geo(M, N, K, ta, tb), epi, chain=K == 48)
        for M, N in ((129, 127), (257, 63), (255, 64), (63, 257)):
            for epi in (Epi(1.0, 7.0, False, 0), MIX_B):
                add("big-ragged", f"{M}x{N}x20 {L} {epi}", geo(M, N, 20, ta, tb, lda=_r4(M) if ta else None, ldb=None if tb else _r4(N)), epi)
    for tb in (1, 0):
        for i, (M, N, K) in enumerate(((5, 7, 3), (130, 70, 50), (70, 5, 3), (5, 70, 3))):
            add("big-elem", f"{M}x{N}x{K} At tb={tb}", geo(M, N, K, 1, tb), (MIX_A, MIX_B)[i & 1])
        add("big-elem", f"128x128x32 At lda=M+1 tb={tb}", geo(128, 128, 32, 1, tb, lda=129), MIX_A)
    # "high", whole aligned tiles, K % 32 == 0: the kernel that splits on the way into LDS (at "highest": the tiled kernel's unchecked loop)
    for ta, tb in LAYOUTS:
        L = _lay(ta, tb)
        for M, N in WHOLE:
            for K in (32, 96):
                for acc in (0, 1):
                    add("x3", f"{M}x{N}x{K} {L} acc={acc}", geo(M, N, K, ta, tb), Epi(-0.5 if acc else 2.0, 7.0 if K == 32 else 0.0, True, acc))
        for M, N in ((256, 256), (512, 64), (64, 512)):
            add("x3", f"{M}x{N}x32 {L}", geo(M, N, 32, ta, tb), MIX_A)
    add("x3", "128x128x1280 ABt long exact chain", geo(128, 128, 1280), MIX_A)
    # the epilogue: all 16 combinations on one case per kernel
    for epi in EPILOGUES:
        add("epilogue", f"fallback 63x65x33 {epi}", geo(63, 65, 33), epi)
        add("epilogue", f"ragged 129x127x20 {epi}", geo(129, 127, 20), epi)
        add("epilogue", f"interior 128x128x16 {epi}", geo(128, 128, 16), epi)
        add("epilogue", f"x3 128x128x32 {epi}", geo(128, 128, 32), epi)
    # batching and addressing
    for n, d in ((130, 32), (128, 32)):
        Cd = 3 * d          # b = 2 bags, 3 heads: q k^T on the head slices of a packed [b][n][3 Cd] tensor
        add("batch", f"qk^T n={n} d={d} (2,3) packed", geo(n, n, d, 0, 1, 2, 3, lda=3 * Cd, ldb=3 * Cd, sAo=n * 3 * Cd, sAi=d, sBo=n * 3 * Cd, sBi=d, b0=Cd), MIX_A)
    add("batch", "128x128x32 (2,2) B shared", geo(128, 128, 32, 0, 1, 2, 2, sBo=0, sBi=0), MIX_B)
    add("batch", "128x128x32 (2,2) AB, B shared", geo(128, 128, 32, 0, 0, 2, 2, sBo=0, sBi=0), MIX_A)
    add("batch", "128x128x32 C window ldc=N+24", geo(128, 128, 32, 0, 1, 1, 2, ldc=152, c0=8, nC=2 * 128 * 152), MIX_A)
    add("batch", "130x70x20 C window ldc=N+3", geo(130, 70, 20, 0, 1, 1, 2, ldc=73, c0=2, nC=2 * 130 * 73), MIX_A)
    add("batch", "63x65x33 C window ldc=N+3", geo(63, 65, 33, 0, 1, 2, 1, ldc=68, c0=1, nC=2 * 63 * 68), MIX_A)
    for outer, inner in ((1, 1), (3, 1), (7, 1), (2, 4), (3, 3), (13, 1)):          # 1, 3, 7, 8, 9, 13 tiles for the XCD re-mapping
        Z = outer * inner
        add("batch", f"128x128x32 Z={Z} distinct", geo(128, 128, 32, 0, 1, outer, inner), MIX_A)
        add("batch", f"128x128x32 Z={Z} identical", geo(128, 128, 32, 0, 1, outer, inner, sAo=0, sAi=0, sBo=0, sBi=0), MIX_B)
        add("batch", f"129x127x20 Z={Z} distinct, 4 tiles each", geo(129, 127, 20, 0, 1, outer, inner), MIX_B)
    add("batch", "256x384x32 AB 6 tiles", geo(256, 384, 32, 0, 0), MIX_A)
    add("batch", "384x128x32 Z=3 9 tiles", geo(384, 128, 32, 0, 1, 3, 1), MIX_B)
    add("batch", "512x64x32 Z=5 10 tiles of 256x64", geo(512, 64, 32, 0, 1, 5, 1), MIX_A)
    # the two outputs of one product
    D = (-1.0, 7.0)
    for M, N, K in ((128, 128, 32), (256, 256, 32), (128, 128, 48)):
        add("dual", f"{M}x{N}x{K} AB Z=3", geo(M, N, K, 0, 0, 3, 1), Epi(0.5, 0.0), dual=D)
    add("dual", "130x70x52 AB ldb=72", geo(130, 70, 52, 0, 0, 2, 1, ldb=72), Epi(0.5, 3.0), dual=D)
    add("dual", "128x128x32 ABt (two calls)", geo(128, 128, 32, 0, 1), Epi(0.5, 0.0), dual=D)
    add("dual", "128x128x32 AtB (two calls)", geo(128, 128, 32, 1, 0), Epi(0.5, 0.0), dual=D)
    add("dual", "256x64x64 AB (two calls)", geo(256, 64, 64, 0, 0), Epi(0.5, 0.0), dual=D)
    add("dual", "40x40x40 AB (fallback twice)", geo(40, 40, 40, 0, 0, 2, 1), Epi(0.5, 0.0), dual=D)
    add("dual", "40x40x40 ABt (fallback twice)", geo(40, 40, 40, 0, 1, 2, 1), Epi(0.5, 0.0), dual=D)
    # the fmaf chain on the remaining "highest" kernels (the fallback's and the tiled kernels' are flagged above)
    add("chain", "64x64x64 A+1float tb=1", geo(64, 64, 64, 0, 1, misA=1), chain=True, seed=1)
    add("chain", "64x64x64 A+1float tb=0", geo(64, 64, 64, 0, 0, misA=1), chain=True, seed=1)
    add("chain", "128x128x256 ABt", geo(128, 128, 256), chain=True, seed=1)
    add("chain", "128x128x64 AB Z=2 dual", geo(128, 128, 64, 0, 0, 2, 1), Epi(1.0, 0.0), dual=(1.0, 0.0), chain=True)
    names = [x.name for x in c]
    assert len(set(names)) == len(names), "case names are the seeds: they must be unique"
    return tuple(c)


CASES = _build_cases()
GROUPS = tuple(dict.fromkeys(x.group for x in CASES))
CHILD_GROUPS = ("big-whole", "x3", "batch")          # re-run with AMDS_BGEMM_XCD=0 AMDS_BGEMM_X3_LDS=0, grid and lo


def cases(group):
    return [x for x in CASES if x.group == group]


def _rng(case, family):
    return np.random.default_rng([zlib.crc32(case.name.encode()), zlib.crc32(family.encode()), case.seed])


def operands(case, family):
    """-> dict(A, B flat fp32; bias [N] fp32 or None; c0 flat fp32 = the output buffer before the call, MARK outside the product's elements; alpha, diag, accumulate).
    The old C values are there whether or not the call accumulates: a product without the flag must overwrite them."""
    g, e, r = case.g, case.epi, _rng(case, family)
    if family in ("grid", "lo", "lo-swapped"):
        small = lambda n: r.integers(-4, 5, n).astype(F32)
        big = lambda n: r.integers(-4096, 4097, n).astype(F32)
        A = (big if family == "lo" else small)(g.nA)
        B = (big if family == "lo-swapped" else small)(g.nB)
        bias, old = small(g.N), small(g.Z * g.M * g.N)
    else:
        A, B = r.standard_normal(g.nA).astype(F32), r.standard_normal(g.nB).astype(F32)
        if family == "real":
            i = np.arange(g.nA)
            A = A * np.exp2(((i % g.lda if g.transa else i // g.lda) % 7) - 3).astype(F32)
        else:          # chain: odd significands (see the module docstring)
            A, B = (A.view(np.uint32) | np.uint32(1)).view(F32), (B.view(np.uint32) | np.uint32(1)).view(F32)
        bias, old = r.standard_normal(g.N).astype(F32), r.standard_normal(g.Z * g.M * g.N).astype(F32)
    c0 = np.full(g.nC, MARK, dtype=F32)
    c0[c_index(g).reshape(-1)] = old
    if family == "chain":
        return dict(A=A, B=B, bias=None, c0=c0, alpha=1.0, diag=0.0, accumulate=0)
    return dict(A=A, B=B, bias=bias if e.bias else None, c0=c0, alpha=e.alpha, diag=e.diag, accumulate=e.acc)


def reference(case, family, op):
    """(value, abs_sum) [outer, inner, M, N] fp64 of the call `operands` describes"""
    args = (op["A"], op["B"], case.g, op["alpha"], op["diag"], op["bias"], op["c0"], op["accumulate"])
    return product(*args), abs_sum(*args)


def assert_exact(ab):
    """grid and lo: every partial sum is an integer multiple of 1/2 (alpha = -0.5) below 2^24 -- representable in fp32 however the sum is ordered or fused"""
    assert float(ab.max()) < EXACT, f"abs_sum {float(ab.max())} is not below 2^24"


def lo_fraction(x):
    """share of values whose bf16 lo part is nonzero, and whether hi + lo == x exactly for all of them"""
    hi, lo = split_bf16(x)
    return float((lo != 0).mean()), bool((hi.astype(F64) + lo.astype(F64) == np.asarray(x, dtype=F64)).all())


# ---- amds_linear_f32: out = act(x W^T + bias), x [M][K], W [N][K], all dense -----------------------------------------------------------------------------------------
LINEAR_M, LINEAR_N, LINEAR_K = (1, 63, 64, 65, 130), (1, 2, 64, 65), (1, 3, 6, 32, 33)
LINEAR_BIG = (130, 512, 768)
LINEAR_FORMS = (("grid", 1, True), ("grid", 0, False), ("real", 0, True), ("real", 1, False), ("chain", 0, False))          # (family, relu, bias given)


def linear_case(M, N, K, family, relu, bias):
    return Case("linear", f"{M}x{N}x{K} relu={relu} bias={int(bias)}", geo(M, N, K), Epi(1.0, 0.0, bias, 0), chain=family == "chain", seed=relu)


def linear_operands(case, family, relu):
    """as `operands`; the ReLU grid plants an exact zero (x's row 0 is zero, bias[0] = 0) and, from N = 2, a negative (bias[N - 1] = -3) in front of the activation"""
    op = operands(case, family)
    if family == "grid" and relu:
        op["A"][:case.g.K] = 0
        if op["bias"] is not None:
            op["bias"][0] = 0
            op["bias"][-1] = -3 if case.g.N > 1 else 0
    return op


def linear_reference(case, family, op, relu):
    v, ab = reference(case, family, op)
    return (np.maximum(v, 0) if relu else v), ab, v
