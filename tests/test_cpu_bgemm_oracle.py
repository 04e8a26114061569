"""Pins tests/bgemm_oracle.py, the reference test_gpu_bgemm_kernels.py holds the fp32 batched products to: the strided fp64 product against torch.matmul on
strided views, the exactness of the grid and lo families and the tie-free chains on every case the GPU module lists, the "high" bar against an fp32-accumulate
emulation of the three-term sum (held by the emulation, exceeded 4 x by one that drops A's lo plane), and the kernel each case is expected to reach: a restatement
of bgemm_f32_at's conditions whose leaves must cover every hipLaunchKernelGGL of bgemm_f32_at and gemm_f32."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import bgemm_oracle as O

CSRC = Path(__file__).resolve().parent.parent / "stamp_amd" / "csrc"


def _views(A, B, g):
    """op(A) [outer, inner, M, K] and op(B) [outer, inner, K, N] as torch strided views of the flat buffers"""
    a = torch.as_strided(torch.from_numpy(A).double(), (g.outer, g.inner, g.M, g.K), (g.sAo, g.sAi) + ((1, g.lda) if g.transa else (g.lda, 1)), g.a0)
    b = torch.as_strided(torch.from_numpy(B).double(), (g.outer, g.inner, g.K, g.N), (g.sBo, g.sBi) + ((1, g.ldb) if g.transb else (g.ldb, 1)), g.b0)
    return a, b


@pytest.mark.parametrize("group", O.GROUPS)
def test_product_is_torch_matmul_on_strided_views(group):
    for case in O.cases(group):
        g = case.g
        for family in ("grid", "real"):
            op = O.operands(case, family)
            a, b = _views(op["A"], op["B"], g)
            want = op["alpha"] * torch.matmul(a, b) + op["diag"] * torch.eye(g.M, g.N, dtype=torch.float64)
            wabs = abs(op["alpha"]) * torch.matmul(a.abs(), b.abs()) + abs(op["diag"]) * torch.eye(g.M, g.N, dtype=torch.float64)
            if op["bias"] is not None:
                want, wabs = want + torch.from_numpy(op["bias"]).double(), wabs + torch.from_numpy(op["bias"]).double().abs()
            old = torch.as_strided(torch.from_numpy(op["c0"]).double(), (g.outer, g.inner, g.M, g.N), (g.sCo, g.sCi, g.ldc, 1), g.c0)
            assert bool((old != O.MARK).all()) and int((torch.from_numpy(op["c0"]) != O.MARK).sum()) == g.Z * g.M * g.N          # the old values, and the marker everywhere else
            if op["accumulate"]:
                want, wabs = want + old, wabs + old.abs()
            ref, ab = O.reference(case, family, op)
            tol = 0 if family == "grid" else 1e-12 * float(wabs.max())
            assert float((torch.from_numpy(ref) - want).abs().max()) <= tol, case.name
            assert float((torch.from_numpy(ab) - wabs).abs().max()) <= tol, case.name


def test_index_maps_stay_inside_the_buffers_and_outputs_do_not_overlap():
    for case in O.CASES:
        g = case.g
        ia, ib, ic = O.a_index(g), O.b_index(g), O.c_index(g)
        assert ia.min() >= 0 and ia.max() == g.nA - 1 and ib.min() >= 0 and ib.max() == g.nB - 1 and ic.min() >= 0 and ic.max() < g.nC, case.name
        assert np.unique(ic).size == ic.size, case.name


@pytest.mark.parametrize("group", O.GROUPS)
def test_grid_and_lo_are_exact_on_every_case(group):
    for case in O.cases(group):
        fams = set(case.families("highest")) | set(case.families("high")) | set(case.families("high", x3_lds=False))
        for family in sorted(fams & {"grid", "lo", "lo-swapped"}):
            op = O.operands(case, family)
            ref, ab = O.reference(case, family, op)
            O.assert_exact(ab)
            assert bool((ref * 2 == np.round(ref * 2)).all()) and bool((ref.astype(np.float32).astype(np.float64) == ref).all()), case.name
            for name in ("A", "B"):
                share, exact = O.lo_fraction(op[name])
                assert exact, f"{case.name}: hi + lo != value"
                big = (family, name) in (("lo", "A"), ("lo-swapped", "B"))
                assert (share > 0.75) if (big and op[name].size >= 256) else (big or share == 0.0), (case.name, family, name, share)
        if case.dual:
            assert case.dual[0] in (1.0, -1.0, 0.5, 2.0) and float(case.dual[1]).is_integer()


def test_lo_family_is_limited_to_short_sums():
    for case in O.CASES:
        for p in O.PRECISIONS:
            if "lo" in case.families(p):
                assert case.g.K <= 128
            if "real" in case.families(p) and p == "high" and any(O.is_split(l) for l in case.launches("high")):
                assert case.g.K <= 128


def _chain_cases():
    out = [c for c in O.CASES if c.chain]
    out += [O.linear_case(M, N, K, "chain", 0, False) for M in O.LINEAR_M for N in O.LINEAR_N for K in O.LINEAR_K]
    out.append(O.linear_case(*O.LINEAR_BIG, "chain", 0, False))
    return out


def test_chain_cases_have_no_ties_and_sit_inside_the_highest_bar():
    cases = _chain_cases()
    assert len(cases) > 100
    for case in cases:
        op = O.operands(case, "chain")
        assert (op["alpha"], op["diag"], op["bias"], op["accumulate"]) == (1.0, 0.0, None, 0)
        val, ties = O.chain(op["A"], op["B"], case.g)
        assert ties == 0, f"{case.name}: {ties} fp32 tie(s) in the fp64 emulation of the chain -- change the case's seed"
        ref, ab = O.reference(case, "chain", op)
        assert bool((np.abs(val - ref) <= O.bar_highest(case.g.K, ab)).all()), case.name


def test_chain_is_a_true_fmaf_chain_on_a_hand_case():
    """1 + 2^-24 * (1 + 2^-20): above the half-way point only through the product's low bits -- a chain that rounded the product first would give 1"""
    g = O.geo(1, 1, 2)
    a = np.array([1.0, 2.0 ** -12 * (1 + 2.0 ** -10)], dtype=np.float32)
    b = np.array([1.0, 2.0 ** -12 * (1 + 2.0 ** -10)], dtype=np.float32)
    val, ties = O.chain(a, b, g)
    assert ties == 0 and float(val[0, 0, 0, 0]) == 1.0 + 2.0 ** -23
    _, ties = O.chain(np.array([1.0, 2.0 ** -12], dtype=np.float32), np.array([1.0, 2.0 ** -12], dtype=np.float32), g)
    assert ties == 1          # 1 + 2^-24 exactly: the tie the oracle refuses to judge


@pytest.mark.parametrize("group", O.GROUPS)
def test_high_bar_holds_the_emulation_and_sees_a_dropped_lo_plane(group):
    """Per real case that "high" takes to a splitting kernel: the fp32-accumulate emulation of lo hi + hi lo + hi hi stays under bar_high on every element; with A's
    lo plane read as zero the worst element is at least 4 x the bar."""
    for case in O.cases(group):
        if not any(O.is_split(l) for l in case.launches("high")) or "real" not in case.families("high"):
            continue
        g = case.g
        op = O.operands(case, "real")
        ref, ab = O.product(op["A"], op["B"], g), O.abs_sum(op["A"], op["B"], g)
        bar = O.bar_high(g.K, ab)
        good = float((np.abs(O.emulate_high(op["A"], op["B"], g) - ref) / bar).max())
        bad = float((np.abs(O.emulate_high(op["A"], op["B"], g, drop_lo_a=True) - ref) / bar).max())
        assert good <= 1.0 and bad >= 4.0, f"{case.name}: emulation at {good:.3f} of the bar, without A's lo plane {bad:.2f}"
        assert float(O.rel_l2(O.emulate_high(op["A"], op["B"], g), ref).max()) <= 2e-5


def test_row_class_pairs():
    for M, M2 in O.ROW_CLASS_PAIRS:
        assert O.row_class(M[0]) == O.row_class(M2[0])
    assert O.row_class(64) != O.row_class(65) and O.row_class(95) != O.row_class(96) and O.row_class(128) != O.row_class(256)


# ---- the expected kernels ------------------------------------------------------------------------------------------------------------------------------------------
def _reached(precision):
    out = {}
    for case in O.CASES:
        for l in case.launches(precision):
            out.setdefault(l.leaf, []).append((case, l))
    if precision == "highest":
        for relu in (0, 1):
            out[O.dispatch_linear(relu)[0].leaf] = [(O.linear_case(64, 64, 32, "grid", relu, True), O.dispatch_linear(relu)[0])]
    return out


@pytest.mark.parametrize("precision", O.PRECISIONS)
def test_every_launch_of_the_dispatch_is_reached(precision):
    reached = _reached(precision)
    missing = O.all_leaves(precision) - set(reached)
    assert not missing, f"no case reaches {sorted(missing)} at {precision}"
    assert not set(reached) - O.all_leaves(precision)
    x3 = 1 if precision == "high" else 0
    for tb in (0, 1):
        for ta in (0, 1):
            for wm, wn in ((2, 2), (4, 1), (1, 4)):
                hits = reached[(1433 if x3 else 1435, f"bgemm_f32_big_kernel<{tb},{ta},{wm},{wn},{x3}>")]
                loaders = set().union(*(l.loaders for _, l in hits))
                stores = set().union(*(l.stores for _, l in hits))
                assert loaders >= ({"fast", "vec4", "elem"} if ta else {"fast", "vec4"}), (tb, ta, wm, wn, loaders)          # the element loader needs A^T: anything else unaligned is the fallback's
                assert stores == {"inside", "inside+diag", "edge", "edge+diag"}, (tb, ta, wm, wn, stores)
                if x3:
                    for acc in ("true", "false"):
                        hits = reached[(1451 if acc == "true" else 1454, f"bgemm_x3_kernel<{tb},{ta},{wm},{wn},false,{acc}>")]
                        assert set().union(*(l.stores for _, l in hits)) == {"inside", "inside+diag"}
                        assert {c.g.K for c, _ in hits} >= {32, 96}
    # tile counts of the re-mapped kernels: below 8, 8, and every remainder class that matters (0, odd, r < 8 < total)
    tiles = {l.tiles for hits in reached.values() for _, l in hits if "big" in l.kernel or "x3" in l.kernel}
    assert tiles >= {1, 3, 7, 8, 9, 13}


def test_named_cases_reach_the_kernels_the_issue_names():
    def one(name, precision, **kw):
        (case,) = [c for c in O.CASES if c.name == name]
        return [l.kernel for l in case.launches(precision, **kw)]

    assert one("95x95x32 tb=1", "high") == ["bgemm_f32_kernel<1>"]
    assert one("96x8x32 tb=1", "highest") == ["bgemm_f32_big_kernel<1,0,4,1,0>"] and one("96x64x32 tb=0", "high") == ["bgemm_f32_big_kernel<0,0,4,1,1>"]
    assert one("8x96x32 tb=1", "highest") == ["bgemm_f32_big_kernel<1,0,1,4,0>"] and one("64x96x32 tb=1", "highest") == ["bgemm_f32_big_kernel<1,0,1,4,0>"]
    for n in ("96x96x32 tb=1", "97x65x32 tb=1", "65x97x32 tb=1"):
        assert one(n, "highest") == ["bgemm_f32_big_kernel<1,0,2,2,0>"]
    assert one("128x128x48 ABt", "high") == ["bgemm_f32_big_kernel<1,0,2,2,1>"]
    assert one("128x128x32 ABt acc=1", "high") == ["bgemm_x3_kernel<1,0,2,2,false,true>"]
    assert one("128x128x32 ABt acc=1", "high", x3_lds=False) == ["bgemm_f32_big_kernel<1,0,2,2,1>"]
    assert one("128x128x32 ABt acc=1", "highest") == ["bgemm_f32_big_kernel<1,0,2,2,0>"]
    assert one("128x128x32 A+1float tb=1", "high") == ["bgemm_f32_kernel<1>"] and one("128x128x32 lda=K+1 tb=0", "high") == ["bgemm_f32_kernel<0>"]
    assert one("5x7x3 At tb=1", "highest") == ["bgemm_f32_big_kernel<1,1,2,2,0>"]
    assert one("128x128x32 AB Z=3", "high") == ["bgemm_x3_kernel<0,0,2,2,true,false>"] and one("128x128x32 AB Z=3", "highest") == ["bgemm_f32_big_kernel<0,0,2,2,0,true>"]
    assert one("128x128x48 AB Z=3", "high") == ["bgemm_f32_big_kernel<0,0,2,2,1,true>"]
    assert one("130x70x52 AB ldb=72", "high") == ["bgemm_f32_big_kernel<0,0,2,2,1,true>"]
    assert one("256x64x64 AB (two calls)", "high") == ["bgemm_x3_kernel<0,0,4,1,false,false>"] * 2
    assert one("128x128x32 ABt (two calls)", "highest") == ["bgemm_f32_big_kernel<1,0,2,2,0>"] * 2
    assert one("40x40x40 AB (fallback twice)", "high") == ["bgemm_f32_kernel<0>"] * 2


def _launch_lines(src, first, last):
    return [(i, src[i - 1]) for i in range(first, last + 1) if "hipLaunchKernelGGL" in src[i - 1]]


def test_restated_launch_sites_are_the_launches_in_the_source():
    """`bgemm_oracle.LAUNCH_SITES` lists every hipLaunchKernelGGL of bgemm_f32_at in order, by the kernel text that stands there; its line numbers (the ones the GPU
    module's table and `Launch.line` carry) are the source's up to ONE common shift -- code added above the function moves them together."""
    src = (CSRC / "transmil.hip").read_text().splitlines()
    first = [i for i, s in enumerate(src, 1) if s.startswith("static int bgemm_f32_at")][-1]          # the definition follows the forward declaration
    last = next(i for i, s in enumerate(src, 1) if i > first and s.startswith("}"))
    gap = (CSRC / "gap.hip").read_text().splitlines()
    gfirst = next(i for i, s in enumerate(gap, 1) if s.startswith("int gemm_f32("))
    glast = next(i for i, s in enumerate(gap, 1) if i > gfirst and s.startswith("}"))
    for found, sites in ((_launch_lines(src, first, last), O.LAUNCH_SITES), (_launch_lines(gap, gfirst, glast), O.LINEAR_LAUNCH_SITES)):
        assert len(found) == len(sites), [i for i, _ in found]
        assert all(text_at in text for (_, text), (_, text_at) in zip(found, sites))
        assert len({i - line for (i, _), (line, _) in zip(found, sites)}) == 1
    leaves = {leaf for p in O.PRECISIONS for leaf in O.all_leaves(p)}
    assert {line for line, _ in leaves} == {line for line, _ in O.LAUNCH_SITES + O.LINEAR_LAUNCH_SITES}
    for line, kernel in leaves:          # a leaf's template arguments fit the text at its site
        text = dict(O.LAUNCH_SITES + O.LINEAR_LAUNCH_SITES)[line]
        name, args = kernel.split("<")[0], kernel.split("<")[1].rstrip(">").split(",")
        there = text.split("<")[1].rstrip(">").replace(" ", "").split(",")
        assert text.startswith(name + "<") and all(t == a or not (t.isdigit() or t in ("true", "false")) for t, a in zip(there, args)), (line, kernel)
        assert all(a in ("false", "0") for a in args[len(there):]), (line, kernel)


def test_print_the_case_that_reaches_each_launch():
    """under -s: launch site, kernel instance, and the first case that reaches it"""
    for precision in O.PRECISIONS:
        for (line, kernel), hits in sorted(_reached(precision).items()):
            assert hits
            print(f"bgemm-cpu| {precision} | :{line} | {kernel} | {len(hits)} case(s), first: {hits[0][0].name}")
