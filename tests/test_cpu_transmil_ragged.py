"""Host side of the ragged TransMIL forward: per-bag geometry, the library's bag order and buckets, grouping by padded rows, refusals -- no kernels."""
import ctypes as C
import math

import pytest
import torch

from stamp_amd import _lib, transmil_core
from stamp_amd.transmil_core import bag_geometry, group_bags_padded, ragged_plan

TILES = [1, 2, 3, 4, 5, 255, 256, 257, 1024, 1025, 16384]
LANDMARKS = [32, 64, 256]


def _reference_geometry(T: int, m: int) -> dict:
    """trans_mil.py:306-314 (`_H = _W = int(np.ceil(np.sqrt(H)))`, one class token) and :96-100, :113 (`padding = m - (n % m)` when there is a remainder,
    `l = ceil(n / m)`), written out independently of the code under test."""
    side = int(math.ceil(math.sqrt(T)))
    assert (side - 1) ** 2 < T <= side * side
    n = side * side + 1
    rem = n % m
    pad = m - rem if rem > 0 else 0
    return dict(side=side, n=n, pad=pad, np=n + pad, l=int(math.ceil(n / m)))


@pytest.mark.parametrize("m", LANDMARKS)
def test_bag_geometry_follows_the_reference_formulas(m):
    for T in TILES:
        got, ref = bag_geometry(T, m), _reference_geometry(T, m)
        assert got == ref, (T, m, got, ref)
        assert got["np"] % m == 0 and got["np"] // m == got["l"] and 0 <= got["pad"] < m
    with pytest.raises(ValueError):
        bag_geometry(0, m)


@pytest.mark.parametrize("m", LANDMARKS)
def test_library_plan_matches_the_formulas_and_buckets_partition_the_bags(m):
    lengths = TILES + [300, 5, 1024, 1]                        # repeated np values in different places of the caller's order
    table, buckets, perm = ragged_plan(lengths, 2 * m)
    n = len(lengths)
    assert sorted(perm) == list(range(n))                       # a permutation: every bag once
    inv = [0] * n
    for s, i in enumerate(perm):
        inv[i] = s
    assert [perm[inv[i]] for i in range(n)] == list(range(n))   # and it round-trips
    tile_offs = [sum(lengths[:i]) for i in range(n)]
    row = 0
    for s in range(n):
        g, i = table[s], perm[s]
        ref = _reference_geometry(lengths[i], m)
        assert (g.tiles, g.side, g.n, g.pad, g.np, g.orig) == (lengths[i], ref["side"], ref["n"], ref["pad"], ref["np"], i)
        assert g.tile_off == tile_offs[i] and g.row_off == row
        row += g.np
    # ordered by np, then by the caller's order
    assert [(table[s].np, table[s].orig) for s in range(n)] == sorted((table[s].np, table[s].orig) for s in range(n))
    # the buckets are the runs of equal np and cover every slot once
    assert buckets[0][0] == 0 and sum(c for _, c, _ in buckets) == n
    for k, (s0, cnt, np_) in enumerate(buckets):
        assert cnt >= 1 and all(table[s].np == np_ for s in range(s0, s0 + cnt))
        if k:
            assert s0 == buckets[k - 1][0] + buckets[k - 1][1] and np_ > buckets[k - 1][2]
    assert ragged_plan([], 2 * m)[1:] == ([], [])


def test_group_bags_padded_caps():
    m, dim = 256, 512
    np_of = lambda t: bag_geometry(t, m)["np"]  # noqa: E731
    assert group_bags_padded([], dim, 4, 1000) == []
    assert group_bags_padded([10] * 10, dim, 4, 10 ** 9) == [(0, 4), (4, 8), (8, 10)]
    # the cap counts PADDED rows: a 10-tile bag occupies np = 256 rows
    assert np_of(10) == 256 and group_bags_padded([10] * 5, dim, 64, 512) == [(0, 2), (2, 4), (4, 5)]
    # a bag whose padded rows alone exceed the limit forms its own group; neighbours keep their order
    assert np_of(1024) == 1280 and group_bags_padded([5, 1024, 5], dim, 64, 600) == [(0, 1), (1, 2), (2, 3)]
    g = torch.Generator().manual_seed(0)
    lengths = [int(x) for x in torch.randint(1, 20000, (300,), generator=g)]
    for k, rows in ((1, 10 ** 9), (7, 262144), (64, 65536), (10 ** 6, 10 ** 12)):
        groups = group_bags_padded(lengths, dim, k, rows)
        assert [a for a, _ in groups] == [0] + [e for _, e in groups[:-1]] and groups[-1][1] == len(lengths)
        for a, e in groups:
            assert 1 <= e - a <= min(k, transmil_core.MAX_BAGS_PER_CALL)
            if e - a > 1:
                assert sum(np_of(t) for t in lengths[a:e]) <= rows
    with pytest.raises(ValueError):
        group_bags_padded([1], dim, 0, 10)
    with pytest.raises(ValueError):
        group_bags_padded([1], dim, 1, 0)


def test_plan_entry_rejects_bad_input_on_the_host():
    lib = _lib.lib()
    cfg = _lib.TransMilCfg(8, 64, 2)
    table = (_lib.TransMilBag * 3)()
    assert lib.amds_transmil_ragged_plan(C.byref(cfg), 0, None, None) == 0
    assert lib.amds_transmil_ragged_workspace_bytes(C.byref(cfg), 3, (C.c_int * 3)(5, 1, 70)) > 0
    assert lib.amds_transmil_ragged_plan(C.byref(cfg), 3, (C.c_int * 3)(5, 0, 7), table) == -1 and b"empty bag" in lib.amds_last_error()
    assert lib.amds_transmil_ragged_workspace_bytes(C.byref(cfg), 3, (C.c_int * 3)(5, 0, 7)) == 0
    assert lib.amds_transmil_ragged_workspace_bytes(C.byref(cfg), -1, None) == 0
    assert lib.amds_transmil_ragged_plan(C.byref(cfg), 8192, (C.c_int * 8192)(*([1] * 8192)), None) == -1 and b"batch dimension" in lib.amds_last_error()
    bad = _lib.TransMilCfg(8, 60, 2)
    assert lib.amds_transmil_ragged_workspace_bytes(C.byref(bad), 1, (C.c_int * 1)(5)) == 0 and b"multiple of 8" in lib.amds_last_error()


def test_forward_ragged_refuses_training_grad_cpu_and_bad_bags():
    from stamp_amd.mil import TransMIL

    m = TransMIL(dim_output=2, dim_input=8, dim_hidden=64)
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_ragged([torch.randn(3, 8)])
    m.eval()
    with pytest.raises(RuntimeError, match="eval"):            # grad mode still enabled
        m.forward_ragged([torch.randn(3, 8)])
    with torch.no_grad():
        with pytest.raises(ValueError, match="empty"):
            m.forward_ragged([torch.randn(3, 8), torch.randn(0, 8)])
        with pytest.raises(ValueError, match="features"):
            m.forward_ragged([torch.randn(3, 9)])
        with pytest.raises(ValueError):
            m.forward_ragged([torch.randn(1, 3, 8)])
        with pytest.raises(RuntimeError, match="GPU"):
            m.forward_ragged([torch.randn(3, 8)], coords=[torch.zeros(3, 2)])
        out = m.forward_ragged([])
        assert out.shape == (0, 2) and out.dtype == torch.float32


def test_predict_argument_checks_with_a_transmil_head():
    from stamp_amd.deploy import predict_
    from stamp_amd.mil import TransMIL

    m = TransMIL(dim_output=2, dim_input=8, dim_hidden=64)
    for kw in (dict(bags_per_call=0), dict(max_rows_per_call=0), dict(bags_per_call=-3)):
        with pytest.raises(ValueError, match=">= 1"):
            predict_(m, [], [], task="classification", device="cpu", **kw)
    with pytest.raises(ValueError, match="task"):
        predict_(m, [], [], task="ranking", device="cpu", bags_per_call=4)
    assert predict_(m, [], [], task="classification", device="cpu", bags_per_call=4) == {}
    # the ragged branch is taken for this head: a CPU bag reaches TransMIL.forward_ragged, which has no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        predict_(m, [(torch.randn(1, 5, 8), None, None, None)], ["a"], task="classification", device="cpu", bags_per_call=4)
