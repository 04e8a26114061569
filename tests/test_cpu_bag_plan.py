"""The permutation of amds_bag_plan, without a GPU: `bag_plan_oracle` restates it in numpy (integers only; tests/test_gpu_bag_plan.py holds the kernel to it
bit for bit).  Here: it IS a permutation, its cycle walk keeps to the stated bound, and its first `bag` entries are distributed like
`torch.randperm(rows)[:bag]` -- the same statistics on torch's own generator as a control, and on a 4-round network as a mutant that must fail.

The bar |z| <= 6 on every statistic.  For a fair source z has mean 0 and variance 1; with r - 1 >= 4 degrees of freedom 6 sigma is far in the tail, at one or
two degrees of freedom (rows 2 and 3) the chi-square tail is heavier and a fair source passes 6 with probability 2e-3 / 1e-3 per statistic.  The key set is
fixed (numpy default_rng(0), chosen before any statistic was looked at), so the test is deterministic; observed with 12 rounds on it: max |z| = 2.10 over 22
statistics (torch.randperm under manual_seed(0): 1.58; 4 rounds: 290).  Of two further key sets one gave 1.87 and one 7.37 at rows = 2 (a 3.4 sigma coin); 800 000
keys pooled show no bias there (399 717 : 400 283)."""
import numpy as np
import pytest
import torch

import bag_plan_oracle as O

CASES = [(2, 2), (3, 2), (5, 4), (6, 6), (17, 8), (33, 16), (97, 16), (1025, 16)]
N_KEYS = 20000
BAR = 6.0


def _all_z(sample) -> dict:
    out = {}
    for rows, bag in CASES:
        s = sample(rows, bag)
        assert s.shape == (N_KEYS, bag) and s.min() >= 0 and s.max() < rows
        assert all(np.unique(row).size == bag for row in s[:200])          # entries of one bag are distinct
        for k, v in O.z_scores(s, rows).items():
            out[(rows, bag, k)] = float(v)
            print(f"rows {rows} bag {bag} {k}: z = {v:+.2f}")
    # inclusion is skipped where bag == rows, pairs past rows = 100
    assert len(out) == 3 * len(CASES) - 2 - 1
    return out


def _assert_fair(z: dict) -> None:
    worst = max(z, key=lambda k: abs(z[k]))
    print("max |z| =", abs(z[worst]), "at", worst)
    assert abs(z[worst]) <= BAR, (worst, z[worst])


@pytest.mark.parametrize("rows", [1, 2, 3, 5, 64, 65, 1000, 4097])
def test_full_permutation_is_a_permutation_within_the_walk_bound(rows):
    """Five keys per size; `permute` itself raises when an entry takes more than domain - rows + 1 applications."""
    rk = O.round_keys(np.arange(5, dtype=np.uint64) * np.uint64(0x123456789), np.uint64(3), np.uint64(11))
    perm, steps = O.permute(rows, rows, rk, return_steps=True)
    half, mask, domain = O.geometry(rows)
    assert domain == (mask + 1) ** 2 == 1 << (2 * half) and rows <= domain and (rows == 1 or domain < 4 * rows)
    assert 1 <= steps <= domain - rows + 1
    assert np.array_equal(np.sort(perm, axis=1), np.broadcast_to(np.arange(rows), (5, rows)))
    if rows >= 64:
        assert not np.array_equal(perm[0], perm[1]) and not np.array_equal(perm[0], np.arange(rows))
    # the key is (seed, epoch, patient): each of the three changes the permutation, and nothing else enters
    base = O.permute(1000, 16, O.round_keys(np.uint64(5), np.uint64(2), np.uint64(9))[None])
    for other in ((6, 2, 9), (5, 3, 9), (5, 2, 10), (5 + 2 ** 32, 2, 9), (5, 2, 9 + 2 ** 32)):
        assert not np.array_equal(base, O.permute(1000, 16, O.round_keys(*(np.uint64(v) for v in other))[None])), other


def test_prefixes_are_distributed_like_randperm():
    _assert_fair(_all_z(lambda rows, bag: O.keyed_samples(rows, bag, N_KEYS)))


def test_control_torch_randperm_passes_the_same_statistics():
    torch.manual_seed(0)
    _assert_fair(_all_z(lambda rows, bag: O.torch_samples(rows, bag, N_KEYS)))


def test_mutant_four_round_network_fails_the_statistics():
    z = _all_z(lambda rows, bag: O.keyed_samples(rows, bag, N_KEYS, rounds=4))
    with pytest.raises(AssertionError):
        _assert_fair(z)
    assert max(abs(v) for v in z.values()) > 3 * BAR


def test_bag_plan_oracle_pads_and_sizes():
    offsets = [0, 0, 1, 3, 20]
    idx, sizes = O.bag_plan(offsets, [3, 0, 1, 2, 3], 4, seed=1, epoch=0)
    assert sizes.tolist() == [4, 0, 1, 2, 4] and np.array_equal(idx[0], idx[4])
    assert (idx[1] == -1).all() and idx[2].tolist() == [0, -1, -1, -1] and sorted(idx[3, :2].tolist()) == [1, 2] and (idx[3, 2:] == -1).all()
    assert ((idx[0] >= 3) & (idx[0] < 20)).all() and np.unique(idx[0]).size == 4
    assert not np.array_equal(idx[0], O.bag_plan(offsets, [3], 4, seed=1, epoch=1)[0][0])


def test_bag_plan_refuses_invalid_arguments_before_any_launch():
    """NULL pointers, bag_size < 1 and n < 0 come back as AMDS_ERR_INVALID (-1) with their text (the pointers are never dereferenced: no GPU here); n == 0
    succeeds and launches nothing; the symbol is declared and bound."""
    from pathlib import Path

    from stamp_amd import _lib
    lib = _lib.lib()
    P = 0x1000

    def call(offsets=P, patients=P, idx=P, sizes=P, n=2, bag=4):
        return lib.amds_bag_plan(offsets, patients, idx, sizes, n, bag, 1, 0, None)

    for kw, text in [(dict(offsets=None), b"null pointer"), (dict(patients=None), b"null pointer"), (dict(idx=None), b"null pointer"),
                     (dict(sizes=None), b"null pointer"), (dict(bag=0), b"bag_size=0 must be >= 1"), (dict(bag=-2), b"bag_size=-2"), (dict(n=-1), b"n=-1")]:
        assert call(**kw) == -1 and text in lib.amds_last_error(), (kw, lib.amds_last_error())
        if "n" not in kw:
            assert call(n=0, **kw) == -1
    assert call(n=0) == 0
    header = (Path(__file__).resolve().parent.parent / "include" / "amdstamp.h").read_text()
    assert "int amds_bag_plan(" in header and "amds_bag_plan" in _lib.PROTOTYPES
