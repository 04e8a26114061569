"""amds_bag_plan on the GPU against its numpy restatement (tests/bag_plan_oracle.py; test_cpu_bag_plan.py holds THAT to the statistics of
`torch.randperm`), exactly: every size at which the geometry changes (0, 1, 2 rows; one below, at and above a power of two; an odd size past 2^16), bag sizes
below, at and above the rows, a patient list with repeats and out of order.  Then through `ResidentCohort`: the device sampler's batches are the store's rows
at the restated indices, and the host sampler's batches are what the parent's code path (`plan_indices` + `ops.bag_batch_gather`) gives, bit for bit."""
import numpy as np
import pytest
import torch

import bag_plan_oracle as O
from stamp_amd import _lib, h5io, ops
from stamp_amd.bags import PatientData
from stamp_amd.cohort import ResidentCohort, plan_indices

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 2, 511, 512, 513, 1024, 1025, 100_003]
OFFSETS = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.int64)
PATIENTS = [8, 0, 3, 3, 1, 7, 2, 5, 4, 6, 8, 0, 5]          # repeats, out of order, every patient
SEED = 0x1234_5678_9ABC_DEF1


def _plan(gpu, patients, bag, seed=SEED, epoch=0):
    idx, sizes = ops.bag_plan(torch.tensor(OFFSETS, dtype=torch.int32, device=gpu), torch.tensor(patients, dtype=torch.int64, device=gpu), bag, seed, epoch)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sizes.cpu().numpy()


@pytest.fixture(scope="module")
def oracle_plans():
    return {bag: O.bag_plan(OFFSETS, PATIENTS, bag, SEED, 0) for bag in (1, 16, 512)}


@pytest.mark.parametrize("bag", [1, 16, 512])
def test_plan_equals_the_restatement_exactly(gpu, bag, oracle_plans):
    idx, sizes = _plan(gpu, PATIENTS, bag)
    want_idx, want_sizes = oracle_plans[bag]
    assert idx.shape == (len(PATIENTS), bag) and idx.dtype == np.int64 and sizes.dtype == np.int64
    assert np.array_equal(sizes, want_sizes) and np.array_equal(sizes, [min(bag, ROWS[p]) for p in PATIENTS])
    assert np.array_equal(idx, want_idx), np.argwhere(idx != want_idx)[:5]
    for b, p in enumerate(PATIENTS):
        m = int(sizes[b])
        assert (idx[b, m:] == -1).all()                                                  # entries past `sizes` are -1; a patient without rows: all of them
        real = idx[b, :m]
        assert ((real >= OFFSETS[p]) & (real < OFFSETS[p + 1])).all() and np.unique(real).size == m          # the patient's own rows, each at most once
    # the same patient in another position of the list: the same bag
    for p in (3, 8, 0, 5):
        b0, b1 = [b for b, q in enumerate(PATIENTS) if q == p][:2]
        assert np.array_equal(idx[b0], idx[b1])


def test_plan_depends_on_the_key_alone(gpu, oracle_plans):
    """(seed, epoch, patient) decide a bag: another list, another length of the list (another grid) and a second call change nothing; the epoch and the
    seed do."""
    idx, _ = _plan(gpu, PATIENTS, 16)
    again, _ = _plan(gpu, PATIENTS, 16)
    assert np.array_equal(idx, again)
    alone, sizes = _plan(gpu, [8], 16)
    assert np.array_equal(alone[0], idx[0]) and sizes.tolist() == [16]
    shuffled, _ = _plan(gpu, PATIENTS[::-1], 16)
    assert np.array_equal(shuffled[::-1], idx)
    # a prefix of a longer bag: entry j is pi(j) whatever the bag size
    long, _ = _plan(gpu, PATIENTS, 512)
    assert np.array_equal(long[:, :16][idx >= 0], idx[idx >= 0])
    e1, _ = _plan(gpu, PATIENTS, 16, epoch=1)
    s1, _ = _plan(gpu, PATIENTS, 16, seed=SEED + 1)
    hi, _ = _plan(gpu, PATIENTS, 16, seed=SEED + 2 ** 32)
    for other in (e1, s1, hi):
        assert not np.array_equal(other[0], idx[0]) and np.array_equal(other < 0, idx < 0)
    assert np.array_equal(e1, O.bag_plan(OFFSETS, PATIENTS, 16, SEED, 1)[0])
    assert np.array_equal(hi, O.bag_plan(OFFSETS, PATIENTS, 16, SEED + 2 ** 32, 0)[0])
    # a whole permutation: bag_size = rows
    full, _ = _plan(gpu, [7], 1025)
    assert np.array_equal(np.sort(full[0]), np.arange(OFFSETS[7], OFFSETS[8]))


def test_plan_refuses_invalid_arguments_before_a_launch(gpu):
    off = torch.tensor(OFFSETS, dtype=torch.int32, device=gpu)
    pat = torch.tensor([1, 2], dtype=torch.int64, device=gpu)
    idx = torch.full((2, 4), 77, dtype=torch.int64, device=gpu)
    sizes = torch.full((2,), 77, dtype=torch.int64, device=gpu)
    lib = _lib.lib()
    for args, text in [((None, pat.data_ptr(), idx.data_ptr(), sizes.data_ptr(), 2, 4), b"null pointer"),
                       ((off.data_ptr(), pat.data_ptr(), None, sizes.data_ptr(), 2, 4), b"null pointer"),
                       ((off.data_ptr(), pat.data_ptr(), idx.data_ptr(), sizes.data_ptr(), 2, 0), b"bag_size=0"),
                       ((off.data_ptr(), pat.data_ptr(), idx.data_ptr(), sizes.data_ptr(), -1, 4), b"n=-1")]:
        assert lib.amds_bag_plan(*args, 1, 0, None) == -1 and text in lib.amds_last_error(), args
    assert lib.amds_bag_plan(off.data_ptr(), pat.data_ptr(), idx.data_ptr(), sizes.data_ptr(), 0, 4, 1, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((idx == 77).all()) and bool((sizes == 77).all())          # nothing was launched
    with pytest.raises(ValueError, match="bag_size"):
        ops.bag_plan(off, pat, 0)
    e_idx, e_sizes = ops.bag_plan(off, pat[:0], 4)
    assert e_idx.shape == (0, 4) and e_sizes.shape == (0,)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.bag_plan(off.cpu(), pat.cpu(), 4)


# ---- through ResidentCohort ------------------------------------------------------------------------------------------------------------------------
TILES = [5, 40, 16, 17, 1, 33, 8]


@pytest.fixture(scope="module")
def small_cohort(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("bag_plan_cohort")
    rng = np.random.default_rng(0)
    pdata, feats = [], []
    for i, n in enumerate(TILES):
        x = rng.standard_normal((n, 24)).astype(np.float16)
        coords = rng.integers(0, 50, (n, 2)).astype(np.float32) * 256.0
        h5io.write_tile_features(d / f"p{i}.h5", x, coords, extractor="test", tile_size_um=256.0, tile_size_px=224, code_hash="0", stamp_version="2.4.0")
        pdata.append(PatientData(ground_truth="a" if i % 2 else "b", feature_files=[d / f"p{i}.h5"]))
        feats.append(x)
    return ResidentCohort(pdata, task="classification", device=gpu), np.concatenate(feats)


def _expected(cohort, idx, out_dtype=torch.float32):
    idx = torch.as_tensor(idx, device=cohort.device)
    real = (idx >= 0)[..., None]
    return (torch.where(real, cohort.feats[idx.clamp(min=0)].float(), torch.zeros((), device=cohort.device)).to(out_dtype),
            torch.where(real, cohort.coords[idx.clamp(min=0)], torch.zeros((), device=cohort.device)))


@pytest.mark.parametrize("members", [None, [6, 1, 3, 5, 0]], ids=["cohort", "view"])
def test_device_sampler_batches_are_the_stores_rows_at_the_restated_indices(small_cohort, members):
    cohort, host_feats = small_cohort
    assert torch.equal(cohort.feats.cpu(), torch.from_numpy(host_feats))
    src = cohort if members is None else cohort.view(members)
    store_of = list(range(len(cohort))) if members is None else members
    bag, batch, seed = 16, 3, 11
    feed = src.train_batches(batch, bag, generator=torch.Generator().manual_seed(5), sampler="device", seed=seed)
    g = torch.Generator().manual_seed(5)
    for epoch in range(2):          # the returned callable counts its invocations: epoch 0, then 1
        order = [store_of[i] for i in torch.randperm(len(store_of), generator=g).tolist()]
        want_idx, want_sizes = O.bag_plan(cohort.offsets, order, bag, seed, epoch)
        got = list(feed())
        assert len(got) == -(-len(order) // batch)
        for j, (bags, coords, sizes, targets) in enumerate(got):
            sl = slice(j * batch, (j + 1) * batch)
            wb, wc = _expected(cohort, want_idx[sl])
            assert bags.dtype == torch.float32 and torch.equal(bags.view(torch.int32), wb.view(torch.int32)) and torch.equal(coords, wc)
            assert sizes.tolist() == want_sizes[sl].tolist() and torch.equal(targets, cohort._targets_dev[order[sl]])
            assert bool((bags[torch.as_tensor(want_idx[sl] < 0, device=bags.device)] == 0).all())          # zero padding
    assert not np.array_equal(O.bag_plan(cohort.offsets, [1], bag, seed, 0)[0], O.bag_plan(cohort.offsets, [1], bag, seed, 1)[0])


def test_device_sampler_draws_nothing_but_the_order_from_the_generator(small_cohort):
    cohort, _ = small_cohort
    g, h = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    list(cohort.train_batches(4, 8, generator=g, sampler="device")())
    torch.randperm(len(cohort), generator=h)
    assert torch.equal(g.get_state(), h.get_state())
    # with vary_precision: the order, then the epoch's mask seed -- the rule of the host sampler
    list(cohort.barspoon_batches(4, 8, generator=g, sampler="device", vary_precision_bits=4)())
    torch.randperm(len(cohort), generator=h)
    torch.randint(0, 2 ** 62, (1,), generator=h)
    assert torch.equal(g.get_state(), h.get_state())
    with pytest.raises(ValueError, match="shuffle=False"):
        cohort.train_batches(4, 8, shuffle=False, sampler="device")


@pytest.mark.parametrize("shuffle", [True, False])
def test_host_sampler_batches_are_the_parents_bit_for_bit(small_cohort, shuffle):
    """sampler="torch" (the default): `plan_indices` + `ops.bag_batch_gather` by hand, as before views existed."""
    cohort, _ = small_cohort
    bag, batch = 16, 3
    for kw in ({}, {"sampler": "torch"}):
        got = list(cohort.train_batches(batch, bag, shuffle=shuffle, generator=torch.Generator().manual_seed(3), out_dtype=torch.float16, vary_precision_bits=5, **kw)())
        g = torch.Generator().manual_seed(3)
        N = len(cohort)
        order = torch.randperm(N, generator=g) if shuffle else torch.arange(N)
        idx, sizes = plan_indices(cohort.offsets, cohort.lengths, order.tolist(), bag, deterministic=not shuffle, generator=g)
        vp_seed = int(torch.randint(0, 2 ** 62, (1,), generator=g).item())
        assert len(got) == 3
        for j, (bags, coords, bs, targets) in enumerate(got):
            sl = slice(j * batch, (j + 1) * batch)
            wb, wc = ops.bag_batch_gather(cohort.feats, cohort.coords, idx[sl].to(cohort.device), torch.float16, vary_precision_bits=5, seed=vp_seed, stream_id=j)
            assert torch.equal(bags.view(torch.int16), wb.view(torch.int16)) and torch.equal(coords, wc)
            assert torch.equal(bs.cpu(), sizes[sl]) and torch.equal(targets, cohort._targets_dev[order[sl].to(cohort.device)])
