"""The host side of the HBM-resident cohort feed (stamp_amd/cohort.py) and the argument checks of amds_bag_batch_gather -- no GPU needed: the index plan
against the per-patient sampling stream, the size refusals (before any allocation), every invalid C argument with its text, the new symbols."""
from pathlib import Path

import numpy as np
import pytest
import torch

from stamp_amd import _lib, cohort, h5io
from stamp_amd.bags import PatientData
from stamp_amd.mil import fixed_size_bag_indices

ROOT = Path(__file__).resolve().parent.parent
BAG = 64
LENGTHS = [1, 64, 65, 700, 65, 1, 700, 64]


def _offsets(lengths):
    o = [0]
    for n in lengths:
        o.append(o[-1] + n)
    return o


@pytest.mark.parametrize("deterministic", [False, True])
def test_plan_indices_is_the_per_patient_sampling_stream(deterministic):
    """One seeded generator: the plan of a batch order equals `fixed_size_bag_indices` called per patient in that order (what BagDataset items fetched in
    that order draw), shifted by the patient's first store row, -1 behind a short bag; the generator ends in the same state."""
    offs = _offsets(LENGTHS)
    order = [3, 0, 6, 1, 2, 4, 7, 5, 3]
    g1, g2 = torch.Generator().manual_seed(1234), torch.Generator().manual_seed(1234)
    idx, sizes = cohort.plan_indices(offs, LENGTHS, order, BAG, deterministic, g1)
    assert idx.dtype == torch.int64 and idx.shape == (len(order), BAG) and sizes.dtype == torch.int64
    for b, p in enumerate(order):
        local = fixed_size_bag_indices(LENGTHS[p], BAG, deterministic, g2)
        k = local.numel()
        assert k == min(BAG, LENGTHS[p]) == int(sizes[b])
        assert torch.equal(idx[b, :k], local + offs[p])
        assert bool((idx[b, k:] == -1).all())
        assert int(idx[b, :k].min()) >= offs[p] and int(idx[b, :k].max()) < offs[p + 1]
    assert torch.equal(torch.randint(0, 2 ** 31, (4,), generator=g1), torch.randint(0, 2 ** 31, (4,), generator=g2))
    if deterministic:          # nothing random: a second plan is the same plan
        assert torch.equal(cohort.plan_indices(offs, LENGTHS, order, BAG, True, g1)[0], idx)
    # the global generator when none is given -- the one BagDataset's own draws come from
    torch.manual_seed(7)
    a, _ = cohort.plan_indices(offs, LENGTHS, order, BAG, deterministic)
    torch.manual_seed(7)
    ref = [fixed_size_bag_indices(LENGTHS[p], BAG, deterministic) + offs[p] for p in order]
    assert all(torch.equal(a[b, :r.numel()], r) for b, r in enumerate(ref))
    with pytest.raises(ValueError):
        cohort.plan_indices(offs, LENGTHS, order, 0)


def _write_patients(tmp_path, rows=(5, 9), Fd=16):
    rng = np.random.default_rng(0)
    pdata = []
    for i, n in enumerate(rows):
        p = tmp_path / f"p{i}.h5"
        h5io.write_tile_features(p, rng.standard_normal((n, Fd)).astype(np.float16), rng.integers(0, 9, (n, 2)).astype(np.float32) * 256.0, extractor="test",
                                 tile_size_um=256.0, tile_size_px=224, code_hash="0", stamp_version="2.4.0")
        pdata.append(PatientData(ground_truth="a" if i % 2 else "b", feature_files=[p]))
    return pdata


def test_feature_shape_reads_what_the_file_holds(tmp_path):
    pdata = _write_patients(tmp_path)
    assert [h5io.feature_shape(p.feature_files[0]) for p in pdata] == [(5, 16, np.dtype(np.float16)), (9, 16, np.dtype(np.float16))]


def test_size_refusals_come_before_any_allocation(tmp_path, monkeypatch):
    """14 rows x (16 fp16 features + 2 fp32 coordinates) = 14 * 40 = 560 bytes.  A smaller `max_bytes`, or less free device memory, is a ValueError that names
    both numbers -- raised before a tensor is allocated or (max_bytes) the device is even asked."""
    pdata = _write_patients(tmp_path)

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the size check")

    def no_device(*a, **k):
        raise AssertionError("the device was queried before max_bytes was checked")

    monkeypatch.setattr(torch, "empty", no_alloc)
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    with pytest.raises(ValueError, match=r"560 bytes.*max_bytes allows 559"):
        cohort.ResidentCohort(pdata, task="classification", device="cuda:0", max_bytes=559)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (100, 1 << 30))
    with pytest.raises(ValueError, match=r"560 bytes.*100 are free"):
        cohort.ResidentCohort(pdata, task="classification", device="cuda:0", max_bytes=560)
    with pytest.raises(ValueError, match=r"560 bytes.*100 are free"):
        cohort.ResidentCohort(feature_files=[p.feature_files for p in pdata], ground_truths=["b", "a"], task="classification", device="cuda:0")
    monkeypatch.setattr(h5io, "feature_shape", lambda path: (2 ** 30, 16, np.dtype(np.float16)))
    with pytest.raises(ValueError, match="32-bit row index"):
        cohort.ResidentCohort(pdata, task="classification", device="cuda:0")
    with pytest.raises(ValueError, match="ground_truths"):
        cohort.ResidentCohort(feature_files=[[]], task="classification")


def test_bag_batch_gather_refuses_invalid_arguments_with_their_text():
    """Every refusal of include/amdstamp.h comes back as AMDS_ERR_INVALID (-1) with its text, before any launch (the pointers are never dereferenced: no GPU
    here); n_bags == 0 succeeds and launches nothing."""
    lib = _lib.lib()
    P = 0x1000          # a non-null pointer nobody reads
    F16, BF16, F32 = _lib.F16, _lib.BF16, _lib.F32

    def call(store=P, store_ld=8, sdt=F16, sc=P, idx=P, out=P, out_ld=8, odt=F32, co=P, n_bags=2, bag=4, cols=8, bits=0):
        return lib.amds_bag_batch_gather(store, store_ld, sdt, sc, idx, out, out_ld, odt, co, n_bags, bag, cols, bits, 1, 0, None)

    cases = [(dict(store=None), b"null pointer"), (dict(idx=None), b"null pointer"), (dict(out=None), b"null pointer"),
             (dict(sc=None), b"come together"), (dict(co=None), b"come together"),
             (dict(bag=0), b"bag_size=0 must be >= 1"), (dict(bag=-3), b"bag_size=-3 must be >= 1"), (dict(n_bags=-1), b"n_bags=-1"),
             (dict(out_ld=7), b"out_ld=7 < cols=8"), (dict(store_ld=7), b"store_ld=7 < cols=8"), (dict(cols=0, store_ld=0, out_ld=0), b"cols < 1"),
             (dict(sdt=F32, odt=F16), b"unsupported dtype pair 2 -> 0"), (dict(sdt=F32, odt=BF16), b"unsupported dtype pair"),
             (dict(sdt=BF16, odt=F32), b"unsupported dtype pair 1 -> 2"), (dict(sdt=BF16, odt=BF16), b"unsupported dtype pair"), (dict(odt=7), b"unsupported dtype pair"),
             (dict(bits=-1), b"vp_min_fraction_bits=-1 outside 0..22"), (dict(bits=23), b"vp_min_fraction_bits=23 outside 0..22")]
    for kw, text in cases:
        assert call(**kw) == -1 and text in lib.amds_last_error(), (kw, lib.amds_last_error())
        if "n_bags" not in kw:
            assert call(n_bags=0, **kw) == -1          # invalid stays invalid for an empty batch
    for sdt, odt in ((F16, F32), (F16, F16), (F16, BF16), (F32, F32)):
        assert call(sdt=sdt, odt=odt, n_bags=0) == 0
    assert call(n_bags=0, sc=None, co=None, bits=22) == 0
    sh = lib.amds_bag_batch_shifts
    assert sh(None, 1, 1, 1, 2, 0, 0, None) == -1 and b"null pointer" in lib.amds_last_error()
    assert sh(P, 1, 0, 1, 2, 0, 0, None) == -1 and b"bad sizes" in lib.amds_last_error()
    assert sh(P, 1, 1, 1, 23, 0, 0, None) == -1 and b"outside 0..22" in lib.amds_last_error()
    assert sh(P, 0, 1, 1, 2, 0, 0, None) == 0


def test_new_symbols_are_declared_and_bound():
    header = (ROOT / "include" / "amdstamp.h").read_text()
    for name in ("amds_bag_batch_gather", "amds_bag_batch_shifts"):
        assert f"int {name}(" in header and name in _lib.PROTOTYPES and hasattr(_lib.lib(), name)
    assert len(_lib.PROTOTYPES["amds_bag_batch_gather"][1]) == 16 and len(_lib.PROTOTYPES["amds_bag_batch_shifts"][1]) == 8
    assert "not torch's CPU" in header          # the header says which random stream the fused vary_precision is NOT
