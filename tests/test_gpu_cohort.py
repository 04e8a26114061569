"""The HBM-resident cohort feed on the GPU: amds_bag_batch_gather against torch indexing (bit for bit, in guarded buffers, past 2 GiB, with the fused
vary_precision), `ResidentCohort` against `BagDataset` + the reference's collate functions, training through `fit` from either feed, and the zero-copy
ragged views through the three ragged inference forwards."""
import copy

import numpy as np
import pytest
import torch

import guarded as gd
from stamp_amd import bags as B
from stamp_amd import h5io, ops
from stamp_amd.cohort import ResidentCohort

pytestmark = pytest.mark.gpu

ROWS = 300
PAIRS = {"f16_f32": (torch.float16, torch.float32), "f16_f16": (torch.float16, torch.float16), "f16_bf16": (torch.float16, torch.bfloat16),
         "f32_f32": (torch.float32, torch.float32)}
_INT = {2: torch.int16, 4: torch.int32}


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def _round_up(n, m):
    return (n + m - 1) // m * m


def _store(cols, dt, ld, seed=0):
    """[ROWS, cols] view of a [ROWS, ld] tensor; row 0 starts with the values a cast can get wrong: -0, the largest, the smallest normal and subnormal fp16."""
    g = torch.Generator().manual_seed(seed + cols)
    full = (torch.randn(ROWS, ld, generator=g) * 3).to(dt)
    special = torch.tensor([-0.0, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24, -(2.0 ** -24) * 3, 1.0009765625], dtype=torch.float32).to(dt)
    full[0, :min(cols, special.numel())] = special[:cols]
    return full


def _idx(n_bags, bag, g):
    """row 0, the last row, a repeat inside a bag and across bags, runs of -1 at a bag's end and start"""
    idx = torch.randint(0, ROWS, (n_bags, bag), generator=g)
    idx.view(-1)[0] = 0
    idx.view(-1)[-1] = ROWS - 1
    if bag >= 5:
        idx[0, 1] = idx[0, 0]
        idx[0, -2:] = -1
    if n_bags == 3:
        idx[1] = idx[0]
        if bag >= 5:
            idx[2, :3] = -1
    return idx


def _expect(store, coords, idx, out_dtype, out_ld):
    """torch indexing: the gathered rows as fp32, cast, zero pad columns, zero padding rows"""
    n_bags, bag = idx.shape
    cols = store.shape[1]
    real = (idx >= 0)
    rows = store[idx.clamp(min=0)].float().to(out_dtype)
    want = torch.zeros(n_bags, bag, out_ld, dtype=out_dtype, device=store.device)
    want[..., :cols] = torch.where(real[..., None], rows, torch.zeros_like(rows))
    return want, coords[idx.clamp(min=0)] * real[..., None]


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("cols", [1, 7, 48, 1024, 1030])
def test_gather_equals_torch_indexing_bit_for_bit(gpu, cols, pair):
    """Every combination of n_bags {1, 3} x bag_size {1, 5, 64} x out_ld {cols, round_up(cols, 256)}, on a packed store and on a pitched one (pitch a multiple
    of 8: the 16-byte path with a chunk that straddles `cols`), into a guarded output poisoned with 0xFF: equal bits (so every byte inside was written:
    the expected values hold no all-ones pattern), zero pad columns and padding rows, bands intact; the coordinates likewise."""
    sdt, odt = PAIRS[pair]
    g = torch.Generator().manual_seed(cols)
    coords = (torch.randint(0, 500, (ROWS, 2), generator=g).float() * 256.0).to(gpu)
    for store_ld in (cols, _round_up(cols, 8) + 8):
        store = _store(cols, sdt, store_ld).to(gpu)[:, :cols]
        for n_bags in (1, 3):
            for bag in (1, 5, 64):
                variants = [_idx(n_bags, bag, g)]
                if n_bags * bag == 1:
                    variants += [torch.tensor([[0]]), torch.tensor([[-1]])]
                for idx in variants:
                    idx = idx.to(gpu)
                    for out_ld in (cols, _round_up(cols, 256)):
                        out, ho = gd.guarded((n_bags * bag, out_ld), odt, gpu, pattern=0xFF, name="bags_out")
                        cout, hc = gd.guarded((n_bags * bag, 2), torch.float32, gpu, pattern=0xFF, name="coords_out")
                        got, gotc = ops.bag_batch_gather(store, coords, idx, odt, out_ld=out_ld, out=out.view(-1), coords_out=cout.view(-1))
                        torch.cuda.synchronize()
                        want, wantc = _expect(store, coords, idx, odt, out_ld)
                        where = (cols, pair, store_ld, n_bags, bag, out_ld)
                        assert got.shape == (n_bags, bag, cols) and got.data_ptr() == out.data_ptr(), where
                        assert torch.equal(_bits(out.view(n_bags, bag, out_ld)), _bits(want)), where
                        assert torch.equal(_bits(gotc), _bits(wantc.contiguous())), where
                        ho.assert_bands_intact()
                        hc.assert_bands_intact()
    # without coordinates; an empty batch launches nothing
    got, none = ops.bag_batch_gather(store, None, idx, odt)
    assert none is None and torch.equal(_bits(got), _bits(_expect(store, coords, idx, odt, cols)[0]))
    got, _ = ops.bag_batch_gather(store, None, idx[:0], odt)
    assert got.shape == (0, idx.shape[1], cols)


def test_gather_from_a_store_just_past_2_gib(gpu):
    """1.1 M fp16 rows of 1 024 = 2.25 GB, allocated uninitialised; only the 2 x 64 sampled rows are written -- half of them in the store's last MiB, the
    others including row 0 and the two rows on either side of the 2 GiB byte offset -- and gathered bit-exactly: a 32-bit byte offset cannot reach them."""
    R, Fd, bag = 1_100_000, 1024, 64
    assert R * Fd * 2 > 2 ** 31
    store = torch.empty(R, Fd, dtype=torch.float16, device=gpu)
    g = torch.Generator().manual_seed(0)
    last = R - 1 - torch.randperm(512, generator=g)[:bag]                     # the last MiB = the last 512 rows
    edge = torch.tensor([0, 2 ** 31 // (Fd * 2) - 1, 2 ** 31 // (Fd * 2), R - 513])
    rest = torch.randperm(R - 1024, generator=g)[:bag - edge.numel()] + 1
    rows = torch.cat([edge, rest, last])
    rows = rows[torch.randperm(rows.numel(), generator=g)]
    assert rows.unique().numel() == 2 * bag
    data = torch.randn(2 * bag, Fd, generator=g).half().to(gpu)
    store[rows.to(gpu)] = data
    for odt in (torch.float32, torch.float16):
        got, _ = ops.bag_batch_gather(store, None, rows.view(2, bag).to(gpu), odt)
        assert torch.equal(_bits(got.reshape(2 * bag, Fd)), _bits(data.to(odt)))


# ---- the cohort against BagDataset ---------------------------------------------------------------------------------------------------------------
BAG, FD = 64, 48
PATIENTS = [(1, 1), (37, 2), (64, 3), (65, 1), (700, 3), (65, 2), (700, 1)]          # (tiles, slides)
LABELS = ["pos", "neg", "pos", "pos", "neg", "neg", "pos"]
MULTI = [{"a": "x", "b": "u"}, {"a": "y", "b": "v"}, {"a": "x", "b": "w"}, {"a": "y", "b": None}, {"a": "x", "b": "v"}, {"a": "y", "b": "u"}, {"a": "x", "b": "w"}]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cohort")
    rng = np.random.default_rng(0)
    out = []
    for i, (n, slides) in enumerate(PATIENTS):
        cuts = [0] + sorted(rng.choice(np.arange(1, n), slides - 1, replace=False).tolist()) + [n] if slides > 1 else [0, n]
        fs = []
        for s in range(slides):
            k = cuts[s + 1] - cuts[s]
            feats = (rng.standard_normal((k, FD)) + (1.0 if LABELS[i] == "pos" else -1.0)).astype(np.float16)
            coords = np.stack([rng.integers(0, 60, k), rng.integers(0, 60, k)], 1).astype(np.float32) * 256.0
            p = d / f"p{i}_s{s}.h5"
            h5io.write_tile_features(p, feats, coords, extractor="test", tile_size_um=256.0, tile_size_px=224, code_hash="0", stamp_version="2.4.0")
            fs.append(p)
        out.append(fs)
    return out


@pytest.fixture(scope="module")
def cohort(gpu, files):
    return ResidentCohort([B.PatientData(ground_truth=g, feature_files=f) for g, f in zip(LABELS, files)], task="classification", device=gpu)


def _dataset(files, gts, bag_size, deterministic):
    targets, _ = B.parse_targets(patient_data=[B.PatientData(ground_truth=g, feature_files=f) for g, f in zip(gts, files)], task="classification")
    return B.BagDataset(bags=files, bag_size=bag_size, ground_truths=targets, transform=None, deterministic=deterministic)


def _reference_epoch(ds, order, batch_size, collate):
    items = [ds[int(i)] for i in order]          # num_workers=0: items are fetched, and draw, in batch order
    return [collate(items[a:a + batch_size]) for a in range(0, len(items), batch_size)]


def _same_batch(got, want):
    (gb, gc, gs, gt), (wb, wc, ws, wt) = got, want
    assert gb.dtype == torch.float32 and gb.is_cuda and gc.is_cuda and gs.is_cuda
    assert torch.equal(_bits(gb.cpu()), _bits(wb)) and torch.equal(_bits(gc.cpu()), _bits(wc.float())) and torch.equal(gs.cpu(), ws)
    if isinstance(wt, dict):
        assert list(gt) == list(wt) and all(torch.equal(gt[k].cpu(), wt[k]) for k in wt)
    else:
        assert torch.equal(gt.cpu(), wt)


def test_cohort_store_is_the_files(cohort, files):
    assert cohort.dtype == torch.float16 and cohort.feats.shape == (sum(n for n, _ in PATIENTS), FD) and cohort.lengths == [n for n, _ in PATIENTS]
    assert cohort.nbytes == cohort.feats.numel() * 2 + cohort.coords.numel() * 4 and cohort.load_seconds > 0
    ds = _dataset(files, LABELS, None, True)
    for p, (vb, vc, vs, vt) in enumerate(cohort.valid_batches()()):
        wb, wc, wn, wt = ds[p]
        assert vb.shape == (1, wn, FD) and torch.equal(vb[0].float().cpu(), wb) and torch.equal(vc[0].cpu(), wc) and int(vs) == wn and torch.equal(vt[0].cpu(), wt)
        assert vb.untyped_storage().data_ptr() == cohort.feats.untyped_storage().data_ptr()          # a view of the store, not a copy


def test_cohort_batches_equal_bagdataset_deterministic(cohort, files):
    ds = _dataset(files, LABELS, BAG, True)
    got = list(cohort.train_batches(3, BAG, shuffle=False)())
    want = _reference_epoch(ds, range(len(ds)), 3, B.collate_to_tuple)
    assert len(got) == len(want) == 3
    for g_, w_ in zip(got, want):
        _same_batch(g_, w_)
    assert len(list(cohort.train_batches(3, BAG, shuffle=False, drop_last=True)())) == 2


def test_cohort_batches_equal_bagdataset_seeded_random(cohort, files):
    """One seeded generator (torch's global one, which BagDataset draws from): the epoch's randperm first, then the bags' draws in batch order -- twice, so
    the second epoch starts from the state the first one left."""
    ds = _dataset(files, LABELS, BAG, False)
    torch.manual_seed(11)
    feed = cohort.train_batches(3, BAG, shuffle=True)
    got = [list(feed()) for _ in range(2)]
    torch.manual_seed(11)
    for epoch in got:
        order = torch.randperm(len(ds))
        want = _reference_epoch(ds, order, 3, B.collate_to_tuple)
        assert len(epoch) == len(want)
        for g_, w_ in zip(epoch, want):
            _same_batch(g_, w_)
    # an explicit generator gives the plan of that generator
    idx, _ = cohort.plan_indices([4, 6], BAG, False, torch.Generator().manual_seed(3))
    g2 = torch.Generator().manual_seed(3)
    assert torch.equal(idx[0], torch.randperm(700, generator=g2)[:BAG] + cohort.offsets[4]) and torch.equal(idx[1], torch.randperm(700, generator=g2)[:BAG] + cohort.offsets[6])


def test_cohort_multi_target_batches(gpu, files):
    mc = ResidentCohort(feature_files=files, ground_truths=MULTI, task="classification", device=gpu)
    ds = _dataset(files, MULTI, BAG, False)
    torch.manual_seed(5)
    got = list(mc.train_batches(4, BAG, shuffle=True)())
    torch.manual_seed(5)
    want = _reference_epoch(ds, torch.randperm(len(ds)), 4, B.collate_multitarget)
    assert len(got) == len(want) == 2
    for g_, w_ in zip(got, want):
        _same_batch(g_, w_)
    three = next(iter(mc.barspoon_batches(4, BAG, shuffle=False)()))
    assert len(three) == 3 and set(three[2]) == {"a", "b"}


# ---- the fused vary_precision ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols,store_ld,out_ld", [(48, 48, 48), (1024, 1024, 1024), (7, 7, 7), (52, 56, 256), (1030, 1030, 1280)])
def test_fused_vary_precision_masks_with_the_exported_shifts(gpu, cols, store_ld, out_ld):
    """out = cast(fp32 bits & (~0 << s)) with s from amds_bag_batch_shifts, bit for bit, on the 16-byte path (aligned chunks, a straddling chunk) and the
    element-wise one; the shifts do not depend on idx; 22 bits leave one shift value, 0 = the identity."""
    g = torch.Generator().manual_seed(cols)
    store = _store(cols, torch.float16, store_ld).to(gpu)[:, :cols]
    n_bags, bag, seed, sid = 3, 5, 0x1234_5678_9ABC, 9
    for bits in (1, 2, 13):
        shifts = ops.bag_batch_shifts(n_bags, bag, cols, bits, seed, sid, gpu)
        assert int(shifts.max()) < 23 - bits
        for idx in (_idx(n_bags, bag, g).to(gpu), _idx(n_bags, bag, g).to(gpu)):
            plain, _ = ops.bag_batch_gather(store, None, idx, torch.float32)
            masked = (_bits(plain) & (torch.full_like(shifts, -1, dtype=torch.int32) << shifts.to(torch.int32))).view(torch.float32)
            for odt in (torch.float32, torch.float16, torch.bfloat16):
                got, _ = ops.bag_batch_gather(store, None, idx, odt, out_ld=out_ld, vary_precision_bits=bits, seed=seed, stream_id=sid)
                assert torch.equal(_bits(got), _bits(masked.to(odt))), (bits, odt)
        assert not torch.equal(shifts, ops.bag_batch_shifts(n_bags, bag, cols, bits, seed + 1, sid, gpu)) or cols * n_bags * bag < 64
        assert not torch.equal(shifts, ops.bag_batch_shifts(n_bags, bag, cols, bits, seed, sid + 1, gpu)) or cols * n_bags * bag < 64
    idx = _idx(n_bags, bag, g).to(gpu)
    plain, _ = ops.bag_batch_gather(store, None, idx, torch.float32)
    same, _ = ops.bag_batch_gather(store, None, idx, torch.float32, vary_precision_bits=22, seed=seed, stream_id=sid)
    assert torch.equal(_bits(same), _bits(plain)) and int(ops.bag_batch_shifts(n_bags, bag, cols, 22, seed, sid, gpu).max()) == 0


@pytest.mark.parametrize("bits", [1, 2, 10, 21])
def test_fused_vary_precision_shifts_are_uniform(gpu, bits):
    """2^20 elements: every shift value 0 .. k - 1 (k = 23 - bits) within 3e-3 of 1 / k -- the bar of the dropout-mask test; the standard deviation of a fair
    source's frequency is sqrt(p (1 - p) / 2^20) <= 5e-4 (k = 2) and about 2e-4 at k = 21."""
    k = 23 - bits
    s = ops.bag_batch_shifts(4, 256, 1024, bits, 2024, 3, gpu)
    freq = torch.bincount(s.view(-1).to(torch.int64), minlength=k).double().cpu() / s.numel()
    print(f"bits {bits}: k {k}, max |freq - 1/k| = {(freq - 1 / k).abs().max().item():.3e}")
    assert freq.numel() == k and (freq - 1 / k).abs().max().item() < 3e-3, freq


# ---- training from either feed ---------------------------------------------------------------------------------------------------------------------
def test_fit_on_the_resident_cohort_equals_fit_on_the_bagdataset_feed(gpu, cohort, files):
    """Two epochs, dropout off: the loss history of `fit` fed by the cohort (gathered on the device, validated on views of the store) equals, float for float,
    the history of `fit` fed by batches built through BagDataset + collate_to_tuple from the same seed."""
    from stamp_amd.mil import VisionTransformer
    from stamp_amd.mil_train import HipMilVitTrainer, fit
    torch.manual_seed(0)
    model = VisionTransformer(dim_output=2, dim_input=FD, dim_model=64, n_layers=1, n_heads=2, dim_feedforward=64, dropout=0.0, use_alibi=False)
    make = lambda m: HipMilVitTrainer(m, device=gpu, max_lr=3e-3, total_steps=12, sched_interval="step", dropout=False)  # noqa: E731
    tr_a, tr_b = make(copy.deepcopy(model)), make(copy.deepcopy(model))
    torch.manual_seed(21)
    hist_a = fit(tr_a, cohort.train_batches(3, BAG, shuffle=True), cohort.valid_batches(), max_epochs=2, patience=8)
    ds_t, ds_v = _dataset(files, LABELS, BAG, False), _dataset(files, LABELS, None, True)
    torch.manual_seed(21)
    epochs = iter([_reference_epoch(ds_t, torch.randperm(len(ds_t)), 3, B.collate_to_tuple) for _ in range(2)])
    valid = _reference_epoch(ds_v, range(len(ds_v)), 1, B.collate_to_tuple)
    hist_b = fit(tr_b, lambda: next(epochs), lambda: valid, max_epochs=2, patience=8)
    print("resident:", hist_a["train_loss"], hist_a["validation_loss"], "\nbagdataset:", hist_b["train_loss"], hist_b["validation_loss"])
    assert hist_a["train_loss"] == hist_b["train_loss"] and hist_a["validation_loss"] == hist_b["validation_loss"]
    assert all(np.isfinite(hist_a["train_loss"])) and torch.equal(tr_a.P, tr_b.P)
    # grouped validation (`valid_bags_per_call`) takes the store's views as they are
    hist_c = fit(tr_a, cohort.train_batches(3, BAG, shuffle=False), cohort.valid_batches(), max_epochs=1, valid_bags_per_call=4)
    assert np.isfinite(hist_c["validation_loss"][0])


def test_barspoon_trainer_fits_from_barspoon_batches(gpu, files):
    from stamp_amd.barspoon import EncDecTransformer
    from stamp_amd.barspoon_train import HipBarspoonTrainer
    mc = ResidentCohort(feature_files=files, ground_truths=MULTI, task="classification", device=gpu)
    assert mc.categories == {"a": ["x", "y"], "b": ["u", "v", "w"]}
    torch.manual_seed(0)
    model = EncDecTransformer(FD, {"a": 2, "b": 3}, d_model=128, num_encoder_heads=4, num_decoder_heads=2, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=192)
    tr = HipBarspoonTrainer(model, device=gpu, learning_rate=1e-3, dropout=False)
    torch.manual_seed(2)
    hist = tr.fit(mc.barspoon_batches(4, BAG, shuffle=True), mc.barspoon_valid_batches(), max_epochs=1)
    assert tr.steps == 2 and np.isfinite(hist["train_loss"][0]) and np.isfinite(hist["validation_loss"][0])


# ---- ragged views of the store --------------------------------------------------------------------------------------------------------------------
def _group_as_list(cohort, a, e):
    return ([cohort.feats[cohort.offsets[p]:cohort.offsets[p + 1]].clone() for p in range(a, e)],
            [cohort.coords[cohort.offsets[p]:cohort.offsets[p + 1]].clone() for p in range(a, e)])


@pytest.mark.parametrize("a,e", [(0, 7), (1, 5), (4, 5)])
def test_ragged_group_is_a_view_the_ragged_forwards_take(gpu, cohort, a, e):
    """`forward_infer_ragged(ragged_group(a, e))` == `forward_ragged` on the list of the same bags, bit for bit, for the `vit` head (with and without ALiBi),
    TransMIL and barspoon; the group is a slice of the store (no copy) with offsets rebased to it."""
    from stamp_amd.barspoon import EncDecTransformer
    from stamp_amd.mil import TransMIL, VisionTransformer
    rb = cohort.ragged_group(a, e)
    assert rb.feats.data_ptr() == cohort.feats.data_ptr() + cohort.offsets[a] * FD * 2 and rb.coords.data_ptr() == cohort.coords.data_ptr() + cohort.offsets[a] * 8
    assert rb.offsets.dtype == torch.int32 and rb.offsets.cpu().tolist() == [o - cohort.offsets[a] for o in cohort.offsets[a:e + 1]]
    assert rb.lengths == tuple(cohort.lengths[a:e]) and rb.feats.shape[0] == rb.total_tiles
    bags, coords = _group_as_list(cohort, a, e)
    torch.manual_seed(1)
    heads = [VisionTransformer(dim_output=3, dim_input=FD, dim_model=64, n_layers=2, n_heads=2, dim_feedforward=64, dropout=0.0, use_alibi=alibi).eval().to(gpu)
             for alibi in (False, True)]
    heads.append(TransMIL(dim_output=3, dim_input=FD, dim_hidden=128).eval().to(gpu))
    with torch.no_grad():
        for m in heads:
            got, want = m.forward_infer_ragged(rb), m.forward_ragged(bags, coords=coords)
            assert got.shape == (e - a, 3) and torch.isfinite(got).all() and torch.equal(got, want), type(m).__name__
        bs = EncDecTransformer(FD, {"a": 2, "b": 3}, d_model=128, num_encoder_heads=4, num_decoder_heads=2, num_encoder_layers=1, num_decoder_layers=1,
                               dim_feedforward=192).eval().to(gpu)
        got, want = bs.forward_infer_ragged(rb), bs.forward_ragged(bags, coords)
        assert set(got) == {"a", "b"} and all(torch.equal(got[t], want[t]) and torch.isfinite(got[t]).all() for t in want)
    with pytest.raises(ValueError):
        cohort.ragged_group(3, 99)
