"""tests/gap_oracle.py pinned on the CPU: the fp64 reference against oracle/gated_attention.py and the reference fixtures, every family-I case exact in fp32, K_FN
measured on the plain fp32 evaluation, and every reference-side mutant caught by the bars (a case no mutant can fail would prove nothing on the GPU)."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import gap_oracle as O
from oracle.gated_attention import KEYS, gated_attention_pool

GOLD = Path(__file__).parent / "golden"
MUTANT_GEOMS = {"offsets_minus_256": ("bags257", "ragged300"), "drop_cols_1024": ("f1040",)}
GRID_CASES = [(g, f) for g, v in O.GEOMS.items() for f in v[5] if f in O.GRID_FAMILIES]
REAL_CASES = [(g, f) for g, v in O.GEOMS.items() for f in v[5] if f in O.REAL_FAMILIES]


@functools.lru_cache(maxsize=None)
def _case(geom, family):
    x, lengths, w = O.build_case(geom, family)
    return x, lengths, w, O.reference(x, lengths, w)


def _sd(w):
    return {KEYS[k]: w[k] for k in O.KEYS}


def test_reference_matches_the_oracle_taken_to_fp64(monkeypatch):
    x, lengths, w = O.build_case("f32d64", "gaussian")
    ref = O.reference(x, lengths, w)
    sd64 = {k: v.double() for k, v in _sd(w).items()}
    monkeypatch.setattr(torch.Tensor, "float", lambda t: t.double())          # gated_attention_pool casts its weights with .float(): here that keeps fp64
    o = 0
    for i, n in enumerate(lengths):
        r = gated_attention_pool(x[o:o + n].double(), sd64)
        assert r["WSI_feature"].dtype == torch.float64
        np.testing.assert_allclose(ref.A[o:o + n].numpy(), r["attention_raw"].reshape(-1).numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref.out[i].numpy(), r["WSI_feature"].reshape(-1).numpy(), rtol=1e-12, atol=1e-13)
        o += n


@pytest.mark.parametrize("tag", ["small", "xs"])
def test_reference_matches_the_reference_fixtures(tag):
    z = np.load(GOLD / f"chief_gated_attention_{tag}.npz")
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    w = {k: sd[v] for k, v in KEYS.items()}
    x = torch.from_numpy(z["x"])
    ref = O.reference(x, [x.shape[0]], w)
    np.testing.assert_allclose(ref.out[0].numpy(), z["wsi_feature"].reshape(-1), rtol=2e-5, atol=2e-6)         # test_gpu_seams.py's tolerances
    if "attention_raw" in z.files:
        np.testing.assert_allclose(ref.A.numpy(), z["attention_raw"].reshape(-1), rtol=1e-4, atol=1e-4)


def test_saturation_facts_and_probe_patterns():
    f = torch.tensor
    assert torch.equal(torch.tanh(f([-32.0, 32.0])), f([-1.0, 1.0]))
    assert torch.equal(1.0 / (1.0 + torch.exp(-f([-128.0, 32.0]))), f([0.0, 1.0])) and torch.equal(torch.sigmoid(f([-128.0, 32.0])), f([0.0, 1.0]))
    assert torch.exp(f([128.0])).isinf().all() and float(1.0 + torch.exp(f([-32.0]))) == 1.0 and float(torch.exp(f([-128.0]))) == 0.0
    for (k1, w1), (k2, w2) in O.PROBES:
        assert O.KF not in (k1, k2) and w1 * O.col_mult(k1) + w2 * O.col_mult(k2) == 0
        for s in (1, 2, 3):                         # an XOR swizzle of the 16-byte chunks pairs the weights with other multipliers: the payload no longer cancels
            assert w1 * O.col_mult(k1 ^ (4 * s)) + w2 * O.col_mult(k2 ^ (4 * s)) != 0
        assert w1 * O.col_mult(k1 ^ 1) + w2 * O.col_mult(k2 ^ 1) != 0
    # the gates of a flagged and an unflagged row sit exactly on the grid
    w = O.grid_weights(32, 256, 64)
    x = O.grid_x([2], 32, f([0.0, 1.0]))
    h = torch.relu(x @ w["fc_w"].T + w["fc_b"])
    assert set((h @ w["a_w"].T + w["a_b"]).reshape(-1).tolist()) == {-32.0, 32.0}
    assert set((h @ w["b_w"].T + w["b_b"]).reshape(-1).tolist()) == {-128.0, 32.0}


@pytest.mark.parametrize("geom,family", GRID_CASES)
def test_family_one_is_exact_in_fp32(geom, family):
    x, lengths, w, ref = _case(geom, family)
    A, out, num, den = O.evaluate_fp32(x, lengths, w)
    A64 = ref.A.float()                             # fp64 keeps sigmoid(32) = 1 - 1.3e-14 and sigmoid(-128) = 2.6e-56: "bit-equal to fp64" is after the cast
    assert torch.equal(A64, A64.round()) and float(A64.abs().max()) < 2 ** 24 and float(x.abs().max()) <= 48 and float((ref.A - A64).abs().max()) < 1e-9
    assert torch.equal(A, A64), "A_raw of the plain fp32 evaluation differs from fp64"
    gap = A64[:, None] - A64[None, :5]
    assert bool(((gap == 0) | (gap.abs() >= 128)).all())
    # exp(A - m) is 1 or 0: numerator and denominator are integer sums below 2^24
    assert torch.equal(den.double(), ref.nwin.double()) and float(num.abs().max()) < 2 ** 24
    numer64 = ref.num.float()                       # fp64 keeps exp(-128) ~ 1e-56 per losing row: it vanishes in the cast
    assert torch.equal(num, numer64)
    pow2 = (ref.nwin & (ref.nwin - 1)) == 0
    assert torch.equal(out[pow2], ref.out.float()[pow2])
    bar = O.grid_out_bar(ref)
    assert bool(((out.double() - ref.out).abs() <= bar + 2.0 ** -150).all())
    if family == "uniform":
        o = 0
        for i, n in enumerate(lengths[:8]):
            assert torch.allclose(ref.out[i], x[o:o + n].double().mean(0), rtol=1e-14, atol=0)
            o += n
    if family in ("winner", "two_winners", "winner_per_unit") and max(lengths) > 1:
        assert int((ref.nwin < torch.as_tensor(lengths)).sum()) > 0


def _fp32_plain(x, lengths, w):
    """The existing oracle bag by bag (the vectorised restatement where that loop would run 65 537 times)."""
    if len(lengths) > 400:
        A, out, _, _ = O.evaluate_fp32(x, lengths, w)
        return A, out
    sd, As, outs, o = _sd(w), [], [], 0
    for n in lengths:
        r = gated_attention_pool(x[o:o + n], sd)
        As.append(r["attention_raw"].reshape(-1))
        outs.append(r["WSI_feature"].reshape(1, -1))
        o += n
    return torch.cat(As), torch.cat(outs)


def _ratios(geom, family, k_fn):
    x, lengths, w, ref = _case(geom, family)
    A, out = _fp32_plain(x, lengths, w)
    barA, barO = O.real_bars(ref, O.depth_fused(ref.lengths, 64), k_fn)
    return float(((A.double() - ref.A).abs() / barA).max()), float(((out.double() - ref.out).abs() / barO.clamp_min(1e-300)).max())


def test_k_fn_is_the_smallest_that_fits(capsys):
    assert O.K_FN in (1, 2, 4, 8)
    worst = {k: (0.0, 0.0) for k in (O.K_FN, O.K_FN // 2)}
    for geom, family in REAL_CASES:
        for k in worst:
            if k:
                ra, ro = _ratios(geom, family, k)
                worst[k] = (max(worst[k][0], ra), max(worst[k][1], ro))
                if k == O.K_FN:
                    with capsys.disabled():
                        print(f"gap-cpu| plain fp32 | {geom} | {family} | A_raw {ra:.4f} | out {ro:.4f}")
    ra, ro = worst[O.K_FN]
    assert ra <= 0.5 and ro <= 0.5, (ra, ro)
    assert ra <= O.K_FN_WORST["A_raw"] and ro <= O.K_FN_WORST["out"], f"measured {ra:.4f} / {ro:.4f}: update K_FN_WORST"
    if O.K_FN > 1:
        assert max(worst[O.K_FN // 2]) > 0.5, "a smaller K_FN fits"


def _exceeds(geom, family, mutant):
    x, lengths, w, ref = _case(geom, family)
    mut = O.reference(x, lengths, w, mutant=mutant)
    if family in O.GRID_FAMILIES:
        barA, barO = torch.zeros_like(ref.A), O.grid_out_bar(ref)
    else:
        barA, barO = O.real_bars(ref, O.depth_fused(ref.lengths, 64))
    dA, dO = (mut.A - ref.A).abs(), (mut.out - ref.out).abs()
    return bool((dA > barA).any()) or bool((dO > barO).any()) or not bool(torch.isfinite(mut.out).all())


def test_every_mutant_fails_and_every_family_is_failed(capsys):
    failed_by = {f: [] for f in O.ALL_FAMILIES}
    for mutant in O.MUTANTS:
        caught = []
        for geom in MUTANT_GEOMS.get(mutant, ("l256",)):
            for family in O.GEOMS[geom][5]:
                if _exceeds(geom, family, mutant):
                    caught.append(f"{geom}/{family}")
                    failed_by[family].append(mutant)
        with capsys.disabled():
            print(f"gap-cpu| mutant {mutant} | exceeds the bar on: {' '.join(caught) or 'NOTHING'}")
        assert caught, f"mutant {mutant} passes every case"
    for family, ms in failed_by.items():
        assert ms, f"no mutant fails family {family}"
