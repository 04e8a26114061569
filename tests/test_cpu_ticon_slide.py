"""TICON slide mode without a GPU: the fp64 restatement the GPU tests lean on (tests/chains/ticon_slide.py) against the reference's own float64 run
(tests/golden/ticon_slide.npz), the host slope rule, and the one-token case against the tile-mode oracle."""
from pathlib import Path

import numpy as np
import pytest
import torch

from chains.ticon_slide import MODELS, load_fixture, ticon_slide_forward

GOLD = Path(__file__).parent / "golden"
CASES = [(tag, name) for tag in MODELS for name in ("b2_hoptimus1", "b2_conchv15", "n70", "n1")]


def _batched(c):
    emb, coords, out64 = c["emb"], c["coords"], c["out64"]
    return (emb, coords, out64) if emb.dim() == 3 else (emb[None], coords[None], out64[None])


@pytest.mark.parametrize("tag,name", CASES)
def test_restatement_fp64_matches_the_reference_run(tag, name):
    """max |restatement - out64| <= 1e-9 max |out64|: fp32 against fp64 is 3-5e-7 on these cases, a wrong formula is of order 1 (the stored out64 is
    the float64 run to 2^-33 relative)."""
    fx = load_fixture()
    m, c = fx[tag], fx[tag]["cases"][name]
    emb, coords, out64 = _batched(c)
    got = ticon_slide_forward(emb.double(), coords.double(), m["sd"], c["key"], m["heads"], fx["slopes"][m["heads"]])
    assert got.shape == out64.shape and got.dtype == torch.float64
    err = (got - out64).abs().max().item()
    print(f"{tag}/{name}: max abs {err:.3e}, max |out64| {out64.abs().max().item():.3e}")
    assert err <= 1e-9 * out64.abs().max().item()


def test_fixture_holds_the_cases_the_gpu_tests_use():
    fx = load_fixture()
    assert (fx["a"]["dim"], fx["a"]["heads"], fx["a"]["depth"]) == (192, 3, 2) and (fx["b"]["dim"], fx["b"]["heads"], fx["b"]["depth"]) == (96, 6, 3)
    for tag in MODELS:
        cs = fx[tag]["cases"]
        assert {cs[f"b2_{k}"]["key"] for k in fx[tag]["keys"]} == set(fx[tag]["keys"])
        for k in fx[tag]["keys"]:
            c = cs[f"b2_{k}"]
            assert c["emb"].shape[:2] == (2, 150) and c["coords"].shape == (2, 150, 2)
            for b in range(2):      # distinct cells of a 20 x 20 grid
                assert len({(int(x), int(y)) for x, y in c["coords"][b].tolist()}) == 150 and c["coords"][b].max() < 20
            assert torch.equal(c["emb"], c["emb"].half().float())
        assert cs["n70"]["emb"].dim() == 2 and cs["n70"]["emb"].shape[0] == 70 and bool((cs["n70"]["coords"] % 1 != 0).any())
        assert cs["n1"]["emb"].shape[0] == 1 and not bool(cs["n1"]["coords"].any())
        for c in cs.values():       # the fp32 run of the reference sits within fp32 rounding of its fp64 run
            assert (c["out"].double() - c["out64"]).abs().max() < 1e-5 * c["out64"].abs().max()


@pytest.mark.parametrize("heads", [3, 6, 24])
def test_host_slopes_are_the_references(heads):
    from stamp_amd.ticon import alibi_slopes
    want = load_fixture()["slopes"][heads]
    got = np.array(alibi_slopes(heads), dtype=np.float32)
    assert want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want)


def test_host_slopes_powers_of_two_and_in_between():
    from stamp_amd.ticon import alibi_slopes
    assert alibi_slopes(8) == [2.0 ** -(i + 1) for i in range(8)]
    assert alibi_slopes(1) == [2.0 ** -8]
    s12 = alibi_slopes(12)
    assert s12[:8] == alibi_slopes(8) and s12[8:] == alibi_slopes(16)[0::2][:4]
    with pytest.raises(ValueError):
        alibi_slopes(0)


def test_one_tile_is_tile_mode():
    """N = 1, zero coordinates: the softmax over one key is 1, so slide mode is the tile-mode oracle -- on the slide fixture's model b (the geometry of
    ticon.npz) against the reference's float64 run, and on ticon.npz's own weights and embeddings."""
    from oracle.ticon import ticon_tile_forward
    fx = load_fixture()
    m, c = fx["b"], fx["b"]["cases"]["n1"]
    tile = ticon_tile_forward(c["emb"].double(), m["sd"], c["key"])
    assert (tile - c["out64"]).abs().max() <= 1e-9 * c["out64"].abs().max()
    z = np.load(GOLD / "ticon.npz")
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    for key in ("hoptimus1", "conchv15"):
        emb = torch.from_numpy(z[f"emb_{key}"]).double()
        got = ticon_slide_forward(emb[:, None], torch.zeros(emb.shape[0], 1, 2, dtype=torch.float64), sd, key, 6, fx["slopes"][6])[:, 0]
        want = torch.from_numpy(z[f"out64_{key}"])
        assert (got - want).abs().max() <= 1e-9 * want.abs().max()
        assert (got - ticon_tile_forward(emb, sd, key)).abs().max() <= 1e-12 * want.abs().max()


def test_context_matters_in_the_fixture():
    """What a build that ignored coordinates or context would miss: slide mode is far from tile mode on the fixture -- 0.79-0.89 relative L2 on the
    unit grid, 0.48-0.50 where the grid is 37.5 wide (the bias then nearly isolates a tile under the steepest slopes)."""
    from oracle.ticon import ticon_tile_forward
    fx = load_fixture()
    for tag in MODELS:
        m = fx[tag]
        for name, least in ((f"b2_{m['keys'][0]}", 0.7), (f"b2_{m['keys'][1]}", 0.7), ("n70", 0.4)):
            c = m["cases"][name]
            emb = c["emb"].double()
            tile = ticon_tile_forward(emb.reshape(-1, emb.shape[-1]), m["sd"], c["key"]).reshape(c["out64"].shape)
            rel = ((tile - c["out64"]).norm() / c["out64"].norm()).item()
            assert rel > least, (tag, name, rel)
