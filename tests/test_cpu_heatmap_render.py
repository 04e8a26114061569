"""Heat-map rendering without a GPU: tests/heatmap_render_oracle.py (plain numpy) reproduces, byte for byte, what matplotlib, Pillow and the reference's own
`_vals_to_im`, `_show_class_map` and `_create_overlay` returned (tests/golden/heatmap_render.npz, tools/make_heatmap_render_golden.py); the committed colour
tables and the running-sum resize table against the libraries where they are installed; the host side of `stamp_amd.heatmaps`' new entry points."""
from pathlib import Path

import numpy as np
import pytest
import torch

import heatmap_render_oracle as oracle
from stamp_amd import heatmaps

G = Path(__file__).parent / "golden"
THUMBS = ("56x40", "53x37", "17x91", "1x1")
OPACITIES = (0.6, 0.35)


@pytest.fixture(scope="module")
def z():
    with np.load(G / "heatmap_render.npz") as f:
        return {k: f[k] for k in f.files}


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert int((got != want).sum()) == 0, f"{what}: {int((got != want).sum())} differing bytes"


def test_lookup_rule_reproduces_matplotlib(z):
    for name in ("RdBu_r", "magma", "Reds"):
        _same(oracle.lut_float(z["probe"], heatmaps.colormap_table(name)), z[f"probe_{name}"], name)
    # outside [0, 1] and NaN: under -> lut[0], over -> lut[N - 1], bad -> (0, 0, 0, 0)
    lut = heatmaps.colormap_table("RdBu_r")
    got = oracle.lut_float(z["edge"], lut)
    _same(got, z["edge_RdBu_r"], "edge values")
    assert (got[:4] == lut[0]).all() and (got[4:7] == lut[255]).all() and (got[7] == 0).all()
    pastel = heatmaps.colormap_table("Pastel1")
    assert pastel.shape == (9, 4)
    _same(oracle.lut_int(z["pastel_idx"], pastel), z["pastel_rgba"], "Pastel1 integer look-up")
    assert (oracle.lut_int([9, 11], pastel) == pastel[8]).all()


def test_oracle_reproduces_classification_rasters_and_overlays(z):
    cn = z["coords_norm"]
    cell = oracle.cell_table(cn)
    assert cell.shape == (7, 5) and (cell < 0).sum() == 13 and cell[cn[3, 1], cn[3, 0]] == 17          # empty cells; two tiles on one cell
    lut = heatmaps.colormap_table("RdBu_r")
    for C in (2, 3):
        arg = z[f"cs{C}"] / np.float32(2) + np.float32(0.5)
        for v in (0.0, 1.0, 0.5, 1 / 256, 192 / 256, np.nextafter(np.float32(192 / 256), np.float32(0))):          # the planted arguments arrive
            assert (arg == np.float32(v)).any(axis=1).all(), v
        assert (z[f"att{C}"][C - 1] <= 0).all()
        got = oracle.raster(arg, z[f"att{C}"], lut, cell=cell, scale=8)
        _same(got, z[f"rgba{C}"], f"score image C={C}")
        assert (got[C - 1, ..., 3] == 0).all() and (got[0, ..., 3] == 255).any()
        empty = np.repeat(np.repeat(cell < 0, 8, 0), 8, 1)
        assert (got[:, empty][..., :3] == lut[0, :3]).all() and (got[:, empty][..., 3] == 0).all()          # `_vals_to_im`'s zero fill: lut[0], not the colour of 0.5
        unscaled = oracle.raster(arg, z[f"att{C}"], lut, cell=cell, scale=1)
        for t in THUMBS:
            for o in OPACITIES:
                want = z[f"ov{C}_{t}_{o}"]
                _same(oracle.overlay(unscaled, z[f"thumb_{t}"], o), want, f"overlay C={C} {t} {o}")
                _same(oracle.overlay(got, z[f"thumb_{t}"], o, scale=8), want, f"overlay of the x8 image C={C} {t} {o}")
                keep = np.broadcast_to((want != z[f"thumb_{t}"][None]).any(-1), want.shape[:-1])
                assert not keep[C - 1].any()          # an unblended pixel is the thumbnail's byte


def test_oracle_reproduces_class_map(z):
    cell = oracle.cell_table(z["coords_norm"])
    top = oracle.top_class(z["cm_scores"])
    assert top[2] == 3 and z["cm_scores"][2, 3] == z["cm_scores"][2, 5] and {8, 9, 11} <= set(top.tolist())
    has = cell >= 0
    assert (oracle._gather(top[None], cell)[0][has] == z["cm_top_2d"][has]).all()          # the tie goes where torch.topk on the CPU sends it
    got = oracle.classmap(top, z["cm_gradcam"].sum(-1), heatmaps.colormap_table("Pastel1"), cell=cell, scale=8)
    want = z["cm_rgba"]
    assert got.shape == want.shape and (got[..., 3] == want[..., 3]).all()          # alpha everywhere, RGB where something is drawn
    on = want[..., 3] == 255
    assert on.any() and (~on).sum() > 13 * 64 and (got[on] == want[on]).all()
    gridded = oracle.classmap(oracle._gather(top[None], cell)[0], oracle._gather(z["cm_gradcam"].sum(-1)[None], cell)[0],
                              heatmaps.colormap_table("Pastel1"), scale=8)
    _same(gridded, got, "gridded class map")


def test_oracle_reproduces_regression_and_survival(z):
    cell = oracle.cell_table(z["coords_norm"])
    alpha = oracle._gather(z["reg_gradcam"][None], cell)
    g = z["reg_g2d"]
    args = {"reg": ("magma", g), "surv": ("Reds", g)}
    for tag, med in zip(("neg", "pos"), z["surv_medians"]):
        arg = oracle.survival_arg(g, float(med))
        assert arg.dtype == np.float32 and (arg.view(np.int32) == z[f"surv_{tag}_arg"].view(np.int32)).all()          # bit-equal to torch's
        args[f"surv_{tag}"] = ("RdBu_r", arg)
    assert z["surv_medians"][0] < 0 < z["surv_medians"][1]
    for key, (cmap, x) in args.items():
        unscaled = oracle.raster(x[None], alpha, heatmaps.colormap_table(cmap), scale=1)
        _same(oracle.raster(x[None], alpha, heatmaps.colormap_table(cmap), scale=8), z[f"{key}_rgba"], key)
        _same(oracle.overlay(unscaled, z["thumb_53x37"], 0.6), z[f"{key}_ov_53x37_0.6"], key + " overlay")


def test_committed_tables_equal_matplotlib(z):
    mpl = pytest.importorskip("matplotlib")
    import json
    recorded = json.loads(Path(heatmaps.__file__).with_name("colormaps.json").read_text())["matplotlib_version"]
    if mpl.__version__ != recorded:
        pytest.skip(f"tables recorded from matplotlib {recorded}, installed {mpl.__version__}")
    for name in heatmaps.COLORMAPS:
        cmap = mpl.colormaps[name]
        _same(heatmaps.colormap_table(name), np.uint8(cmap(np.arange(cmap.N)) * 255), name)


def test_running_sum_table_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    pairs = [(int(a), int(b)) for a, b in rng.integers(1, 400, size=(50, 2))] + [(7, 56), (7, 53), (5, 37), (7, 17), (5, 91), (7, 1), (300, 2395), (200, 1597)]
    closed_form_differs = 0
    for n_in, n_out in pairs:
        src = np.arange(n_in, dtype=np.int32)[None, :]
        want = np.array(Image.fromarray(src).resize((n_out, 1), resample=Image.Resampling.NEAREST))[0]
        tab = heatmaps.resize_index_table(n_in, n_out)
        assert tab == want.tolist() == oracle.resize_table(n_in, n_out).tolist(), (n_in, n_out)
        closed_form_differs += tab != [int(np.floor((i + 0.5) * (n_in / n_out))) for i in range(n_out)]
    print(f"running sum vs closed form: {closed_form_differs} of {len(pairs)} size pairs differ")


def test_cpu_tensors_raise():
    arg, thumb = torch.rand(2, 6), torch.zeros(4, 4, 3, dtype=torch.uint8)
    cn = torch.tensor([[0, 0], [1, 0], [2, 0], [0, 1], [1, 1], [2, 1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        heatmaps.colorize(arg, arg, "RdBu_r", coords_norm=cn)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        heatmaps.colorize(torch.rand(2, 3, 3), torch.rand(2, 3, 3), "magma")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        heatmaps.class_map(torch.zeros(6, dtype=torch.long), arg[0], coords_norm=cn)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        heatmaps.overlay(torch.zeros(1, 2, 3, 4, dtype=torch.uint8), thumb)
    hm = heatmaps.SlideHeatmap("regression", torch.zeros(()), cn, torch.rand(6), torch.rand(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hm.render(thumb)
    with pytest.raises(ValueError, match="survival"):
        hm.render(train_pred_median=0.1)
    import stamp_amd
    assert stamp_amd.colorize is heatmaps.colorize and stamp_amd.ranked_tiles is heatmaps.ranked_tiles and stamp_amd.HeatmapImages is heatmaps.HeatmapImages


def test_task_survival_is_accepted():
    """The task check lets "survival" through to the device check (a CPU bag then raises the no-CPU-fallback error); an unknown task is still a ValueError."""
    model = torch.nn.Linear(4, 1)
    feats, coords = torch.rand(5, 4), torch.rand(5, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        heatmaps.slide_heatmap(model, feats, coords, task="survival")
    with pytest.raises(ValueError, match="task must be"):
        heatmaps.slide_heatmap(model, feats, coords, task="ranking")


def test_ranked_tiles_order_and_ties():
    s = torch.tensor([0.5, 0.9, 0.1, 0.9, 0.1, 0.7, 0.1])
    ti, tv, bi, bv = heatmaps.ranked_tiles(s, 3, 4)
    assert ti.tolist() == [1, 3, 5] and tv.tolist() == s[[1, 3, 5]].tolist()          # equal scores: the lower tile index first
    assert bi.tolist() == [2, 4, 6, 0] and bv.tolist() == s[[2, 4, 6, 0]].tolist()
    ti, tv, bi, bv = heatmaps.ranked_tiles(s, 100, 0)          # k = min(k, N); k = 0 selects nothing
    assert ti.tolist() == [1, 3, 5, 0, 2, 4, 6] and bi.numel() == 0 and bv.numel() == 0
    assert torch.equal(tv, s[ti])
    ti, _, bi, _ = heatmaps.ranked_tiles(s.reshape(7, 1), 1, 1)          # the reference flattens
    assert ti.tolist() == [1] and bi.tolist() == [2]
