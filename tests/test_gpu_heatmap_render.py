"""Heat-map rendering on the GPU (`stamp_amd.heatmaps.colorize`, `class_map`, `overlay`, `SlideHeatmap.render` over amds_heatmap_raster,
amds_heatmap_classmap, amds_heatmap_overlay): bit-equal to what matplotlib, Pillow and the reference's own functions returned
(tests/golden/heatmap_render.npz) and to tests/heatmap_render_oracle.py.  The bar everywhere is 0 differing bytes: integer look-ups, one exact fp32
multiply and binary64 blends leave nothing to tolerate.  Outputs live inside guard bands (tests/guarded.py)."""
from pathlib import Path

import numpy as np
import pytest
import torch

import guarded
import heatmap_render_oracle as oracle
from stamp_amd import _lib, heatmaps
from stamp_amd.mil import VisionTransformer

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
THUMBS = ("56x40", "53x37", "17x91", "1x1")
OPACITIES = (0.6, 0.35)


@pytest.fixture(scope="module")
def z():
    with np.load(G / "heatmap_render.npz") as f:
        return {k: f[k] for k in f.files}


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _same(got: torch.Tensor, want: np.ndarray, what: str):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((got != want).sum())
    print(f"{what}: {bad} differing bytes of {want.size}")
    assert bad == 0, f"{what}: {bad} differing bytes of {want.size}"


class Bands:
    """u8 outputs inside guard bands; `check()` after the calls: nothing outside them is written."""

    def __init__(self, gpu):
        self.gpu, self.handles = gpu, []

    def out(self, *shape):
        v, h = guarded.guarded(shape, torch.uint8, self.gpu, pattern=0xA5, name=f"out{len(self.handles)}{shape}")
        self.handles.append(h)
        return v

    def check(self):
        torch.cuda.synchronize()
        for h in self.handles:
            h.assert_bands_intact()


@pytest.mark.parametrize("C", [2, 3])
def test_small_grid_score_images_and_overlays(gpu, z, C):
    """5 x 7 grid, 23 tiles (two on one cell, 13 empty cells), arguments planted at 0, 1, k / 256 and the float below, the last category without alpha;
    thumbnails at 8 x the grid, smaller, transposed-looking and 1 x 1; two opacities.  Against matplotlib + Pillow + `_create_overlay`."""
    cn = _dev(z["coords_norm"], gpu)
    cs, att = _dev(z[f"cs{C}"], gpu), _dev(z[f"att{C}"], gpu)
    b = Bands(gpu)
    rgba = heatmaps.colorize(cs / 2 + 0.5, att, "RdBu_r", coords_norm=cn, scale=8, out=b.out(C, 56, 40, 4))
    _same(rgba, z[f"rgba{C}"], f"score image C={C}")
    assert int(rgba[C - 1, ..., 3].max()) == 0
    unscaled = heatmaps.colorize(cs / 2 + 0.5, att, "RdBu_r", coords_norm=cn, scale=1, out=b.out(C, 7, 5, 4))
    _same(unscaled, oracle.raster(z[f"cs{C}"] / np.float32(2) + np.float32(0.5), z[f"att{C}"], heatmaps.colormap_table("RdBu_r"),
                                  cell=oracle.cell_table(z["coords_norm"]), scale=1), "unscaled score image")
    for t in THUMBS:
        thumb = _dev(z[f"thumb_{t}"], gpu)
        for o in OPACITIES:
            want = z[f"ov{C}_{t}_{o}"]
            _same(heatmaps.overlay(unscaled, thumb, o, out=b.out(*want.shape)), want, f"overlay C={C} {t} opacity {o}")
            _same(heatmaps.overlay(rgba, thumb, o, scale=8, out=b.out(*want.shape)), want, f"overlay of the x8 image C={C} {t} opacity {o}")
    one = heatmaps.overlay(unscaled[0], _dev(z["thumb_53x37"], gpu), 0.6)          # one image without the category axis
    _same(one, z[f"ov{C}_53x37_0.6"][0], "single-image overlay")
    b.check()


def test_lookup_edges(gpu, z):
    """The look-up rule on 24 random images with 0, 1, 0.5, 0.99999994 and 1e-8 planted, then -0, negatives, -inf, > 1, inf and NaN."""
    probe = _dev(z["probe"], gpu)
    ones = torch.ones_like(probe)
    for name in ("RdBu_r", "magma", "Reds"):
        want = z[f"probe_{name}"].copy()
        want[..., 3] = 255
        _same(heatmaps.colorize(probe, ones, name, scale=1), want, f"look-up {name}")
    edge = _dev(z["edge"], gpu)[None, None, :]
    want = z["edge_RdBu_r"].copy()[None, None]
    want[..., 3] = 0
    got = heatmaps.colorize(edge, torch.full_like(edge, float("nan")), "RdBu_r", scale=1)          # a NaN alpha source is not > 0
    _same(got, want, "edge values")
    assert got[0, 0, -1].tolist() == [0, 0, 0, 0]
    pastel = heatmaps.class_map(_dev(z["pastel_idx"], gpu)[None, :], torch.ones(1, 16, device=gpu), scale=1)
    _same(pastel, z["pastel_rgba"][None], "Pastel1 integer look-up")


def test_class_map(gpu, z):
    """12 classes: a tie on tile 2 (the lower class wins), top classes 8, 9 and 11 (9 and 11 take the last Pastel1 entry), three tiles without Grad-CAM
    mass.  Alpha is compared everywhere, RGB where alpha is 255; a cell without a tile is lut[0] with alpha 0 by this project's definition."""
    cn = _dev(z["coords_norm"], gpu)
    scores, cam = _dev(z["cm_scores"], gpu), _dev(z["cm_gradcam"], gpu)
    want = z["cm_rgba"]
    b = Bands(gpu)
    top = scores.argmax(1)
    assert int(top[2]) == 3 and {8, 9, 11} <= set(top.tolist())
    per_tile = heatmaps.class_map(top, cam.sum(-1), coords_norm=cn, scale=8, out=b.out(56, 40, 4))
    gridded = heatmaps.class_map(heatmaps.vals_to_im(scores, cn).argmax(-1), heatmaps.vals_to_im(cam, cn).sum(-1), scale=8, out=b.out(56, 40, 4))
    b.check()
    pastel = heatmaps.colormap_table("Pastel1")
    ref = oracle.classmap(oracle.top_class(z["cm_scores"]), z["cm_gradcam"].sum(-1), pastel, cell=oracle.cell_table(z["coords_norm"]), scale=8)
    for name, got in (("per tile", per_tile), ("gridded", gridded)):
        _same(got, ref, f"class map {name} vs oracle")
        got = got.cpu().numpy()
        on = want[..., 3] == 255
        assert (got[..., 3] == want[..., 3]).all() and on.any() and (got[on] == want[on]).all(), name
    empty = np.repeat(np.repeat(oracle.cell_table(z["coords_norm"]) < 0, 8, 0), 8, 1)
    assert (per_tile.cpu().numpy()[empty] == np.array([*pastel[0, :3], 0], np.uint8)).all()


def test_regression_and_survival_colourings(gpu, z):
    """`SlideHeatmap.render` for the single-output tasks: magma, Reds, and RdBu_r around a negative and a positive training median, with the overlay."""
    cn, cam, g2 = _dev(z["coords_norm"], gpu), _dev(z["reg_gradcam"], gpu), _dev(z["reg_g2d"], gpu)
    thumb = _dev(z["thumb_53x37"], gpu)
    cases = [("reg", "regression", None), ("surv", "survival", None)] + [(f"surv_{t}", "survival", float(m)) for t, m in zip(("neg", "pos"), z["surv_medians"])]
    assert z["surv_medians"][0] < 0 < z["surv_medians"][1]
    for key, task, med in cases:
        hm = heatmaps.SlideHeatmap(task, torch.zeros((), device=gpu), cn, cam, g2)
        im = hm.render(thumb, opacity=0.6, scale=8, train_pred_median=med)
        assert im.class_map is None
        _same(im.score_rgba, z[f"{key}_rgba"], f"{key} score image")
        _same(im.overlay, z[f"{key}_ov_53x37_0.6"], f"{key} overlay")
    assert heatmaps.SlideHeatmap("survival", torch.zeros((), device=gpu), cn, cam, g2).render().overlay is None
    with pytest.raises(ValueError):
        heatmaps.SlideHeatmap("regression", torch.zeros((), device=gpu), cn, cam, g2).render(train_pred_median=0.2)


def test_large_grid(gpu):
    """300 x 200 cells, 40 000 tiles, C = 4, thumbnail 2 395 x 1 597: ragged last workgroups in both directions, row strides past one sweep of the grid,
    a 3-byte output whose row width is no multiple of 4.  Against the oracle; outputs inside guard bands."""
    h, w, n, C, th, tw = 300, 200, 40_000, 4, 2395, 1597
    g = torch.Generator().manual_seed(5)
    cells = torch.randperm(h * w, generator=g)[:n]
    cells[-1] = h * w - 1
    cn = torch.stack([cells % w, cells // w], 1)
    arg = torch.rand(C, n, generator=g)
    arg[:, :512] = (torch.arange(512) // 2).float() / 256
    arg[:, 1:512:2] = torch.nextafter(arg[:, 1:512:2], torch.tensor(0.0))
    att = torch.rand(C, n, generator=g) - 0.3
    top = torch.randint(0, 12, (n,), generator=g)
    thumb = torch.randint(0, 256, (th, tw, 3), generator=g, dtype=torch.uint8)
    b = Bands(gpu)
    rgba = heatmaps.colorize(arg.to(gpu), att.to(gpu), "RdBu_r", coords_norm=cn.to(gpu), scale=8, out=b.out(C, 8 * h, 8 * w, 4))
    cmap = heatmaps.class_map(top.to(gpu), att[0].to(gpu), coords_norm=cn.to(gpu), scale=8, out=b.out(8 * h, 8 * w, 4))
    over = heatmaps.overlay(rgba, thumb.to(gpu), 0.6, scale=8, out=b.out(C, th, tw, 3))
    b.check()
    cell = oracle.cell_table(cn.numpy(), h, w)
    want = oracle.raster(arg.numpy(), att.numpy(), heatmaps.colormap_table("RdBu_r"), cell=cell, scale=8)
    _same(rgba, want, "large score images")
    _same(cmap, oracle.classmap(top.numpy(), att[0].numpy(), heatmaps.colormap_table("Pastel1"), cell=cell, scale=8), "large class map")
    _same(over, oracle.overlay(want, thumb.numpy(), 0.6, scale=8), "large overlay")
    assert 0.2 < float((want[..., 3] == 255).mean()) < 0.8          # blended and unblended pixels both occur in bulk


def _toy(tag, gpu, prefix="w:", dim_output=None):
    """the toy `vit` head of tests/test_gpu_heatmaps.py (tests/golden/heatmaps_plain.npz)"""
    f = np.load(G / f"heatmaps_{tag}.npz")
    C, F, D, L, H, FF = (int(v) for v in f["hparams"])
    model = VisionTransformer(dim_output=dim_output or C, dim_input=F, dim_model=D, n_layers=L, n_heads=H, dim_feedforward=FF, dropout=0.0, use_alibi=False).eval()
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(f[k]) for k in f.files if k.startswith(prefix)}, strict=True)
    return f, model.to(gpu)


def test_end_to_end_render(gpu):
    """`slide_heatmap(...).render(thumb)` on the toy head equals the oracle fed with the same SlideHeatmap's tensors, for the three tasks."""
    f, model = _toy("plain", gpu)
    feats, cu = torch.from_numpy(f["feats"]).to(gpu), torch.from_numpy(f["coords_um"]).to(gpu)
    thumb = torch.randint(0, 256, (61, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    hm = heatmaps.slide_heatmap(model, feats, cu, task="classification")
    im = hm.render(thumb.to(gpu), opacity=0.35)
    cell = oracle.cell_table(hm.coords_norm.cpu().numpy())
    H, W, C = hm.gradcam_2d.shape
    assert cell.shape == (H, W) and im.score_rgba.shape == (C, 8 * H, 8 * W, 4) and im.class_map.shape == (8 * H, 8 * W, 4) and im.overlay.shape == (C, 61, 70, 3)
    want = oracle.raster(hm.category_score.cpu().numpy() / np.float32(2) + np.float32(0.5), hm.attention.cpu().numpy(), heatmaps.colormap_table("RdBu_r"),
                         cell=cell, scale=8)
    _same(im.score_rgba, want, "end-to-end score images")
    _same(im.overlay, oracle.overlay(want, thumb.numpy(), 0.35, scale=8), "end-to-end overlay")
    _same(im.class_map, oracle.classmap(oracle.top_class(hm.scores_2d.cpu().numpy()), hm.gradcam_2d.cpu().numpy().sum(-1), heatmaps.colormap_table("Pastel1"),
                                        scale=8), "end-to-end class map")
    assert int(im.score_rgba[..., 3].max()) == 255 and int(im.class_map[..., 3].min()) == 0
    _, one = _toy("plain", gpu, prefix="single:", dim_output=1)
    for task, med, cmap in (("regression", None, "magma"), ("survival", None, "Reds"), ("survival", 0.25, "RdBu_r")):
        hs = heatmaps.slide_heatmap(one, feats, cu, task=task)
        assert hs.task == task and hs.gradcam_2d.shape == (H, W)
        ims = hs.render(thumb.to(gpu), train_pred_median=med, scale=3)
        g = hs.gradcam_2d.cpu().numpy()
        alpha = oracle._gather(hs.gradcam.cpu().numpy()[None], cell)
        x = g if med is None else oracle.survival_arg(g, med)
        want = oracle.raster(x[None], alpha, heatmaps.colormap_table(cmap), scale=3)
        _same(ims.score_rgba, want, f"end-to-end {task} median {med}")
        _same(ims.overlay, oracle.overlay(want, thumb.numpy(), 0.6, scale=3), f"end-to-end {task} median {med} overlay")
    top = heatmaps.ranked_tiles(hm.category_score[0], 5, 5)
    assert torch.equal(top[1], hm.category_score[0].sort(descending=True).values[:5]) and torch.equal(top[3], hm.category_score[0].sort().values[:5])


def test_bad_arguments_are_errors_not_faults(gpu):
    score = torch.zeros(1, 2, 2, 4, dtype=torch.uint8, device=gpu)
    thumb = torch.zeros(3, 3, 3, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        heatmaps.overlay(score, thumb, 1.5)
    with pytest.raises(ValueError):
        heatmaps.colorize(torch.rand(2, 3, device=gpu), torch.rand(2, 3, device=gpu), "viridis")
    with pytest.raises(ValueError):
        heatmaps.class_map(torch.rand(2, 3, device=gpu), torch.rand(2, 3, device=gpu))
    with pytest.raises(RuntimeError, match="outside"):          # a negative coordinate with the grid's shape given by the others
        heatmaps.colorize(torch.rand(3, device=gpu), torch.rand(3, device=gpu), "Reds", coords_norm=torch.tensor([[0, 0], [-1, 1], [2, 2]], device=gpu))
    tabs = torch.zeros(3, dtype=torch.int32, device=gpu)
    out = torch.empty(1, 3, 3, 3, dtype=torch.uint8, device=gpu)
    rc = _lib.lib().amds_heatmap_overlay(score.data_ptr(), thumb.data_ptr(), tabs.data_ptr(), tabs.data_ptr(), -0.1, out.data_ptr(), 1, 2, 2, 1, 3, 3, guarded.cur_stream())
    assert rc != 0
    # table entries outside the grid are clamped, never dereferenced
    wild = torch.tensor([-7, 1, 1 << 30], dtype=torch.int32, device=gpu)
    score[0, 1, 1] = torch.tensor([255, 255, 255, 255], dtype=torch.uint8)
    assert _lib.lib().amds_heatmap_overlay(score.data_ptr(), thumb.data_ptr(), wild.data_ptr(), wild.data_ptr(), 1.0, out.data_ptr(), 1, 2, 2, 1, 3, 3, guarded.cur_stream()) == 0
    assert out[0, :, :, 0].tolist() == [[0, 0, 0], [0, 255, 255], [0, 255, 255]]
