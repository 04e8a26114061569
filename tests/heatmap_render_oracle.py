"""The heat-map rasters of include/amdstamp.h (amds_heatmap_raster, amds_heatmap_classmap, amds_heatmap_overlay) as plain numpy: matplotlib's colour-map
look-up, Pillow's NEAREST resize and the reference's `_create_overlay` (src/stamp/heatmaps/__init__.py:241-284, 500-529, 600-609, 683-717) restated
without either library.  tests/test_cpu_heatmap_render.py pins this file against what matplotlib, Pillow and the reference's own functions returned
(tests/golden/heatmap_render.npz, written by tools/make_heatmap_render_golden.py); tests/test_gpu_heatmap_render.py pins the library against this file."""
from __future__ import annotations

import numpy as np


def lut_float(x, lut) -> np.ndarray:
    """`np.uint8(cmap(x) * 255)` for a float array: lut u8 [N, 4] = uint8(cmap(arange(N)) * 255).  NaN -> (0, 0, 0, 0); x < 0 -> lut[0]; x * N >= N ->
    lut[N - 1]; else lut[int(x * N)], the product in fp32."""
    x = np.asarray(x, np.float32)
    n = lut.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        f = x * np.float32(n)
        idx = np.where(f >= n, n - 1, np.where(x < 0, 0, f)).astype(np.float64)
    nan = np.isnan(x)
    out = lut[np.where(nan, 0, idx).astype(np.int64)]
    out[nan] = 0
    return out


def lut_int(idx, lut) -> np.ndarray:
    """cmap(integer array): direct indexing, below 0 the first and from N on the last entry."""
    return lut[np.clip(np.asarray(idx, np.int64), 0, lut.shape[0] - 1)]


def cell_table(coords_norm, h=None, w=None) -> np.ndarray:
    """int64 [N, 2] (column 0 = x) -> int [h, w], the highest tile index that names the cell, -1 where no tile lies (`_vals_to_im`'s indexed assignment)."""
    xy = np.asarray(coords_norm, np.int64)
    w = int(xy[:, 0].max()) + 1 if w is None else w
    h = int(xy[:, 1].max()) + 1 if h is None else h
    cell = np.full((h, w), -1, np.int64)
    for t, (x, y) in enumerate(xy):
        cell[y, x] = t
    return cell


def _gather(vals, cell, fill=0):
    """per-tile [C, N] -> images [C, h, w], `fill` where no tile lies."""
    vals = np.asarray(vals)
    img = vals[:, np.maximum(cell, 0)]
    img[:, cell < 0] = fill
    return img


def _replicate(img, scale):
    return np.repeat(np.repeat(img, scale, axis=-3), scale, axis=-2)


def raster(arg, alpha_src, lut, *, cell=None, scale=8) -> np.ndarray:
    """arg, alpha_src: fp32 per tile [C, N] with `cell`, else images [C, h, w] -> u8 [C, h * scale, w * scale, 4]."""
    arg, alpha_src = np.asarray(arg, np.float32), np.asarray(alpha_src, np.float32)
    if cell is not None:
        arg, alpha_src = _gather(arg, cell), _gather(alpha_src, cell)
    im = lut_float(arg, lut)
    with np.errstate(invalid="ignore"):
        im[..., 3] = np.where(alpha_src > 0, 255, 0)
    return _replicate(im, scale)


def classmap(top, alpha_src, lut, *, cell=None, scale=8) -> np.ndarray:
    """top: integer class per tile [N] with `cell`, else an image [h, w]; alpha_src fp32 alike -> u8 [h * scale, w * scale, 4]; a cell without a tile is
    lut[0] with alpha 0."""
    top, alpha_src = np.asarray(top, np.int64)[None], np.asarray(alpha_src, np.float32)[None]
    if cell is not None:
        top, alpha_src = _gather(top, cell), _gather(alpha_src, cell)
    im = lut_int(top[0], lut).copy()
    with np.errstate(invalid="ignore"):
        im[..., 3] = np.where(alpha_src[0] > 0, 255, 0)
    return _replicate(im, scale)


def resize_table(n_in: int, n_out: int) -> np.ndarray:
    """Pillow's NEAREST source indices: the running sum in double, in order."""
    a = n_in / n_out
    xo = 0.5 * a
    tab = np.empty(n_out, np.int64)
    for i in range(n_out):
        tab[i] = int(xo)
        xo += a
    return np.minimum(tab, n_in - 1)


def overlay(score, thumb, alpha: float, *, scale=1) -> np.ndarray:
    """score u8 [C, h * scale, w * scale, 4], thumb u8 [th, tw, 3] -> u8 [C, th, tw, 3]: `_create_overlay` per category.  A pixel's byte depends on the
    sampled score byte, the thumbnail byte and whether the sampled alpha byte is > 0 only, so the binary64 arithmetic (s = byte / 255.0, t = thumb / 255.0,
    alpha * s + (1 - alpha) * t or t, times 255, truncated) is done once per pair of bytes and looked up: the same operations on the same values."""
    score, thumb = np.asarray(score, np.uint8), np.asarray(thumb, np.uint8)
    h, w = score.shape[1] // scale, score.shape[2] // scale
    th, tw = thumb.shape[:2]
    ys, xs = resize_table(h, th) * scale, resize_table(w, tw) * scale
    unit = np.arange(256).astype(np.float64) / 255.0
    blended = ((alpha * unit[:, None] + (1 - alpha) * unit[None, :]) * 255).astype(np.uint8)          # [score byte][thumbnail byte]
    plain = (unit * 255).astype(np.uint8)
    s = score[:, ys][:, :, xs]
    t = np.broadcast_to(thumb, s[..., :3].shape)
    return np.where(s[..., 3:] > 0, blended[s[..., :3], t], plain[t])


def survival_arg(g, median) -> np.ndarray:
    """:683-694 in fp32: (g - med) / (2 * max|g - med| + 1e-8) + 0.5."""
    g = np.asarray(g, np.float32)
    d = g - np.float32(median)
    return (d / (np.float32(2) * np.abs(d).max() + np.float32(1e-8)) + np.float32(0.5)).astype(np.float32)


def top_class(scores) -> np.ndarray:
    """[..., C] -> the top class, ties to the lower index."""
    return np.argmax(np.asarray(scores), axis=-1)
