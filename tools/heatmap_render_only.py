#!/usr/bin/env python3
"""Times `SlideHeatmap.render` (stamp_amd.heatmaps: score images at 8 px per tile for all categories, the class map, the overlays on a thumbnail; three
launches plus the cell table) on a classification slide of synthetic tensors at two sizes -- 300 x 200 cells / 40 000 tiles / C = 4 / thumbnail
2 400 x 1 600 and 60 x 40 / 1 600 tiles / C = 2 / 480 x 320 -- and the same images on the host: through tests/heatmap_render_oracle.py (numpy) and, where
they import, through matplotlib + Pillow the way the reference's `heatmaps_` makes them (one colour-map call, one x8 NEAREST resize and one float64 blend
per category).  Needs a GPU; writes profiles/heatmap_render_bench.txt.

GPU times: a host clock around the call and a device synchronise, median of three after one warm-up call; the copy of the finished images to the host is
timed separately.  The host paths are timed once.  No ratio is a requirement of anything; the file records what was measured."""
from __future__ import annotations

import argparse
import platform
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def synthetic_slide(h, w, n, C, seed):
    from stamp_amd import heatmaps
    g = torch.Generator().manual_seed(seed)
    cells = torch.randperm(h * w, generator=g)[:n]
    cells[-1] = h * w - 1
    cn = torch.stack([cells % w, cells // w], 1)
    cam = torch.softmax(torch.randn(n, C, generator=g), 0)
    scores = torch.softmax(torch.randn(n, C, generator=g), 1)
    return cn, cam, scores, heatmaps


def host_numpy(hm, thumb, opacity):
    import heatmap_render_oracle as oracle
    from stamp_amd import heatmaps
    cell = oracle.cell_table(hm["cn"])
    rgba = oracle.raster(hm["cs"] / np.float32(2) + np.float32(0.5), hm["att"], heatmaps.colormap_table("RdBu_r"), cell=cell, scale=8)
    cm = oracle.classmap(oracle.top_class(hm["scores"]), hm["cam"].sum(-1), heatmaps.colormap_table("Pastel1"), cell=cell, scale=8)
    return rgba, cm, oracle.overlay(rgba, thumb, opacity, scale=8)


def host_mpl_pillow(hm, thumb, opacity):
    import matplotlib
    from PIL import Image
    h, w = int(hm["cn"][:, 1].max()) + 1, int(hm["cn"][:, 0].max()) + 1
    flat = hm["cn"][:, 1] * w + hm["cn"][:, 0]

    def grid(v):
        im = np.zeros((h * w,) + v.shape[1:], v.dtype)
        im[flat] = v
        return im.reshape((h, w) + v.shape[1:])

    def times8(im):
        return np.array(Image.fromarray(np.uint8(im * 255)).resize((8 * w, 8 * h), resample=Image.Resampling.NEAREST))

    rgba, over = [], []
    th, tw = thumb.shape[:2]
    tf = thumb.astype(float) / 255.0
    for c in range(hm["cs"].shape[0]):
        im = matplotlib.colormaps["RdBu_r"](grid(hm["cs"][c] / np.float32(2) + np.float32(0.5)))
        im[..., -1] = grid(hm["att"][c]) > 0
        rgba.append(times8(im))
        s = np.array(Image.fromarray(np.uint8(im * 255)).resize((tw, th), resample=Image.Resampling.NEAREST)) / 255.0
        o = tf.copy()
        m = s[..., -1] > 0
        o[m] = opacity * s[m, :3] + (1 - opacity) * tf[m]
        over.append((o * 255).astype(np.uint8))
    cls = matplotlib.colormaps["Pastel1"](np.argmax(grid(hm["scores"]), -1))
    cls[..., -1] = grid(hm["cam"]).sum(-1) > 0
    return np.stack(rgba), times8(cls), np.stack(over)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "heatmap_render_bench.txt")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("heatmap_render_only: needs a GPU", file=sys.stderr)
        return 1
    try:
        import matplotlib
        import PIL
        libs = f"matplotlib {matplotlib.__version__}, Pillow {PIL.__version__}"
    except ImportError:
        libs = None
    dev = torch.device("cuda:0")
    lines = [f"SlideHeatmap.render (classification: score images x8 for all categories, class map, overlays at opacity 0.6) on {torch.cuda.get_device_name(0)} "
             f"({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}); host: {platform.processor() or platform.machine()}, "
             f"{torch.get_num_threads()} torch threads, numpy {np.__version__}",
             "GPU: host clock around render + synchronise, median of 3 after a warm-up (min .. max); 'to host': .cpu() of the three results, median of 3; "
             "host paths once: tests/heatmap_render_oracle.py (numpy), and " + (f"the reference's way ({libs})" if libs else "matplotlib + Pillow not installed: not measured"),
             f"{'grid':>9} {'tiles':>6} {'C':>2} {'thumbnail':>11} {'GPU ms':>8} {'min':>8} {'max':>8} {'to host ms':>10} {'numpy ms':>9} {'mpl+PIL ms':>10} {'equal':>6}"]
    for h, w, n, C, th, tw in ((300, 200, 40_000, 4, 2400, 1600), (60, 40, 1_600, 2, 480, 320)):
        cn, cam, scores, heatmaps = synthetic_slide(h, w, n, C, seed=h)
        thumb = torch.randint(0, 256, (th, tw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        cnd, camd, scd, thd = cn.to(dev), cam.to(dev), scores.to(dev), thumb.to(dev)
        support, attention, cat = heatmaps.category_maps(camd, scd)
        hm = heatmaps.SlideHeatmap("classification", scd.mean(0), cnd, camd, heatmaps.vals_to_im(camd, cnd), scd, heatmaps.vals_to_im(scd, cnd), support, attention, cat)
        times, copies = [], []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            im = hm.render(thd, opacity=0.6)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            got = [im.score_rgba.cpu().numpy(), im.class_map.cpu().numpy(), im.overlay.cpu().numpy()]
            t2 = time.perf_counter()
            times.append((t1 - t0) * 1e3)
            copies.append((t2 - t1) * 1e3)
        times, copies = times[1:], copies[1:]
        host = dict(cn=cn.numpy(), cs=cat.cpu().numpy(), att=attention.cpu().numpy(), scores=scores.numpy(), cam=cam.numpy())
        t0 = time.perf_counter()
        want = host_numpy(host, thumb.numpy(), 0.6)
        np_ms = (time.perf_counter() - t0) * 1e3
        equal = all(np.array_equal(g_, w_) for g_, w_ in zip(got, want))
        mpl_ms = ""
        if libs:
            t0 = time.perf_counter()
            ref = host_mpl_pillow(host, thumb.numpy(), 0.6)
            mpl_ms = f"{(time.perf_counter() - t0) * 1e3:10.1f}"
            on = ref[1][..., 3] == 255          # the class map's colour under alpha 0 is not defined by the reference
            equal = equal and np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[1][..., 3], ref[1][..., 3]) \
                and np.array_equal(got[1][on], ref[1][on])
        lines.append(f"{f'{h}x{w}':>9} {n:>6} {C:>2} {f'{th}x{tw}':>11} {statistics.median(times):8.3f} {min(times):8.3f} {max(times):8.3f} "
                     f"{statistics.median(copies):10.1f} {np_ms:9.1f} {mpl_ms:>10} {str(equal):>6}")
        print(lines[-1], flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text("\n".join(lines) + "\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
