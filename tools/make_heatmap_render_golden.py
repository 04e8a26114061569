"""Writes tests/golden/heatmap_render.npz and stamp_amd/colormaps.json: what matplotlib, Pillow and the reference's own `_vals_to_im`, `_show_class_map`
and `_create_overlay` (src/stamp/heatmaps/__init__.py:142-156, 241-258, 261-284; lifted by name with tools/make_golden.py's `exec_defs`, the module
itself needs openslide) return for the small cases of tests/test_cpu_heatmap_render.py and tests/test_gpu_heatmap_render.py.  Data only: inputs and
expected bytes.  Needs the reference checkout, matplotlib and Pillow; the tests need none of them.

    python tools/make_heatmap_render_golden.py [--reference /path/to/reference/src/stamp]
"""
from __future__ import annotations

import argparse
import json
import sys
import types
from pathlib import Path
from typing import Collection, List, Tuple, cast

import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
import PIL  # noqa: E402
import torch  # noqa: E402
from matplotlib.patches import Patch  # noqa: E402
from PIL import Image  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
COLORMAPS = ("RdBu_r", "magma", "Reds", "Pastel1")
THUMBS = ((56, 40), (53, 37), (17, 91), (1, 1))
OPACITIES = (0.6, 0.35)
GW, GH, N = 5, 7, 23


def tables() -> dict:
    return {name: np.uint8(plt.get_cmap(name)(np.arange(plt.get_cmap(name).N)) * 255) for name in COLORMAPS}


def times8(im: np.ndarray) -> np.ndarray:
    """the reference's `Image.fromarray(np.uint8(im * 255)).resize(8 x, NEAREST)` (:445-448, 526-529, 607-609)"""
    target = np.array(im.shape[:2][::-1]) * 8
    return np.array(Image.fromarray(np.uint8(im * 255)).resize(tuple(target), resample=Image.Resampling.NEAREST))


def coords() -> torch.Tensor:
    """23 tiles on a 5 x 7 grid: 22 distinct cells (13 stay empty), tiles 3 and 17 on one cell, the far corner taken so the grid is 5 x 7."""
    g = torch.Generator().manual_seed(41)
    cells = torch.randperm(GW * GH - 1, generator=g)[:N - 2].tolist() + [GW * GH - 1]
    cells.insert(17, cells[3])
    xy = torch.tensor([[c % GW, c // GW] for c in cells], dtype=torch.long)
    assert xy.shape == (N, 2) and len(set(cells)) == N - 1 and tuple(xy.max(0).values.tolist()) == (GW - 1, GH - 1)
    return xy


def planted_scores(C: int, g: torch.Generator):
    """category_score [C, N] whose colour argument cs / 2 + 0.5 hits 0, 1, 0.5, k / 256 and the float just below it exactly; attention [C, N] with zeros and
    negatives, all <= 0 for the last category."""
    want = [0.0, 1.0, 0.5] + [k / 256 for k in (1, 64, 192, 255)] + [float(np.nextafter(np.float32(k / 256), np.float32(0))) for k in (128, 192, 255)]
    want = torch.tensor(want, dtype=torch.float32)
    cs = torch.rand(C, N, generator=g) * 2 - 1
    for c in range(C):
        at = torch.randperm(N, generator=g)[:len(want)]
        cs[c, at] = 2 * want - 1
        assert torch.equal(cs[c, at] / 2 + 0.5, want), "a planted colour argument does not survive cs / 2 + 0.5"
    att = torch.rand(C, N, generator=g)
    att[:, torch.randperm(N, generator=g)[:4]] = 0.0
    att[0, 5] = -0.25
    att[C - 1] = -att[C - 1]
    return cs, att


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="the reference's src/stamp directory (default: tools/make_golden.py's REF)")
    args = ap.parse_args()
    sys.path[:0] = [str(ROOT / "tools"), str(ROOT)]
    from make_golden import REF, exec_defs

    hm_path = Path(args.reference or REF) / "heatmaps" / "__init__.py"
    ref = exec_defs(hm_path, {"_vals_to_im", "_show_class_map", "_create_overlay"},
                    dict(torch=torch, Tensor=torch.Tensor, np=np, plt=plt, Image=Image, Patch=Patch, cast=cast, Collection=Collection, List=List, Tuple=Tuple,
                         Axes=object))
    vals_to_im, show_class_map, create_overlay = ref["_vals_to_im"], ref["_show_class_map"], ref["_create_overlay"]
    no_axes = types.SimpleNamespace(imshow=lambda *a, **k: None, legend=lambda *a, **k: None)

    luts = tables()
    rec = {"matplotlib_version": matplotlib.__version__, **{k: v.tobytes().hex() for k, v in luts.items()}}          # text: 8 hex digits per RGBA entry
    (ROOT / "stamp_amd" / "colormaps.json").write_text(json.dumps(rec, indent=1) + "\n")

    g = torch.Generator().manual_seed(40)
    cn = coords()
    arrs: dict = dict(coords_norm=cn.numpy(), matplotlib_version=np.array(matplotlib.__version__), pillow_version=np.array(PIL.__version__))
    thumbs = {f"{th}x{tw}": torch.randint(0, 256, (th, tw, 3), generator=g, dtype=torch.uint8).numpy() for th, tw in THUMBS}
    thumbs["56x40"][:2, :3] = [[[0, 0, 0], [255, 255, 255], [255, 0, 1]], [[1, 254, 128], [127, 127, 127], [2, 3, 5]]]
    arrs.update({"thumb_" + k: v for k, v in thumbs.items()})

    # ---- classification: :500-522 per category, the x8 resize :526-529, the overlay :536-538
    for C in (2, 3):
        cs, att = planted_scores(C, g)
        rgba, over = [], {k: [] for k in ((t, o) for t in thumbs for o in OPACITIES)}
        for c in range(C):
            score_im = plt.get_cmap("RdBu_r")(vals_to_im(cs[c].unsqueeze(-1) / 2 + 0.5, cn).squeeze(-1).numpy())
            score_im[..., -1] = (vals_to_im(att[c].unsqueeze(-1), cn).squeeze(-1) > 0).numpy()
            rgba.append(times8(score_im))
            for (t, o), dst in over.items():
                dst.append(create_overlay(thumb=thumbs[t], score_im=score_im, alpha=o))
        arrs.update({f"cs{C}": cs.numpy(), f"att{C}": att.numpy(), f"rgba{C}": np.stack(rgba)})
        arrs.update({f"ov{C}_{t}_{o}": np.stack(v) for (t, o), v in over.items()})

    # ---- class map: :437-448.  12 classes; tile 2 ties classes 3 and 5, tiles 4 / 6 / 8 have top classes 8 / 9 / 11; three tiles carry no Grad-CAM mass
    scores = torch.rand(N, 12, generator=g) * 0.5
    scores[2, 3] = scores[2, 5] = 0.75
    for t, k in ((4, 8), (6, 9), (8, 11), (17, 0)):
        scores[t, k] = 0.875
    cam = torch.rand(N, 12, generator=g)
    cam[[1, 8, 20]] = 0.0
    scores_2d, cam_2d = vals_to_im(scores, cn), vals_to_im(cam, cn)
    top_2d = scores_2d.topk(2).indices[:, :, 0]
    classes_img, _ = show_class_map(class_ax=no_axes, top_score_indices=top_2d, gradcam_2d=cam_2d, categories=[str(i) for i in range(12)])
    arrs.update(cm_scores=scores.numpy(), cm_gradcam=cam.numpy(), cm_top_2d=top_2d.numpy(), cm_rgba=times8(classes_img))

    # ---- regression :593-610 and survival :675-717: one Grad-CAM vector, four colourings
    cam1 = torch.rand(N, generator=g) + 0.05
    cam1[[0, 9]] = 0.0
    raw_2d = vals_to_im(cam1, cn)
    g2 = (raw_2d - raw_2d.min()) / (raw_2d.max() - raw_2d.min() + 1e-8)
    medians = (-0.3, 0.4)
    alpha_mask = (raw_2d > 0).numpy().astype(np.float32)
    arrs.update(reg_gradcam=cam1.numpy(), reg_g2d=g2.numpy(), surv_medians=np.array(medians))

    def coloured(key, cmap, x):
        score_im = plt.get_cmap(cmap)(x.numpy())
        score_im[..., -1] = alpha_mask
        arrs[f"{key}_rgba"] = times8(score_im)[None]
        arrs[f"{key}_ov_53x37_0.6"] = create_overlay(thumb=thumbs["53x37"], score_im=score_im, alpha=0.6)[None]

    coloured("reg", "magma", g2)
    coloured("surv", "Reds", g2)
    for tag, med in zip(("neg", "pos"), medians):
        arg = (g2 - med) / (2 * (g2 - med).abs().amax() + 1e-8) + 0.5
        arrs[f"surv_{tag}_arg"] = arg.numpy()
        coloured(f"surv_{tag}", "RdBu_r", arg)

    # ---- the look-up rule itself: 24 random images with the edge values planted
    probe = torch.rand(24, 9, 11, generator=g)
    probe[:, 0, :5] = torch.tensor([0.0, 1.0, 0.5, 0.99999994, 1e-8])
    arrs["probe"] = probe.numpy()
    for name in ("RdBu_r", "magma", "Reds"):
        arrs[f"probe_{name}"] = np.uint8(plt.get_cmap(name)(probe.numpy()) * 255)
    edge = np.array([-0.0, -1e-9, -0.5, -np.inf, 1.0000001, 2.0, np.inf, np.nan], np.float32)
    arrs["edge"] = edge
    arrs["edge_RdBu_r"] = np.uint8(plt.get_cmap("RdBu_r")(edge) * 255)
    arrs["pastel_idx"] = np.arange(-2, 14)
    arrs["pastel_rgba"] = np.uint8(plt.get_cmap("Pastel1")(np.arange(-2, 14)) * 255)

    out = ROOT / "tests" / "golden" / "heatmap_render.npz"
    np.savez_compressed(out, **arrs)
    print(f"wrote {out} ({out.stat().st_size} bytes, {len(arrs)} arrays) and stamp_amd/colormaps.json; matplotlib {matplotlib.__version__}, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
