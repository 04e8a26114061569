"""Whole-slide heat-map scores on the HIP path: the arithmetic of the reference's `stamp heatmaps` for ONE slide, everything on the device.

Reference: src/stamp/heatmaps/__init__.py -- `_gradcam_per_category` :36-56, `_gradcam_single` :115-139, `_vals_to_im` :142-156, the grid coordinates
:376 with `get_stride` (src/stamp/modeling/data.py:1150-1161), the slide score :392-403, the one-tile-bag scores :417-427, the per-category support /
attention / score maps :464-498 and the regression branch's normalisations :593-597.

Rendering: the bytes of the reference's `raw/` images -- the per-category RGBA score image (:500-529, 600-609, 683-717), the class map (:241-258, 437-448)
and the blend over the slide thumbnail (`_create_overlay` :261-284) -- are `colorize`, `class_map`, `overlay` and `SlideHeatmap.render`: matplotlib's
colour-map look-up and Pillow's NEAREST resize restated as three kernels (csrc/heatmap_render.hip), byte for byte; the four colour tables are data
(stamp_amd/colormaps.json).  `ranked_tiles` is the selection of `_export_ranked_tiles` (:190-238).  Not here: matplotlib figures (the `plots/` folder, titles,
legends), PNG / JPEG encoding and file names, reading the slide or its thumbnail (the caller passes the thumbnail crop).

Two routes to the Grad-CAM scores:
  * fused (`stamp_amd.mil.VisionTransformer`, with or without ALiBi): one eval-mode training forward that keeps its activations
    (`mil_core.forward_train`), then ONE library call for all classes (`mil_core.gradcam` -> amds_mil_vit_gradcam) that never forms the
    [classes, tiles, features] Jacobian, then amds_softmax_over_tiles.  Operand type as the module's autograd path: bf16 at
    float32_matmul_precision "medium", else fp16 with the 2^10 scale on the basis vectors; non-finite fp16 logits or scores -> the same slide again on
    bf16 operands and `model.fp16_overflow_events += 1`.
  * jacrev (any module with the reference's ``forward(bags, coords=, mask=)``: TransMIL, a torch model; can be forced for the `vit` head): the
    reference's own three lines on the device.
  * library (`method="library"`, "the head's one-library-call Grad-CAM"): for the `vit` head the fused route above; for `stamp_amd.mil.TransMIL` one
    eval-mode training forward (`transmil_core.forward_train`), ONE library call for all classes (`transmil_core.gradcam` -> amds_transmil_gradcam: per class
    the backward's launches without parameter gradients down to `_fc1`, then a row-dot against the saved `_fc1` output) and amds_softmax_over_tiles.  fp32
    throughout, operand precision from `torch.get_float32_matmul_precision()` like the module: no fp16, so no overflow re-run.  "auto" does not pick it.
  * library, closed form (`stamp_amd.abmil.GatedAttentionMIL`; "auto" and "library" both pick it): ONE library call (`abmil.heatmap_scores` ->
    amds_abmil_heatmap) returns the eval forward's logits, scores and softmax weights, the Grad-CAM scores of ALL classes and every tile's logits as a bag
    of its own.  The head's Grad-CAM has a closed form whose one product does not depend on the class (include/amdstamp.h): no class loop, no gradient
    w.r.t. the features, no Jacobian.  `slide_heatmap` makes that one call per slide and also reports the softmax weights (`SlideHeatmap.tile_attention`).
    The head takes no mask and has no vmap rule, so "jacrev" does not work for it; "fused" is refused.
The module is put in eval mode for the duration of a call; ALiBi running means are not updated; no parameter receives a `.grad` and `feats` needs no
`requires_grad`.  There is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass

import torch

from . import _lib, mil_core, ops, transmil_core
from .abmil import GatedAttentionMIL
from .mil import TransMIL, VisionTransformer, _all_finite

_FP16_SCALE = 1024.0            # the power of two the fp16 basis vectors carry (as `_MilVitFunction`'s loss scale)
MAX_BAGS_PER_CALL = 32768       # one-tile bags per inference call of `tile_scores` (the attention kernels' grids take at most 65535 bags)


@contextlib.contextmanager
def _eval_mode(model: torch.nn.Module):
    was = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was)


def _check_inputs(feats: torch.Tensor, coords: torch.Tensor | None) -> None:
    if not feats.is_cuda or (coords is not None and not coords.is_cuda):
        raise RuntimeError("HIP MIL head needs bags on the GPU (no CPU fallback)")
    if feats.dim() != 2:
        raise ValueError(f"feats must be [tiles, features], got {tuple(feats.shape)}")
    if coords is not None and tuple(coords.shape) != (feats.shape[0], 2):
        raise ValueError(f"coords must be [{feats.shape[0]}, 2], got {tuple(coords.shape)}")


def _pick(model, method: str) -> str:
    if method not in ("auto", "fused", "jacrev", "library"):
        raise ValueError(f"method must be 'auto', 'fused', 'jacrev' or 'library', got {method!r}")
    fused_ok = isinstance(model, VisionTransformer)
    if isinstance(model, GatedAttentionMIL) and method in ("auto", "library"):          # its closed form: one library call, the route "auto" takes too
        return "library"
    if method == "library":          # the head's one-library-call Grad-CAM
        if fused_ok:
            return "fused"
        if isinstance(model, TransMIL):
            return "library"
        raise ValueError(f"method='library' needs a stamp_amd.mil.VisionTransformer, stamp_amd.mil.TransMIL or stamp_amd.abmil.GatedAttentionMIL, "
                         f"got {type(model).__name__}")
    if method == "fused" and not fused_ok:
        raise ValueError(f"method='fused' needs a stamp_amd.mil.VisionTransformer, got {type(model).__name__}")
    return ("fused" if fused_ok else "jacrev") if method == "auto" else method


def _cam_raw_fused(model: VisionTransformer, feats: torch.Tensor, coords: torch.Tensor | None) -> torch.Tensor:
    """-> cam_raw [C, N] (module docstring, the fused route)."""
    dev = feats.device
    tensors = dict(model.named_parameters())
    tensors.update(dict(model.named_buffers()))
    get = lambda n: tensors[n].detach().to(dev, torch.float32)  # noqa: E731
    bags = feats.detach().unsqueeze(0)
    cc = None if coords is None else coords.detach().unsqueeze(0)

    def forward(dt):
        pk = mil_core.PackedVit(model.dims, get, dt, True)
        logits, saved = mil_core.forward_train(pk, bags, cc, training=False)
        return pk, logits, saved

    if torch.get_float32_matmul_precision() != "medium":
        pk, logits, saved = forward(torch.float16)
        if _all_finite(logits):                 # (checked before the class loop is spent on an overflowed forward)
            cam = mil_core.gradcam(pk, saved, scale=_FP16_SCALE)
            if _all_finite(cam):
                return cam
        model.fp16_overflow_events += 1         # an fp16 activation or gradient overflowed: the same slide on bf16 operands (fp32's range)
    pk, _, saved = forward(torch.bfloat16)
    return mil_core.gradcam(pk, saved, scale=1.0)


def _cam_raw_transmil(model: TransMIL, feats: torch.Tensor) -> torch.Tensor:
    """-> cam_raw [C, N] (module docstring, the library route of the TransMIL head; coords are ignored like in its forward)."""
    F = model._fc1[0].in_features
    if feats.shape[1] != F:
        raise ValueError(f"feats must be [tiles, {F}], got {tuple(feats.shape)}")
    if feats.shape[0] < 1:
        raise ValueError("empty bag")
    _, saved = transmil_core.forward_train(model._get(feats.device), feats.detach().unsqueeze(0), (F, model.dim_hidden, model.n_classes), training=False)
    return transmil_core.gradcam(saved)


def _abmil_scores(model: GatedAttentionMIL, feats: torch.Tensor, *, want_cam: bool, want_tiles: bool) -> dict:
    """ONE amds_abmil_heatmap call on one slide (module docstring, the closed-form route; coords are ignored like in the head's forward)."""
    if feats.shape[1] != model.dims[0]:
        raise ValueError(f"feats must be [tiles, {model.dims[0]}], got {tuple(feats.shape)}")
    if feats.shape[0] < 1:
        raise ValueError("empty bag")
    with torch.no_grad():
        return model.heatmap_scores(feats.detach(), want_cam=want_cam, want_tiles=want_tiles)


def _cam_raw_library(model: torch.nn.Module, feats: torch.Tensor) -> torch.Tensor:
    """-> cam_raw [C, N] of the "library" route: TransMIL or the gated-attention head."""
    if isinstance(model, GatedAttentionMIL):
        return _abmil_scores(model, feats, want_cam=True, want_tiles=False)["cam_raw"]
    return _cam_raw_transmil(model, feats)


def _cam_raw_jacrev(model: torch.nn.Module, feats: torch.Tensor, coords: torch.Tensor | None, squeeze_all: bool) -> torch.Tensor:
    """The reference's lines :43-54 (`squeeze_all`: :126-137) -> cam before the softmax, [C, N] (or [N])."""
    from torch.func import jacrev

    feats = feats.detach().float()
    cu = None if coords is None else coords.detach().unsqueeze(0)

    def f(bags):
        out = model.forward(bags.unsqueeze(0), coords=cu, mask=None)
        return out.squeeze() if squeeze_all else out.squeeze(0)

    with torch.enable_grad():
        jac = jacrev(f)(feats)
    return (feats * jac).mean(-1).abs()


def _softmax_over_tiles(cam_raw: torch.Tensor) -> torch.Tensor:
    """fp32 [C, N] -> softmax over the tiles, transposed: [N, C] (amds_softmax_over_tiles; reference :55-56)."""
    ops._dev(cam_raw)
    cam_raw = cam_raw.contiguous().float()
    Cn, N = cam_raw.shape
    out = torch.empty(N, Cn, dtype=torch.float32, device=cam_raw.device)
    _lib.check(_lib.lib().amds_softmax_over_tiles(cam_raw.data_ptr(), out.data_ptr(), Cn, N, ops._stream()), "softmax_over_tiles")
    return out


def gradcam(model: torch.nn.Module, feats: torch.Tensor, coords: torch.Tensor | None = None, *, raw: bool = False, method: str = "auto") -> torch.Tensor:
    """reference `_gradcam_per_category` (:36-56): feats [N, F] fp16 / fp32, coords [N, 2] (micrometres; required by an ALiBi head) -> [N, C] fp32, the
    per-class Grad-CAM scores soft-maxed over the tiles; `raw=True`: the scores before that softmax (line 54), [N, C].  `method`: "auto" (fused for the
    HIP `vit` head, the closed-form library call for `abmil.GatedAttentionMIL`, else jacrev), "fused", "jacrev", "library" (the head's one-library-call
    Grad-CAM: `vit` as "fused", TransMIL through amds_transmil_gradcam, the gated-attention head through amds_abmil_heatmap)."""
    _check_inputs(feats, coords)
    route = _pick(model, method)
    with _eval_mode(model):
        if route in ("fused", "library"):
            cam_raw = _cam_raw_fused(model, feats, coords) if route == "fused" else _cam_raw_library(model, feats)
            return cam_raw.t().contiguous() if raw else _softmax_over_tiles(cam_raw)
        cam_raw = _cam_raw_jacrev(model, feats, coords, squeeze_all=False)
        if cam_raw.dim() != 2:
            raise ValueError(f"the model must return [1, classes] logits for one bag, its Jacobian reduced to {tuple(cam_raw.shape)}")
        return (cam_raw if raw else torch.softmax(cam_raw, dim=-1)).permute(-1, -2)


def gradcam_single(model: torch.nn.Module, feats: torch.Tensor, coords: torch.Tensor | None = None, *, method: str = "auto") -> torch.Tensor:
    """reference `_gradcam_single` (:115-139), regression / survival models (dim_output == 1): -> [N] fp32, |mean_f feats * d output / d feats|."""
    _check_inputs(feats, coords)
    route = _pick(model, method)
    n_out = getattr(model, "dim_output", getattr(model, "n_classes", None))
    if n_out is not None and n_out != 1:
        raise ValueError(f"gradcam_single is for single-output models (dim_output == 1), this one has {n_out} outputs: use gradcam")
    with _eval_mode(model):
        if route == "fused":
            return _cam_raw_fused(model, feats, coords)[0]
        if route == "library":
            return _cam_raw_library(model, feats)[0]
        cam = _cam_raw_jacrev(model, feats, coords, squeeze_all=True)
        if cam.dim() != 1:
            raise ValueError(f"gradcam_single is for single-output models, the Jacobian reduced to {tuple(cam.shape)}")
        return cam


def _largest_fitting(need_bytes, budget: int, limit: int) -> int:
    """The largest bag count in [1, limit] with need_bytes(bags) <= budget (need_bytes grows with the bag count: bisection); 1 if not even one bag fits --
    the call itself then reports what it needs."""
    if need_bytes(limit) <= budget:
        return limit
    lo, hi = 1, limit - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if need_bytes(mid) <= budget:
            lo = mid
        else:
            hi = mid - 1
    return lo


def default_tiles_per_call(model: torch.nn.Module, device=None) -> int:
    """The default chunk of `tile_scores`.  `mil.TransMIL`: the largest bag count <= transmil_core.MAX_BAGS_PER_CALL (bags x 8 heads is one launch's batch
    dimension) whose amds_transmil_workspace_bytes(cfg, bags, 1) fits in half of the free device memory -- a one-tile bag is padded to dim_hidden / 2 token
    rows and carries 8 heads of attention matrices.  Any other module: MAX_BAGS_PER_CALL."""
    if not isinstance(model, TransMIL):
        return MAX_BAGS_PER_CALL
    import ctypes as C
    cfg = _lib.TransMilCfg(model._fc1[0].in_features, model.dim_hidden, model.n_classes)
    query = _lib.lib().amds_transmil_workspace_bytes
    return _largest_fitting(lambda bags: query(C.byref(cfg), bags, 1), torch.cuda.mem_get_info(device)[0] // 2, transmil_core.MAX_BAGS_PER_CALL)


def tile_scores(model: torch.nn.Module, feats: torch.Tensor, coords: torch.Tensor | None = None, *, tiles_per_call: int | None = None) -> torch.Tensor:
    """reference :417-427: every tile as a bag of its own under an all-False mask, softmax over the classes -> [N, C] fp32.  The module's masked inference
    forward in chunks of `tiles_per_call` bags (default: `default_tiles_per_call`); one chunk equals
    ``torch.softmax(model(feats.unsqueeze(-2), coords=coords.unsqueeze(-2), mask=zeros), 1)`` bit for bit.

    `mil.TransMIL`: the bags of one call are NOT independent -- each pseudo-inverse starts from maxima over all bags of the call (trans_mil.py:26-28) --, so
    the chunks whose rows equal the module's own call are fixed: consecutive groups of transmil_core.MAX_BAGS_PER_CALL (8191) tiles, the most one
    forward takes.  `tiles_per_call` (default: what half of the free memory allows; above 8191 raises) only bounds the bags of one LIBRARY call: a group that
    needs several runs staged (`transmil_core.forward_infer_grouped`: three passes, the maxima on the device, sub-call sizes that repeat the one call's
    kernel choices) with the bits of the one call, so the result depends neither on `tiles_per_call` nor on the free memory.  This CHANGES what an explicit
    `tiles_per_call` below the slide size returned for a TransMIL before: independent chunks then, each with its own maxima (3e-4 apart in the
    probabilities); the group's bits now.  Every other call returns the bits it returned.

    `abmil.GatedAttentionMIL` (its forward takes no mask): the classifier over the rows of h (amds_abmil_heatmap's tile_logits, the bits of the head's
    forward on every one-row bag), `tiles_per_call` ROWS per library call; a row's bits do not depend on the chunk."""
    _check_inputs(feats, coords)
    N = feats.shape[0]
    step = default_tiles_per_call(model, feats.device) if tiles_per_call is None else int(tiles_per_call)
    if step < 1:
        raise ValueError("tiles_per_call must be >= 1")
    if isinstance(model, GatedAttentionMIL):
        with _eval_mode(model):
            outs = [torch.softmax(_abmil_scores(model, feats[a:a + step], want_cam=False, want_tiles=True)["tile_logits"], dim=1) for a in range(0, N, step)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
    group = step
    if isinstance(model, TransMIL):
        group = transmil_core.MAX_BAGS_PER_CALL
        if step > group:
            raise ValueError(f"tiles_per_call={step} exceeds the TransMIL forward's limit of {group} bags per call")
    outs = []
    with _eval_mode(model), torch.no_grad():
        for a in range(0, N, group):
            e = min(N, a + group)
            if e - a > step:          # (TransMIL alone: group == step for every other module)
                dims = (model._fc1[0].in_features, model.dim_hidden, model.n_classes)
                logits = transmil_core.forward_infer_grouped(model._c_weights(feats.device), dims, feats[a:e].unsqueeze(-2), step)
            else:
                logits = model(feats[a:e].unsqueeze(-2), coords=None if coords is None else coords[a:e].unsqueeze(-2),
                               mask=torch.zeros(e - a, 1, dtype=torch.bool, device=feats.device))
            outs.append(torch.softmax(logits, dim=1))
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def grid_coords(coords_um: torch.Tensor, stride_um: float | None = None) -> torch.Tensor:
    """reference :376: tile coordinates in micrometres [N, 2] -> int64 grid coordinates (the top-left tile of the grid is a multiple of the stride from
    (0, 0)); `stride_um` None: `get_stride` (modeling/data.py:1150-1161), the smallest step between two distinct x or two distinct y values."""
    if coords_um.dim() != 2 or coords_um.shape[1] != 2:
        raise ValueError(f"coords must be [tiles, 2], got {tuple(coords_um.shape)}")
    coords_um = coords_um.float()
    if stride_um is None:
        steps = []
        for axis in (0, 1):
            v = coords_um[:, axis].unique(sorted=True)
            if v.numel() < 2:
                raise ValueError("get_stride needs at least two distinct x and two distinct y coordinates; pass stride_um")
            steps.append((v[1:] - v[:-1]).min())
        stride_um = float(torch.stack(steps).min().item())
    return (coords_um / stride_um).round().long()


def vals_to_im(vals: torch.Tensor, coords_norm: torch.Tensor) -> torch.Tensor:
    """reference `_vals_to_im` (:142-156): vals [N, ...], int64 grid coordinates [N, 2] (column 0 = x) -> [H, W, ...] with H = max y + 1, W = max x + 1,
    zeros where no tile lies (amds_scatter_grid).  Where several tiles share a cell the highest tile index wins.  A negative coordinate raises."""
    ops._dev(vals, coords_norm)
    if coords_norm.dim() != 2 or coords_norm.shape[1] != 2 or coords_norm.shape[0] != vals.shape[0] or vals.shape[0] < 1:
        raise ValueError(f"coords_norm must be [{vals.shape[0]}, 2] with at least one tile, got {tuple(coords_norm.shape)}")
    xy = coords_norm.to(torch.int64).contiguous()
    w, h = (int(v) + 1 for v in xy.max(0).values.tolist())          # the one host read: the image's shape
    if h < 1 or w < 1:
        raise ValueError("negative grid coordinates")
    N = vals.shape[0]
    v32 = vals.detach().reshape(N, -1).float().contiguous()
    k = v32.shape[1]
    out = torch.empty(h, w, k, dtype=torch.float32, device=vals.device)
    cells = torch.empty(h * w + 1, dtype=torch.int32, device=vals.device)
    _lib.check(_lib.lib().amds_scatter_grid(v32.data_ptr(), xy.data_ptr(), out.data_ptr(), cells.data_ptr(), N, k, h, w, ops._stream()), "scatter_grid")
    return out.reshape(h, w, *vals.shape[1:]).to(vals.dtype)


def _top2(x: torch.Tensor):
    """(index of the largest, largest, second largest) along dim 1; ties go to the LOWER class index (torch.argmax returns the first maximum)."""
    i1 = x.argmax(dim=1, keepdim=True)
    v1 = x.gather(1, i1)
    v2 = x.scatter(1, i1, float("-inf")).max(dim=1).values
    return i1.squeeze(1), v1.squeeze(1), v2


def category_maps(gradcam: torch.Tensor, scores: torch.Tensor):
    """reference :464-498 for every category at once: gradcam [N, C] (soft-maxed over the tiles), scores [N, C] -> (support, attention, category_score),
    each [C, N].  support: a class's score minus its nearest competitor's; attention: the class's Grad-CAM score where it is the top class, else the
    strongest other class's, each normalised by its maximum; category_score = support * attention / max(attention).  Where two classes tie for a tile's
    top score the lower class index counts as the top one."""
    if gradcam.shape != scores.shape or scores.dim() != 2 or scores.shape[1] < 2:
        raise ValueError(f"gradcam and scores must both be [tiles, classes >= 2], got {tuple(gradcam.shape)} and {tuple(scores.shape)}")
    Cn = scores.shape[1]
    top, s1, s2 = _top2(scores)
    gtop, g1, g2 = _top2(gradcam)
    cls = torch.arange(Cn, device=scores.device)[:, None]           # [C, 1]
    is_top = top[None, :] == cls                                    # [C, N]
    support = torch.where(is_top, scores.t() - s2[None, :], scores.t() - s1[None, :])
    others = torch.where(gtop[None, :] == cls, g2[None, :], g1[None, :])         # max over the other classes
    attention = torch.where(is_top, gradcam.t() / gradcam.max(), others / others.max(dim=1, keepdim=True).values)
    score = support * attention / attention.max(dim=1, keepdim=True).values
    return support, attention, score


@dataclass
class SlideHeatmap:
    """What the reference's `heatmaps_` computes for one slide before it starts drawing."""
    task: str
    slide_score: torch.Tensor                   # classification: softmax over the classes [C] (:403); regression: the output, 0-dim (:587)
    coords_norm: torch.Tensor                   # int64 [N, 2]
    gradcam: torch.Tensor                       # [N, C] (:407-411) or [N] (:590-592)
    gradcam_2d: torch.Tensor                    # [H, W, C] (:412-415); regression: [H, W] min / max normalised (:594-597)
    scores: torch.Tensor | None = None          # [N, C] (:417-427)
    scores_2d: torch.Tensor | None = None       # [H, W, C] (:428-430)
    support: torch.Tensor | None = None         # [C, N] (:471-475)
    attention: torch.Tensor | None = None       # [C, N] (:483-494)
    category_score: torch.Tensor | None = None  # [C, N] (:496-498)
    tile_relevance: torch.Tensor | None = None  # regression: gradcam / max [N] (:593)
    tile_attention: torch.Tensor | None = None  # `abmil.GatedAttentionMIL` alone: the softmax weights over the tiles [N] (chief.py:77-79); None for the other heads


    def render(self, thumb: torch.Tensor | None = None, *, opacity: float = 0.6, scale: int = 8, train_pred_median: float | None = None) -> "HeatmapImages":
        """The images of the reference's `raw/` folder for this slide, on the device (module docstring, "Rendering"): the per-category RGBA score image at
        `scale` pixels per tile, the class map (classification) and, with `thumb` u8 [th, tw, 3] (the caller's thumbnail crop, :159-187), the score image
        blended over it at `opacity`.  classification: RdBu_r of category_score / 2 + 0.5, alpha where attention > 0 (:500-522).  regression: magma of
        gradcam_2d, alpha where the scattered gradcam > 0 (:600-604).  survival: Reds likewise (:705-711), or with `train_pred_median` RdBu_r of
        (g - med) / (2 * max|g - med| + 1e-8) + 0.5 over g = gradcam_2d, empty cells included (:683-697).  One launch per kind of output."""
        if train_pred_median is not None and self.task != "survival":
            raise ValueError("train_pred_median belongs to task 'survival'")
        classes = None
        if self.task == "classification":
            score = colorize(self.category_score / 2 + 0.5, self.attention, "RdBu_r", coords_norm=self.coords_norm, scale=scale)
            classes = class_map(self.scores_2d.argmax(-1), self.gradcam_2d.sum(-1), scale=scale)          # :437-442; alpha :250
        else:
            g, cmap = self.gradcam_2d, ("magma" if self.task == "regression" else "Reds")
            if train_pred_median is not None:
                d = g - float(train_pred_median)
                g, cmap = d / (2 * d.abs().amax() + 1e-8) + 0.5, "RdBu_r"
            score = colorize(g[None], vals_to_im(self.gradcam, self.coords_norm)[None], cmap, scale=scale)
        over = None if thumb is None else overlay(score, thumb, opacity, scale=scale)
        return HeatmapImages(score, classes, over)


@dataclass
class HeatmapImages:
    """`SlideHeatmap.render`: u8 device tensors, the bytes the reference writes into `raw/` before PNG encoding."""
    score_rgba: torch.Tensor                    # [C, scale * H, scale * W, 4] (:526-533, 606-610, 713-717); regression / survival: C = 1
    class_map: torch.Tensor | None = None       # [scale * H, scale * W, 4], classification only (:444-448)
    overlay: torch.Tensor | None = None         # [C, th, tw, 3] when a thumbnail was given (:535-541, 620-624, 727-731)


# ---- Rendering: look-up tables, rasters, overlays -------------------------------------------------------------------------------------------------
COLORMAPS = ("RdBu_r", "magma", "Reds", "Pastel1")
_TABLES: dict = {}


def colormap_table(name: str):
    """The u8 [N, 4] table uint8(cmap(arange(N)) * 255) of one of COLORMAPS, from stamp_amd/colormaps.json (text: per map the N RGBA entries as one
    hexadecimal string, 8 digits per entry; recorded from matplotlib, whose version the file's `matplotlib_version` names;
    tools/make_heatmap_render_golden.py writes it): matplotlib itself is not needed at run time."""
    if name not in COLORMAPS:
        raise ValueError(f"colour map must be one of {COLORMAPS}, got {name!r}")
    if "host" not in _TABLES:
        import json
        import numpy as np
        from pathlib import Path
        rec = json.loads(Path(__file__).with_name("colormaps.json").read_text())
        _TABLES["host"] = {k: np.frombuffer(bytes.fromhex(rec[k]), np.uint8).reshape(-1, 4) for k in COLORMAPS}
    return _TABLES["host"][name]


def _lut(name: str, device: torch.device) -> torch.Tensor:
    key = (name, str(device))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(colormap_table(name).copy()).to(device).contiguous()
    return _TABLES[key]


def _cells(coords_norm: torch.Tensor, n: int):
    """int64 grid coordinates [n, 2] -> (cell table int32 [h * w + 1] (amds_scatter_cells), h, w)."""
    if coords_norm.dim() != 2 or coords_norm.shape[1] != 2 or coords_norm.shape[0] != n or n < 1:
        raise ValueError(f"coords_norm must be [{n}, 2] with at least one tile, got {tuple(coords_norm.shape)}")
    xy = coords_norm.to(torch.int64).contiguous()
    w, h = (int(v) + 1 for v in xy.max(0).values.tolist())
    if h < 1 or w < 1:
        raise ValueError("negative grid coordinates")
    cells = torch.empty(h * w + 1, dtype=torch.int32, device=xy.device)
    _lib.check(_lib.lib().amds_scatter_cells(xy.data_ptr(), cells.data_ptr(), n, h, w, ops._stream()), "scatter_cells")
    return cells, h, w


def _out(out: torch.Tensor | None, shape, device) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {tuple(shape)} on {device}")
    return out


def _sources(vals: torch.Tensor, alpha_src: torch.Tensor, coords_norm: torch.Tensor | None, dtype: torch.dtype):
    """-> (vals [C, ...] contiguous `dtype`, alpha_src fp32 alike, cell table or None, n, h, w, whether a leading category axis was added)."""
    ops._dev(vals, alpha_src, coords_norm)
    if vals.shape != alpha_src.shape:
        raise ValueError(f"values and alpha source must have one shape, got {tuple(vals.shape)} and {tuple(alpha_src.shape)}")
    base = 1 if coords_norm is not None else 2
    if vals.dim() not in (base, base + 1):
        raise ValueError(f"expected {'[C, tiles] or [tiles]' if base == 1 else '[C, H, W] or [H, W]'}, got {tuple(vals.shape)}")
    single = vals.dim() == base
    if single:
        vals, alpha_src = vals[None], alpha_src[None]
    if vals.shape[0] < 1:
        raise ValueError("no category")
    vals, alpha_src = vals.detach().to(dtype).contiguous(), alpha_src.detach().float().contiguous()
    if coords_norm is None:
        return vals, alpha_src, None, 0, int(vals.shape[1]), int(vals.shape[2]), single
    cells, h, w = _cells(coords_norm, int(vals.shape[1]))
    return vals, alpha_src, cells, int(vals.shape[1]), h, w, single


def colorize(arg: torch.Tensor, alpha_src: torch.Tensor, cmap: str, *, coords_norm: torch.Tensor | None = None, scale: int = 8,
             out: torch.Tensor | None = None) -> torch.Tensor:
    """`np.uint8(plt.get_cmap(cmap)(x) * 255)` with alpha = 255 where `alpha_src` > 0, enlarged `scale` times by pixel replication (:500-529, 600-609,
    683-717; amds_heatmap_raster, all categories in one launch).  With `coords_norm` int64 [N, 2]: arg, alpha_src per tile, [C, N] or [N], scattered like
    `vals_to_im` (a cell without a tile: argument 0 -> lut[0], alpha 0).  Without: images [C, H, W] or [H, W].  -> u8 [C, scale * H, scale * W, 4]
    (without the leading C for an input without it).  NaN -> RGB (0, 0, 0); x < 0 -> the first, x >= 1 -> the last table entry."""
    arg, alpha_src, cells, n, h, w, single = _sources(arg, alpha_src, coords_norm, torch.float32)
    scale = int(scale)
    if scale < 1:
        raise ValueError("scale must be >= 1")
    lut = _lut(cmap, arg.device)
    res = _out(out, ((h * scale, w * scale, 4) if single else (arg.shape[0], h * scale, w * scale, 4)), arg.device)
    _lib.check(_lib.lib().amds_heatmap_raster(arg.data_ptr(), alpha_src.data_ptr(), ops._p(cells), lut.data_ptr(), lut.shape[0], res.data_ptr(),
                                              arg.shape[0], n, h, w, scale, ops._stream()), "heatmap_raster")
    return res


def class_map(top: torch.Tensor, alpha_src: torch.Tensor, *, coords_norm: torch.Tensor | None = None, scale: int = 8,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """`_show_class_map` (:241-258) and its resize (:445-448): Pastel1 of each tile's top class (an integer tensor; an index >= 9 takes the last entry),
    alpha = 255 where `alpha_src` > 0 (the reference: `gradcam_2d.sum(-1)`).  With `coords_norm`: per tile [N]; without: images [H, W].  A cell without a
    tile is the first table entry with alpha 0.  -> u8 [scale * H, scale * W, 4] (amds_heatmap_classmap)."""
    if top.is_floating_point() or top.dtype == torch.bool:
        raise ValueError(f"top must hold integer class indices, got {top.dtype}")
    if top.dim() != (1 if coords_norm is not None else 2):
        raise ValueError(f"top must be {'[tiles]' if coords_norm is not None else '[H, W]'}, got {tuple(top.shape)}")
    top, alpha_src, cells, n, h, w, _ = _sources(top, alpha_src, coords_norm, torch.int32)
    scale = int(scale)
    if scale < 1:
        raise ValueError("scale must be >= 1")
    lut = _lut("Pastel1", top.device)
    res = _out(out, (h * scale, w * scale, 4), top.device)
    _lib.check(_lib.lib().amds_heatmap_classmap(top.data_ptr(), alpha_src.data_ptr(), ops._p(cells), lut.data_ptr(), lut.shape[0], res.data_ptr(), n, h, w,
                                                scale, ops._stream()), "heatmap_classmap")
    return res


def resize_index_table(n_in: int, n_out: int) -> list[int]:
    """The source index of every output index of Pillow's NEAREST resize from n_in to n_out samples: its running sum in double (`a = n_in / n_out`,
    `xo = 0.5 * a`, then `src = int(xo); xo += a` in order).  The closed form floor((i + 0.5) * a) rounds differently."""
    if n_in < 1 or n_out < 1:
        raise ValueError("sizes must be >= 1")
    a = n_in / n_out
    xo, tab = 0.5 * a, []
    for _ in range(n_out):
        tab.append(min(int(xo), n_in - 1))
        xo += a
    return tab


def overlay(score_rgba: torch.Tensor, thumb: torch.Tensor, opacity: float = 0.6, *, scale: int = 1, out: torch.Tensor | None = None) -> torch.Tensor:
    """`_create_overlay` (:261-284) for all categories in one launch (amds_heatmap_overlay): score_rgba u8 [C, scale * H, scale * W, 4] or without the C,
    as `colorize` returns it at `scale` (1: the unscaled image the reference resizes; any scale gives the same bytes), thumb u8 [th, tw, 3] ->
    u8 [C, th, tw, 3].  The score image is resized to the thumbnail by Pillow's NEAREST rule (`resize_index_table`, built on the host) and blended in
    binary64 where its alpha byte is > 0; elsewhere the thumbnail's byte is returned.  0 <= opacity <= 1."""
    ops._dev(score_rgba, thumb)
    if score_rgba.dtype != torch.uint8 or thumb.dtype != torch.uint8:
        raise ValueError("score_rgba and thumb must be uint8")
    single = score_rgba.dim() == 3
    if single:
        score_rgba = score_rgba[None]
    scale = int(scale)
    if score_rgba.dim() != 4 or score_rgba.shape[3] != 4 or scale < 1 or score_rgba.shape[0] < 1 or score_rgba.shape[1] % scale or score_rgba.shape[2] % scale \
            or min(score_rgba.shape[1:3]) < scale:
        raise ValueError(f"score_rgba must be [C, scale * H, scale * W, 4] or [scale * H, scale * W, 4], got {tuple(score_rgba.shape)} at scale {scale}")
    if thumb.dim() != 3 or thumb.shape[2] != 3 or thumb.shape[0] < 1 or thumb.shape[1] < 1:
        raise ValueError(f"thumb must be [th, tw, 3], got {tuple(thumb.shape)}")
    if not 0.0 <= float(opacity) <= 1.0:
        raise ValueError(f"opacity must lie in [0, 1], got {opacity}")
    score_rgba, thumb = score_rgba.contiguous(), thumb.contiguous()
    Cn, h, w = score_rgba.shape[0], score_rgba.shape[1] // scale, score_rgba.shape[2] // scale
    th, tw = int(thumb.shape[0]), int(thumb.shape[1])
    tabs = torch.tensor(resize_index_table(h, th) + resize_index_table(w, tw), dtype=torch.int32).to(thumb.device)
    res = _out(out, ((th, tw, 3) if single else (Cn, th, tw, 3)), thumb.device)
    _lib.check(_lib.lib().amds_heatmap_overlay(score_rgba.data_ptr(), thumb.data_ptr(), tabs.data_ptr(), tabs[th:].data_ptr(), float(opacity), res.data_ptr(),
                                               Cn, h, w, scale, th, tw, ops._stream()), "heatmap_overlay")
    return res


def ranked_tiles(scores: torch.Tensor, topk: int, bottomk: int):
    """The tiles `_export_ranked_tiles` saves (:216-238): -> (top_idx, top_val, bottom_idx, bottom_val), the `min(topk, N)` highest scores in descending
    and the `min(bottomk, N)` lowest in ascending order; among equal scores the lower tile index comes first (a stable sort).  Plumbing: no kernel, any
    device."""
    s = scores.detach().flatten()
    kt, kb = max(min(int(topk), s.numel()), 0), max(min(int(bottomk), s.numel()), 0)
    tv, ti = torch.sort(s, descending=True, stable=True)
    bv, bi = torch.sort(s, descending=False, stable=True)
    return ti[:kt], tv[:kt], bi[:kb], bv[:kb]


def _slide_heatmap_abmil(model: GatedAttentionMIL, feats: torch.Tensor, coords_um: torch.Tensor, task: str, tiles_per_call: int | None) -> SlideHeatmap:
    if tiles_per_call is not None and int(tiles_per_call) < 1:
        raise ValueError("tiles_per_call must be >= 1")
    classify = task == "classification"
    if not classify and model.n_classes != 1:
        raise ValueError(f"gradcam_single is for single-output models (dim_output == 1), this one has {model.n_classes} outputs: use gradcam")
    with _eval_mode(model):
        sc = _abmil_scores(model, feats, want_cam=True, want_tiles=classify)
    cn = grid_coords(coords_um)
    logits = sc["logits"][0]
    if not classify:
        cam = sc["cam_raw"][0]
        g2 = vals_to_im(cam, cn)
        g2 = (g2 - g2.min()) / (g2.max() - g2.min() + 1e-8)
        return SlideHeatmap(task, logits.squeeze(), cn, cam, g2, tile_relevance=cam / cam.max().clamp(min=1e-8), tile_attention=sc["probs"])
    cam = _softmax_over_tiles(sc["cam_raw"])
    scores = torch.softmax(sc["tile_logits"], dim=1)
    support, attention, cat = category_maps(cam, scores)
    return SlideHeatmap(task, logits.softmax(0), cn, cam, vals_to_im(cam, cn), scores, vals_to_im(scores, cn), support, attention, cat, tile_attention=sc["probs"])


def slide_heatmap(model: torch.nn.Module, feats: torch.Tensor, coords_um: torch.Tensor, *, task: str, method: str = "auto",
                  tiles_per_call: int | None = None) -> SlideHeatmap:
    """One slide, `task` "classification" (:401-498), "regression" (:586-597) or "survival" (:668-679, the regression computation; its colouring is
    `SlideHeatmap.render`'s): slide score, Grad-CAM scores, per-tile scores, their 2-D arrangements and the per-category maps -- the tensors the
    reference's plotting takes from here.  `method` goes to `gradcam` / `gradcam_single`, `tiles_per_call` to `tile_scores`.
    `abmil.GatedAttentionMIL` on its library route: ONE library call gives all of it (bit for bit what the single functions return: `tiles_per_call`
    changes no bit for this head and is not needed), and `tile_attention` holds the softmax weights."""
    if task not in ("classification", "regression", "survival"):
        raise ValueError(f"task must be 'classification', 'regression' or 'survival', got {task!r}")
    _check_inputs(feats, coords_um)
    if isinstance(model, GatedAttentionMIL) and _pick(model, method) == "library":
        return _slide_heatmap_abmil(model, feats, coords_um, task, tiles_per_call)
    with _eval_mode(model), torch.no_grad():
        logits = model(feats.unsqueeze(0), coords=coords_um.unsqueeze(0), mask=None).squeeze(0)          # :392-399
    cn = grid_coords(coords_um)
    if task != "classification":
        cam = gradcam_single(model, feats, coords_um, method=method)
        g2 = vals_to_im(cam, cn)
        g2 = (g2 - g2.min()) / (g2.max() - g2.min() + 1e-8)
        return SlideHeatmap(task, logits.squeeze(), cn, cam, g2, tile_relevance=cam / cam.max().clamp(min=1e-8))
    cam = gradcam(model, feats, coords_um, method=method)
    scores = tile_scores(model, feats, coords_um, tiles_per_call=tiles_per_call)
    support, attention, cat = category_maps(cam, scores)
    return SlideHeatmap(task, logits.softmax(0), cn, cam, vals_to_im(cam, cn), scores, vals_to_im(scores, cn), support, attention, cat)
