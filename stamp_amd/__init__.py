"""stamp_amd: STAMP's compute stages on the HIP path.  Sub-modules are imported by name (`stamp_amd.encoder`, `stamp_amd.mil`, `stamp_amd.deploy`, ...);
the heat-map entry points of `stamp_amd.heatmaps` and the attention-MIL head of `stamp_amd.abmil` are also reachable from here, resolved on first use
(importing the package stays free of torch)."""
_HEATMAPS = ("gradcam", "gradcam_single", "tile_scores", "grid_coords", "vals_to_im", "category_maps", "slide_heatmap", "SlideHeatmap",
             "colorize", "class_map", "overlay", "ranked_tiles", "resize_index_table", "colormap_table", "HeatmapImages")
_ABMIL = ("GatedAttentionMIL", "HipAbmilTrainer")
__all__ = list(_HEATMAPS) + list(_ABMIL)


def __getattr__(name: str):
    if name in _HEATMAPS:
        from . import heatmaps
        return getattr(heatmaps, name)
    if name in _ABMIL:
        from . import abmil
        return getattr(abmil, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
