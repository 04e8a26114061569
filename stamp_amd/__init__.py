"""stamp_amd: STAMP's compute stages on the HIP path.  Sub-modules are imported by name (`stamp_amd.encoder`, `stamp_amd.mil`, `stamp_amd.deploy`, ...);
the heat-map entry points of `stamp_amd.heatmaps` are also reachable from here, resolved on first use (importing the package stays free of torch)."""
_HEATMAPS = ("gradcam", "gradcam_single", "tile_scores", "grid_coords", "vals_to_im", "category_maps", "slide_heatmap", "SlideHeatmap",
             "colorize", "class_map", "overlay", "ranked_tiles", "resize_index_table", "colormap_table", "HeatmapImages")
__all__ = list(_HEATMAPS)


def __getattr__(name: str):
    if name in _HEATMAPS:
        from . import heatmaps
        return getattr(heatmaps, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
