"""Heat maps of the gated-attention MIL head on the GPU (amds_abmil_heatmap, stamp_amd/abmil.py `heatmap_scores`, stamp_amd/heatmaps.py) against
tests/abmil_heatmap_oracle.py in fp64.

Bars: test_gpu_abmil.py's `_check`, per tensor, err = max |hip - fp64| / max |fp64|.
  "highest": max(4 x the error of the same oracle run by torch in fp32 on the CPU -- `cam_autograd`, the reference's own route, for cam_raw --, gamma(n)).
  "high":    2e-4 relative L2 per tensor.
Cases are test_gpu_abmil.py's `_case` (every pre-activation clear of the ReLU's kink: cam_raw carries the same [h > 0] jump as dx).  Every figure is printed
before it is asserted (profiles/abmil_heatmap_errors.txt holds a run's output).
Paths of the two new kernels: 16-byte lanes (L % 4 == 0, D % 4 == 0) or scalar ones ("odd": L = 70, D = 30); W_cls and b_fc in LDS below 64 KB, in LDS past the
opt-in ("c300": 77 KB), read through the caches past 160 KB ("c700"; "odd700": scalar lanes as well); classes in groups of four with a remainder of 1, 2, 3
(C = 5, 1 / 2 / 6, 3); lanes past the row's end (L = 64 / 72 / 70 < 256); more rows than one sweep of the grid covers (the 8 200-row case: 2 050 workgroups).
"""
import ctypes as C

import pytest
import torch

import abmil_heatmap_oracle as H
import abmil_oracle as O
import guarded as G
import test_gpu_abmil as T
from test_gpu_abmil import GEOMS, RAGGED, _case, _check

pytestmark = pytest.mark.gpu

# (`_case` and `_check` look their geometry up by name)
GEOMS.setdefault("rem", (40, 72, 24, 5))
GEOMS.setdefault("single", (48, 64, 32, 1))
GEOMS.setdefault("c300", (48, 64, 32, 300))
GEOMS.setdefault("c700", (48, 64, 32, 700))
GEOMS.setdefault("odd", (50, 70, 30, 6))
GEOMS.setdefault("odd700", (50, 70, 30, 700))
CASES = [("ragged", RAGGED, "random"), ("dense", [33, 33, 33], "random"), ("peak", RAGGED, "peak"), ("equal", [1, 2, 17, 65, 257], "equal"), ("long", [4200], "random")]
NAMES = ["logits", "attn_raw", "probs", "cam_raw", "tile_logits"]
_REFS: dict = {}


def _refs(key, x, lengths, w):
    """fp64 reference and fp32 CPU yardstick of a case, computed once."""
    if key not in _REFS:
        out = []
        for dt in (torch.float64, torch.float32):
            r = O.forward(x, lengths, w, dtype=dt)
            r["cam_raw"], r["tile_logits"] = H.cam_autograd(x, lengths, w, dt), H.tile_logits(x, w, dt)
            out.append(r)
        _REFS[key] = tuple(out)
    return _REFS[key]


def _call(geom, x, lengths, w, gpu, **kw):
    from stamp_amd import abmil
    wd = {k: w[k].to(gpu).contiguous() for k in O.KEYS}
    ws, keep = abmil._weights_struct(lambda k: wd[k])
    return abmil.heatmap_scores(ws, GEOMS[geom], x.to(gpu), abmil._offsets(lengths, gpu), len(lengths), **kw)


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("geom", ["small", "xs", "rem", "single"])
def test_every_tensor_against_fp64(gpu, geom, case, precision):
    from stamp_amd import ops
    tag, lengths, family = case
    x, w = _case(geom, lengths, family)
    ref64, ref32 = _refs((geom, tag), x, lengths, w)
    with ops.float32_matmul_precision(precision):
        got = _call(geom, x, lengths, w, gpu)
    assert got["cam_raw"].shape == (GEOMS[geom][3], sum(lengths)) and got["tile_logits"].shape == (sum(lengths), GEOMS[geom][3])
    _check(f"heatmap {geom}/{tag}", geom, lengths, got, ref64, ref32, NAMES, precision)


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("geom", ["c300", "c700", "odd", "odd700"])
def test_kernel_paths_against_fp64(gpu, geom, precision):
    """The other instantiations of the two kernels (module docstring), and 8 200 rows of "small": the row loop of a workgroup past the first sweep."""
    from stamp_amd import ops
    lengths = [5, 9, 300]
    x, w = _case(geom, lengths, "random", seed=7)
    ref64, ref32 = _refs((geom, "paths"), x, lengths, w)
    with ops.float32_matmul_precision(precision):
        got = _call(geom, x, lengths, w, gpu)
    _check(f"heatmap {geom}/paths", geom, lengths, got, ref64, ref32, NAMES, precision)
    if geom == "c300":
        lengths = [8200]
        x, w = _case("small", lengths, "random", seed=8)
        ref64, ref32 = _refs(("small", "sweep"), x, lengths, w)
        with ops.float32_matmul_precision(precision):
            got = _call("small", x, lengths, w, gpu)
        _check("heatmap small/sweep", "small", lengths, got, ref64, ref32, NAMES, precision)


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("geom", ["small", "xs"])
def test_bit_identity(gpu, geom, precision):
    from stamp_amd import abmil, ops
    lengths = RAGGED
    x, w = _case(geom, lengths, "random", seed=2)
    wd = {k: w[k].to(gpu).contiguous() for k in O.KEYS}
    ws, keep = abmil._weights_struct(lambda k: wd[k])
    xg, offs = x.half().to(gpu), abmil._offsets(lengths, gpu)
    m = T._module(geom, w, gpu).eval()
    with torch.no_grad(), ops.float32_matmul_precision(precision):
        full = abmil.heatmap_scores(ws, GEOMS[geom], xg, offs, len(lengths))
        again = abmil.heatmap_scores(ws, GEOMS[geom], xg, offs, len(lengths))
        logits, raw = abmil.forward_infer(ws, GEOMS[geom], xg, offs, len(lengths), return_attn=True)
        one_row_bags = m.forward_ragged(list(xg.unsqueeze(1)))                      # 1 223 bags of one row each in one call
        own = [abmil.heatmap_scores(ws, GEOMS[geom], b, abmil._offsets([b.shape[0]], gpu), 1) for b in xg.split(lengths)]
        no_cam = abmil.heatmap_scores(ws, GEOMS[geom], xg, offs, len(lengths), want_cam=False)
        no_tiles = abmil.heatmap_scores(ws, GEOMS[geom], xg, offs, len(lengths), want_tiles=False)
        neither = abmil.heatmap_scores(ws, GEOMS[geom], xg, offs, len(lengths), want_cam=False, want_tiles=False)
        module = m.heatmap_scores(list(xg.split(lengths)))
        grouped = m.heatmap_scores(list(xg.split(lengths)), bags_per_call=4)
    assert all(torch.equal(full[k], again[k]) for k in full)
    assert torch.equal(full["logits"], logits) and torch.equal(full["attn_raw"], raw)
    assert torch.equal(full["tile_logits"], one_row_bags)
    # (two fp32 softmaxes of the same scores, each a few units of 2^-24 from the exact value <= 1)
    assert float((full["probs"] - torch.cat([torch.softmax(s, 0) for s in raw.split(lengths)])).abs().max()) < 1e-6
    for k, dim in (("logits", 0), ("attn_raw", 0), ("probs", 0), ("cam_raw", 1), ("tile_logits", 0)):
        assert torch.equal(full[k], torch.cat([o[k] for o in own], dim=dim)), k          # a slide of a ragged call = its own call
        assert torch.equal(full[k], module[k]) and torch.equal(full[k], grouped[k]), k
    assert no_cam["cam_raw"] is None and no_tiles["tile_logits"] is None and neither["cam_raw"] is None and neither["tile_logits"] is None
    for part in (no_cam, no_tiles, neither):
        assert all(torch.equal(full[k], v) for k, v in part.items() if v is not None)
    bag_of = torch.repeat_interleave(torch.arange(len(lengths), device=gpu), torch.tensor(lengths, device=gpu))
    sums = torch.zeros(len(lengths), device=gpu).index_add_(0, bag_of, full["probs"])
    assert float((sums - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("geom", ["small", "rem"])
def test_workspace_contract(gpu, geom, monkeypatch):
    """Poisoned on entry (0x00 / 0xFF), exactly the requested size, guard bands intact, outputs bit-identical and finite; one byte short is refused."""
    from stamp_amd import _lib, abmil
    lengths = [1, 17, 65, 257, 5]
    x, w = _case(geom, lengths, "random", seed=4)
    cfg = abmil._cfg(GEOMS[geom])
    want = _lib.lib().amds_abmil_heatmap_workspace_bytes(C.byref(cfg), len(lengths), sum(lengths))

    def call(pattern):
        with G.scratch_hook(monkeypatch, pattern) as log:
            out = _call(geom, x, lengths, w, gpu)
            torch.cuda.synchronize()
        assert log.bytes_for("abmil_heatmap") == [want]
        return G.Result(out, log.handles)

    G.run_contract(call)
    with G.scratch_hook(monkeypatch, 0xFF, short_by=1) as log:
        with pytest.raises(RuntimeError, match="workspace"):
            _call(geom, x, lengths, w, gpu)
        torch.cuda.synchronize()
        log.assert_bands_intact()


def test_bad_arguments_launch_nothing(gpu):
    from stamp_amd import _lib, abmil
    dims = GEOMS["small"]
    lengths = [5, 9]
    x, w = _case("small", lengths, "random")
    wd = {k: w[k].to(gpu).contiguous() for k in O.KEYS}
    ws_, keep = abmil._weights_struct(lambda k: wd[k])
    lib, cfg = _lib.lib(), abmil._cfg(dims)
    xg, offs = x.to(gpu), abmil._offsets(lengths, gpu)
    n_ws = lib.amds_abmil_heatmap_workspace_bytes(C.byref(cfg), 2, 14)
    bufs = G.Bufs(gpu, 0xFF)
    wsb = bufs.out((n_ws + 256,), torch.uint8, name="ws")
    outs = {"logits": bufs.out((2, 3), torch.float32, name="logits"), "attn": bufs.out((14,), torch.float32, name="attn_raw"), "probs": bufs.out((14,), torch.float32, name="probs"),
            "cam": bufs.out((3, 14), torch.float32, name="cam_raw"), "tiles": bufs.out((14, 3), torch.float32, name="tile_logits")}
    st = G.cur_stream()
    half = _lib.AbmilWeights()
    half.fc_w = ws_.fc_w

    def call(**k):
        return lib.amds_abmil_heatmap(C.byref(k.get("cfg", cfg)), C.byref(k.get("w", ws_)), k.get("x", xg.data_ptr()), k.get("dt", _lib.F32), k.get("offs", offs.data_ptr()),
                                      k.get("bags", 2), k.get("rows", 14), k.get("logits", outs["logits"].data_ptr()), outs["attn"].data_ptr(), outs["probs"].data_ptr(),
                                      outs["cam"].data_ptr(), outs["tiles"].data_ptr(), k.get("ws", wsb.data_ptr()), k.get("wsn", n_ws), st)

    cases = [("null logits", dict(logits=None), "null pointer"), ("null x", dict(x=None), "null pointer"), ("null workspace", dict(ws=None), "null pointer"),
             ("bad dtype", dict(dt=7), "bad x dtype"), ("no offsets", dict(offs=None), "row_offsets"), ("incomplete weights", dict(w=half), "incomplete weights"),
             ("rows < bags", dict(rows=1), "at least one row"), ("misaligned workspace", dict(ws=wsb.data_ptr() + 4), "256-byte aligned"),
             ("bad config", dict(cfg=abmil._cfg((48, 64, 0, 3))), "every width must be >= 1")]
    for name, kw, text in cases:
        rc = call(**kw)
        assert rc == -1 and text in lib.amds_last_error().decode() and "amds_abmil_heatmap" in lib.amds_last_error().decode(), (name, rc, lib.amds_last_error())
    assert call(wsn=n_ws - 1) == -2 and "workspace" in lib.amds_last_error().decode()
    torch.cuda.synchronize()
    for t in [wsb] + list(outs.values()):
        assert bool((t.view(torch.uint8) == 0xFF).all())          # nothing was launched: every byte keeps its poison
    assert call() == 0
    torch.cuda.synchronize()
    for h in bufs.handles:
        h.assert_bands_intact()
    good = _call("small", x, lengths, w, gpu)
    assert torch.equal(outs["cam"], good["cam_raw"]) and torch.equal(outs["tiles"], good["tile_logits"]) and torch.equal(outs["probs"], good["probs"])
    assert bool((wsb[n_ws:] == 0xFF).all())                       # nothing past the size the entry names


def _grid_um(n, width, gpu):
    i = torch.arange(n)
    return torch.stack([i % width, i // width], 1).float().to(gpu) * 256.0


@pytest.mark.parametrize("precision", ["highest", "high"])
def test_heatmaps_module_on_the_gated_attention_head(gpu, precision):
    from stamp_amd import heatmaps, ops
    N = 300
    x, w = _case("small", [N], "random", seed=5)
    m = T._module("small", w, gpu).train()
    feats, cu = x.half().to(gpu), _grid_um(N, 20, gpu)
    ref64, ref32 = _refs(("small", "seam"), x, [N], w)
    with ops.float32_matmul_precision(precision):
        raw = heatmaps.gradcam(m, feats, cu, raw=True)
        cam = heatmaps.gradcam(m, feats, cu, method="library")
        scores = heatmaps.tile_scores(m, feats, cu)
        hm = heatmaps.slide_heatmap(m, feats, cu, task="classification")
        with torch.no_grad():
            logits = m.eval()(feats[None])[0]
            direct = m.heatmap_scores(feats)
            wts, _ = m.attention(feats)
        m.train()
        for step in (7, 128, 299, 300, 5000):
            assert torch.equal(heatmaps.tile_scores(m, feats, cu, tiles_per_call=step), scores), step
        assert torch.equal(heatmaps.slide_heatmap(m, feats, cu, task="classification", method="library", tiles_per_call=64).scores, scores)
    assert m.training and all(p.grad is None for p in m.parameters()) and not feats.requires_grad
    assert raw.shape == (N, 3) and cam.shape == (N, 3) and scores.shape == (N, 3) and raw.dtype == torch.float32
    _check("heatmap small/seam", "small", [N], {"cam_raw": raw.t(), "tile_logits": direct["tile_logits"]}, ref64, ref32, ["cam_raw", "tile_logits"], precision)
    assert torch.equal(scores, torch.softmax(direct["tile_logits"], 1)) and torch.equal(raw.t(), direct["cam_raw"])
    assert float((cam.cpu() - torch.softmax(raw.cpu(), 0)).abs().max()) < 1e-7 and torch.allclose(cam.sum(0).cpu(), torch.ones(3), atol=1e-5)
    # slide_heatmap: one library call, the bits of the single functions
    assert torch.equal(hm.gradcam, cam) and torch.equal(hm.scores, scores) and torch.equal(hm.slide_score, logits.softmax(0))
    support, attention, cat = heatmaps.category_maps(cam, scores)
    assert torch.equal(hm.support, support) and torch.equal(hm.attention, attention) and torch.equal(hm.category_score, cat)
    assert torch.equal(hm.gradcam_2d, heatmaps.vals_to_im(cam, hm.coords_norm)) and torch.equal(hm.scores_2d, heatmaps.vals_to_im(scores, hm.coords_norm))
    assert hm.tile_attention.shape == (N,) and abs(float(hm.tile_attention.sum()) - 1) < 1e-5 and float((hm.tile_attention - wts).abs().max()) < 1e-6
    thumb = torch.randint(0, 256, (45, 61, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(gpu)
    im = hm.render(thumb, scale=4)
    assert im.score_rgba.shape == (3, 4 * 15, 4 * 20, 4) and im.class_map.shape == (4 * 15, 4 * 20, 4) and im.overlay.shape == (3, 45, 61, 3)
    assert im.score_rgba.dtype == im.class_map.dtype == im.overlay.dtype == torch.uint8
    with pytest.raises(ValueError, match="fused"):
        heatmaps.gradcam(m, feats, cu, method="fused")
    with pytest.raises(ValueError):
        heatmaps.gradcam_single(m, feats, cu)                         # dim_output == 3
    with pytest.raises(ValueError):
        heatmaps.gradcam(m, feats[:, :47], cu)


@pytest.mark.parametrize("precision", ["highest", "high"])
def test_single_output_head_regression_and_survival(gpu, precision):
    from stamp_amd import heatmaps, ops
    N = 300
    x, w = _case("single", [N], "random", seed=6)
    m = T._module("single", w, gpu).eval()
    feats, cu = x.to(gpu), _grid_um(N, 20, gpu)
    ref64, ref32 = _refs(("single", "seam"), x, [N], w)
    with ops.float32_matmul_precision(precision):
        cam = heatmaps.gradcam_single(m, feats, cu)
        hr = heatmaps.slide_heatmap(m, feats, cu, task="regression")
        hs = heatmaps.slide_heatmap(m, feats, cu, task="survival", method="library")
        with torch.no_grad():
            out = m(feats[None])
    assert cam.shape == (N,)
    _check("heatmap single/seam", "single", [N], {"cam_raw": cam[None]}, ref64, ref32, ["cam_raw"], precision)
    assert torch.equal(hr.gradcam, cam) and torch.equal(hs.gradcam, cam) and hr.slide_score.dim() == 0 and torch.equal(hr.slide_score, out.squeeze())
    assert torch.equal(hr.tile_relevance, cam / cam.max()) and hr.scores is None and abs(float(hr.tile_attention.sum()) - 1) < 1e-5
    g2 = heatmaps.vals_to_im(cam, hr.coords_norm)
    assert torch.equal(hr.gradcam_2d, (g2 - g2.min()) / (g2.max() - g2.min() + 1e-8))
    for h_, kw in ((hr, {}), (hs, {}), (hs, {"train_pred_median": 0.3})):
        im = h_.render(scale=2, **kw)
        assert im.score_rgba.shape == (1, 2 * 15, 2 * 20, 4) and im.score_rgba.dtype == torch.uint8 and im.class_map is None and im.overlay is None
