"""TransMIL heat maps without a GPU: the reference fixture (tests/golden/heatmaps_transmil.npz, written by tools/make_golden.py `golden_heatmaps_transmil`
from the reference's own TransMIL, `_gradcam_per_category` and `_gradcam_single`) against torch autograd through oracle.transmil -- which pins the
oracle's GRADIENT to the reference and is what tests/test_gpu_heatmaps_transmil.py judges the GPU routes against --, the `_pick` routing table and the
chunk arithmetic of `tile_scores`."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.transmil import transmil_forward
from stamp_amd import heatmaps, transmil_core
from stamp_amd.mil import TransMIL, VisionTransformer

G = Path(__file__).parent / "golden"
SLIDES = [(61, 3), (50, 14), (49, 0)]          # (tiles, wrap-padded tiles: side 8 for all three)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _fixture():
    z = np.load(G / "heatmaps_transmil.npz")
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    sd1 = {k[len("single:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("single:")}
    return z, sd, sd1


def oracle_cam_raw(feats, sd, dtype):
    """|mean_f feats * d logit_c / d feats| by torch autograd through the oracle -> ([N, C], logits [C])."""
    x = feats.to(dtype)
    sdt = {k: v.to(dtype) for k, v in sd.items()}
    f = lambda b: transmil_forward(b.unsqueeze(0), sdt, dtype=dtype).squeeze(0)  # noqa: E731
    jac = torch.autograd.functional.jacobian(f, x)
    with torch.no_grad():
        logits = f(x)
    return (x * jac).mean(-1).abs().t().contiguous(), logits


# ---- (a) the oracle's gradient is the reference's --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,add", SLIDES)
def test_fixture_equals_oracle_autograd(N, add):
    """fp32 oracle + autograd against the reference's fp32 values: rtol = atol = 1e-4, the bar tests/test_oracle_golden.py::test_transmil puts on the
    TransMIL logits fixtures; the fp64 oracle's distance is printed (and the relative L2 of both, which the GPU tests speak in)."""
    z, sd, sd1 = _fixture()
    C, F, D = (int(v) for v in z["hparams"])
    feats = torch.from_numpy(z[f"feats_{N}"])
    side = int(np.ceil(np.sqrt(N)))
    assert feats.shape == (N, F) and side * side - N == add
    cam_raw, cam_single, logits = (torch.from_numpy(z[f"{k}_{N}"]) for k in ("cam_raw", "cam_single", "slide_logits"))
    assert cam_raw.shape == (N, C) and cam_single.shape == (N,) and logits.shape == (C,)
    got, got_logits = oracle_cam_raw(feats, sd, torch.float32)
    got1, _ = oracle_cam_raw(feats, sd1, torch.float32)
    r64, l64 = oracle_cam_raw(feats, sd, torch.float64)
    r64_1, _ = oracle_cam_raw(feats, sd1, torch.float64)
    print(f"N={N} add={add}: fixture vs fp32 oracle rel-L2 cam_raw {_rel(got, cam_raw):.3e} cam_single {_rel(got1[:, 0], cam_single):.3e} "
          f"logits max abs {(got_logits - logits).abs().max().item():.3e} | vs fp64 oracle rel-L2 cam_raw {_rel(cam_raw, r64):.3e} "
          f"cam_single {_rel(cam_single, r64_1[:, 0]):.3e} logits max abs {(logits.double() - l64).abs().max().item():.3e}")
    # the scores are small (cam_raw <= 3.5e-3, cam_single <= 7e-4): the absolute term of the logits' bar alone would let a wrong wrap-padding term through, so
    # the relative L2 is asserted too -- fp32 sums in another order on another torch build: 1e-5 (measured 3 - 5e-7)
    assert _rel(got, cam_raw) <= 1e-5 and _rel(got1[:, 0], cam_single) <= 1e-5 and max(_rel(got[:, c], cam_raw[:, c]) for c in range(C)) <= 1e-5
    np.testing.assert_allclose(got.numpy(), cam_raw.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(got1[:, 0].numpy(), cam_single.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(got_logits.numpy(), logits.numpy(), rtol=1e-4, atol=1e-4)
    # the fixture's other members are what the reference's lines make of these
    assert (torch.softmax(cam_raw, 0) - torch.from_numpy(z[f"cam_{N}"])).abs().max() < 1e-6
    with torch.no_grad():
        tl = transmil_forward(feats.double().unsqueeze(-2), {k: v.double() for k, v in sd.items()}, dtype=torch.float64)
    assert (torch.softmax(tl, 1) - torch.from_numpy(z[f"scores_{N}"]).double()).abs().max() < 1e-4
    # the fixture discriminates between the classes (the head's rows were scaled apart)
    assert _rel(r64[:, 0], r64[:, 1]) >= 0.5, _rel(r64[:, 0], r64[:, 1])


# ---- (b) routing ---------------------------------------------------------------------------------------------------------------------------
def test_pick_routing_table():
    """Every (class, method) pair.  Pinned by tests/test_gpu_heatmaps.py::test_generic_route_is_the_references_lines and unchanged: "auto" on TransMIL is
    jacrev, "fused" on TransMIL is a ValueError."""
    vit = VisionTransformer.__new__(VisionTransformer)          # stand-ins: `_pick` looks at the class alone
    tm = TransMIL.__new__(TransMIL)
    other = torch.nn.Linear(2, 2)
    table = {
        (vit, "auto"): "fused", (vit, "fused"): "fused", (vit, "jacrev"): "jacrev", (vit, "library"): "fused",
        (tm, "auto"): "jacrev", (tm, "fused"): ValueError, (tm, "jacrev"): "jacrev", (tm, "library"): "library",
        (other, "auto"): "jacrev", (other, "fused"): ValueError, (other, "jacrev"): "jacrev", (other, "library"): ValueError,
    }
    for (model, method), want in table.items():
        if want is ValueError:
            with pytest.raises(ValueError, match=method):
                heatmaps._pick(model, method)
        else:
            assert heatmaps._pick(model, method) == want, (type(model).__name__, method)
    for model in (vit, tm, other):
        with pytest.raises(ValueError, match="method must be"):
            heatmaps._pick(model, "rollout")


# ---- (c) the chunk of tile_scores ----------------------------------------------------------------------------------------------------------------
def test_tile_scores_chunk_arithmetic(monkeypatch):
    """The library query and the free-memory read mocked: a workspace of `per_bag` bytes per bag + a constant.  TransMIL: the largest bag count <= 8191
    under half of the free memory; anything else keeps 32768; the slide runs in groups of 8191 tiles in order, a group above the chunk staged; an explicit chunk
    above the limit raises."""
    assert transmil_core.MAX_BAGS_PER_CALL == 8191 and heatmaps.MAX_BAGS_PER_CALL == 32768
    per_bag, const = 1000, 512
    asked = []

    class Lib:
        @staticmethod
        def amds_transmil_workspace_bytes(cfg, bags, tiles):
            asked.append((cfg._obj.n_feats, cfg._obj.dim, cfg._obj.classes, bags, tiles))
            return const + per_bag * bags

    free = [0]
    monkeypatch.setattr(heatmaps._lib, "lib", lambda: Lib)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (free[0], 1 << 40))
    tm = TransMIL(dim_output=3, dim_input=16, dim_hidden=32)
    for free_bytes, want in ((1 << 40, 8191), (2 * (const + per_bag * 8191), 8191), (2 * (const + per_bag * 8191) - 2, 8190), (2 * (const + per_bag * 100) + 1, 100),
                             (2 * (const + per_bag * 100) - 1, 99), (2 * (const + per_bag), 1), (0, 1)):
        free[0] = free_bytes
        assert heatmaps.default_tiles_per_call(tm) == want, (free_bytes, want)
    assert all(a[:3] == (16, 32, 3) and a[4] == 1 and 1 <= a[3] <= 8191 for a in asked)
    vit = VisionTransformer.__new__(VisionTransformer)
    assert heatmaps.default_tiles_per_call(vit) == 32768 and heatmaps.default_tiles_per_call(torch.nn.Linear(2, 2)) == 32768
    # what tile_scores makes of it: groups of 8191 tiles whatever the chunk; a group larger than the chunk goes to the staged forward, else to the module
    seen = []

    def fwd(self, bags, *, coords=None, mask=None):
        assert bags.shape[1] == 1 and mask.shape == (bags.shape[0], 1) and not mask.any()
        seen.append(("module", bags.shape[0]))
        return bags[:, 0, :3].float()

    def grouped(w, dims, h, bags_per_call):
        assert w == "weights" and dims == (16, 32, 3) and h.shape[1:] == (1, 16)
        seen.append(("staged", h.shape[0], bags_per_call))
        return h[:, 0, :3].float()

    monkeypatch.setattr(TransMIL, "forward", fwd)
    monkeypatch.setattr(TransMIL, "_c_weights", lambda self, dev: "weights")
    monkeypatch.setattr(transmil_core, "forward_infer_grouped", grouped)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    feats = torch.randn(8200, 16)
    want = torch.softmax(feats[:, :3], 1)
    free[0] = 1 << 40
    assert torch.equal(heatmaps.tile_scores(tm, feats), want) and seen == [("module", 8191), ("module", 9)]
    seen.clear()
    free[0] = 2 * (const + per_bag * 3000)
    assert torch.equal(heatmaps.tile_scores(tm, feats), want) and seen == [("staged", 8191, 3000), ("module", 9)]
    seen.clear()
    assert torch.equal(heatmaps.tile_scores(tm, feats, tiles_per_call=8191), want) and seen == [("module", 8191), ("module", 9)]
    seen.clear()
    assert torch.equal(heatmaps.tile_scores(tm, feats, tiles_per_call=5), want) and seen == [("staged", 8191, 5), ("staged", 9, 5)]
    with pytest.raises(ValueError, match="8191"):
        heatmaps.tile_scores(tm, feats, tiles_per_call=8192)
    with pytest.raises(ValueError):
        heatmaps.tile_scores(tm, feats, tiles_per_call=0)


def test_staged_partition_keeps_the_one_calls_kernel_choices():
    """The sub-call sizes of a staged group (host only): never above the chunk, summing to the group, every one in the group's row class for `_fc1`
    (bags x tiles rows) and `to_qkv` (bags x padded tokens) -- the library's own query, which the staged entry enforces."""
    import ctypes as C

    from stamp_amd import _lib
    lib = _lib.lib()
    for (F, D), group, step in (((32, 128), 4096, 1000), ((32, 128), 8191, 4096), ((1024, 512), 8191, 100), ((1024, 512), 4096, 300), ((32, 64), 8191, 1000),
                                ((32, 64), 8200 - 8191, 5), ((40, 72), 1000, 999)):
        cfg = _lib.TransMilCfg(F, D, 3)
        ok = lambda s: bool(lib.amds_transmil_staged_compatible(C.byref(cfg), group, s, 1))  # noqa: E731
        parts = transmil_core.staged_partition(ok, group, step)
        assert sum(parts) == group and max(parts) <= step and all(ok(p) for p in parts), (F, D, group, step, parts)
        assert ok(group) and not ok(group + 1) and not ok(0)
    cfg = _lib.TransMilCfg(32, 128, 3)          # dim_hidden 128: one-tile bags are padded to 64 token rows, `_fc1` can be a bgemm product
    ok = lambda g, s: bool(lib.amds_transmil_staged_compatible(C.byref(cfg), g, s, 1))  # noqa: E731
    assert ok(4096, 768) and ok(4096, 256) and not ok(4096, 1000) and not ok(4096, 128)          # whole tiles of 256 rows on both sides, or not
    assert ok(8191, 4095) and not ok(8191, 4096) and not ok(8191, 1)                             # 8191 x 64 rows: whole tiles of 64 only; one bag is <= 64 rows
    assert transmil_core.staged_partition(lambda s: True, 10, 20) == [10] and transmil_core.staged_partition(lambda s: True, 10, 4) == [4, 4, 2]
    assert transmil_core.staged_partition(lambda s: s >= 3, 11, 4) == [4, 4, 3]          # (4, 4 and a remainder of 3; with 10 bags: 4, 3, 3)
    assert transmil_core.staged_partition(lambda s: s >= 3, 10, 4) == [4, 3, 3]
    with pytest.raises(RuntimeError, match="tiles_per_call"):
        transmil_core.staged_partition(lambda s: False, 10, 4)
    cfg512 = _lib.TransMilCfg(1024, 512, 3)          # 4096 rows of `_fc1` are whole tiles of 256: no sub-call of at most 100 bags is
    with pytest.raises(RuntimeError, match="tiles_per_call"):
        transmil_core.staged_partition(lambda s: bool(lib.amds_transmil_staged_compatible(C.byref(cfg512), 4096, s, 1)), 4096, 100)
