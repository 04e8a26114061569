"""Heat-map scores without a GPU: the reference fixtures (tests/golden/heatmaps_*.npz, written by tools/make_golden.py from the reference's own
`_gradcam_per_category`, `_gradcam_single`, `_vals_to_im`, `get_stride` and the inline statements of heatmaps/__init__.py:468-498) against the fp64 oracle,
the host side of the grid functions, and the plumbing of stamp_amd.heatmaps with stand-in kernels."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.mil_vit import mil_vit_forward
from stamp_amd import heatmaps, mil_core
from stamp_amd.mil import VisionTransformer

G = Path(__file__).parent / "golden"
FIXTURES = [("plain", False), ("alibi", True)]


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _fixture(tag):
    z = np.load(G / f"heatmaps_{tag}.npz")
    return z, {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}


def _oracle_cam_raw(feats, coords, sd, H, alibi):
    """fp64 |mean_f feats * d logit_c / d feats| through the oracle, [N, C]."""
    sd = {k: v.double() for k, v in sd.items()}
    x = feats.double()
    jac = torch.autograd.functional.jacobian(
        lambda b: mil_vit_forward(b.unsqueeze(0), coords.double().unsqueeze(0), None, sd, n_heads=H, use_alibi=alibi, dtype=torch.float64).squeeze(0), x)
    return (x * jac).mean(-1).abs().t()


@pytest.mark.parametrize("tag,alibi", FIXTURES)
def test_fixture_equals_oracle(tag, alibi):
    """The reference's fp32 `cam_raw` is the oracle's fp64 one to 1e-4 relative L2 (measured 3e-6: the margin is for another torch build's fp32 sums),
    `scores` to 1e-5 absolute, and `cam` is the softmax of `cam_raw` over the tiles.  The fixture discriminates: the maps of class 0 and class 1 differ by
    more than 0.5 relative L2, so a parity statement on them cannot pass for a gradient that ignores the class."""
    z, sd = _fixture(tag)
    C, F, D, L, H, FF = (int(v) for v in z["hparams"])
    feats, coords = torch.from_numpy(z["feats"]), torch.from_numpy(z["coords_um"])
    ref = _oracle_cam_raw(feats, coords, sd, H, alibi)
    cam_raw = torch.from_numpy(z["cam_raw"])
    assert cam_raw.shape == (feats.shape[0], C)
    e = _rel(cam_raw, ref)
    print(f"{tag}: fixture cam_raw vs fp64 oracle rel-L2 {e:.3e}")
    assert e < 1e-4, e
    assert _rel(ref[:, 0], ref[:, 1]) >= 0.5, _rel(ref[:, 0], ref[:, 1])
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        logits = mil_vit_forward(feats.double().unsqueeze(-2), coords.double().unsqueeze(-2), torch.zeros(len(feats), 1, dtype=torch.bool), sd64, n_heads=H,
                                 use_alibi=alibi, dtype=torch.float64)
    assert (torch.softmax(logits, 1) - torch.from_numpy(z["scores"]).double()).abs().max() < 1e-5
    assert (torch.softmax(cam_raw, 0) - torch.from_numpy(z["cam"])).abs().max() < 1e-6
    # the single-output model's map, same bar
    sd1 = {k[len("single:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("single:")}
    assert _rel(torch.from_numpy(z["cam_single"]), _oracle_cam_raw(feats, coords, sd1, H, alibi)[:, 0]) < 1e-4


@pytest.mark.parametrize("tag", ["plain", "alibi"])
def test_grid_coords_and_image_shape(tag):
    """`grid_coords` = the reference's `(coords_um / get_stride(coords_um)).round().long()`; the image of `_vals_to_im` is [max y + 1, max x + 1, ...]."""
    z, _ = _fixture(tag)
    cu = torch.from_numpy(z["coords_um"])
    cn = heatmaps.grid_coords(cu)
    assert cn.dtype == torch.int64 and torch.equal(cn, torch.from_numpy(z["coords_norm"]))
    assert torch.equal(heatmaps.grid_coords(cu, float(z["stride_um"])), cn)
    assert torch.equal(heatmaps.grid_coords(cu * 2, 2 * float(z["stride_um"])), cn)
    h, w = int(cn[:, 1].max()) + 1, int(cn[:, 0].max()) + 1
    assert z["cam_2d"].shape == (h, w, z["cam"].shape[1]) and h != w          # (x / y order is visible: the grid is not square)
    # the fixture's image holds tile t's values at [y_t, x_t]
    assert np.array_equal(z["cam_2d"][z["coords_norm"][:, 1], z["coords_norm"][:, 0]], z["cam"])
    with pytest.raises(ValueError):
        heatmaps.grid_coords(torch.tensor([[0.0, 0.0], [0.0, 256.0]]))        # one distinct x: no stride
    with pytest.raises(ValueError):
        heatmaps.grid_coords(torch.zeros(5, 3))


@pytest.mark.parametrize("tag", ["plain", "alibi"])
def test_category_maps_equal_the_reference_statements(tag):
    """support / attention / category_score of the fixture come from the reference's statements :468-498, executed once per category."""
    z, _ = _fixture(tag)
    s, a, c = heatmaps.category_maps(torch.from_numpy(z["cam"]), torch.from_numpy(z["scores"]))
    for got, key in ((s, "support"), (a, "attention"), (c, "category_score")):
        assert got.shape == z[key].shape
        assert torch.allclose(got, torch.from_numpy(z[key]), rtol=1e-6, atol=1e-8), key
    # ties: the lower class index is the top class
    sc = torch.tensor([[0.4, 0.4, 0.2], [0.2, 0.4, 0.4]])
    gc = torch.tensor([[0.5, 0.3, 0.2], [0.1, 0.6, 0.3]])
    s, a, _ = heatmaps.category_maps(gc, sc)
    assert torch.equal(s, torch.tensor([[0.0, -0.2], [0.0, 0.0], [-0.2, 0.0]]))
    assert torch.allclose(a[:, 0], torch.tensor([0.5 / 0.6, 0.5 / 0.5, 0.5 / 0.6]))
    with pytest.raises(ValueError):
        heatmaps.category_maps(gc[:, :1], sc[:, :1])


# ---- plumbing with stand-in kernels ---------------------------------------------------------------------------------------------------
def _patch_kernels(monkeypatch):
    """Stand-ins with the signatures of the kernel entry points (as tests/test_cpu_mil_seam.py): logits = mean_t(bags) @ W^T + b on the module's mlp_head
    (dim_input == dim_model), whose Grad-CAM scores have a closed form."""
    calls = {"gradcam": 0, "forward_train": 0, "softmax": 0, "acts": []}

    class PK:
        def __init__(self, dims, get, act, train):
            self.dims, self.W, self.b, self.act = dims, get("mlp_head.0.weight"), get("mlp_head.0.bias"), act
            calls["acts"].append(act)

    def fwd(pk, bags, coords, *, training, seed=0):
        assert training is False
        calls["forward_train"] += 1
        pooled = bags.float().mean(1)
        return pooled @ pk.W.t() + pk.b, dict(bags=bags.float(), shape=tuple(bags.shape))

    def bwd(pk, saved, dlogits, *, need_params=True, need_bags=False, split_k=32):
        Bb, Tn, Fd = saved["shape"]
        dbags = (dlogits @ pk.W)[:, None, :].expand(Bb, Tn, Fd) / Tn if need_bags else None
        return {}, dbags

    def cam(pk, saved, *, scale=1.0):
        calls["gradcam"] += 1
        assert scale == (1024.0 if pk.act == torch.float16 else 1.0)
        Bb, Tn, Fd = saved["shape"]
        return ((saved["bags"][0] @ pk.W.t()) / (Tn * Fd)).abs().t().contiguous()           # [C, N]

    def soft(cam_raw):
        calls["softmax"] += 1
        return torch.softmax(cam_raw, dim=1).t().contiguous()

    import stamp_amd.mil as mil
    monkeypatch.setattr(mil_core, "PackedVit", PK)
    monkeypatch.setattr(mil, "PackedVit", PK)
    monkeypatch.setattr(mil_core, "forward_train", fwd)
    monkeypatch.setattr(mil_core, "backward", bwd)
    monkeypatch.setattr(mil_core, "gradcam", cam)
    monkeypatch.setattr(heatmaps, "_softmax_over_tiles", soft)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return calls


def test_plumbing_dispatch_raw_and_no_param_grads(monkeypatch):
    calls = _patch_kernels(monkeypatch)
    torch.manual_seed(0)
    model = VisionTransformer(dim_output=3, dim_input=16, dim_model=16, n_layers=1, n_heads=2, dim_feedforward=16, dropout=0.0, use_alibi=False).train()
    feats = torch.randn(7, 16)
    want = ((feats @ model.mlp_head[0].weight.detach().t()) / (7 * 16)).abs()            # [N, C]
    raw = heatmaps.gradcam(model, feats, raw=True)
    assert calls == {"gradcam": 1, "forward_train": 1, "softmax": 0, "acts": [torch.float16]}          # auto -> fused, fp16 at the default precision
    assert raw.shape == (7, 3) and torch.allclose(raw, want, atol=1e-7)
    assert model.training                                                                   # eval for the call only
    cam = heatmaps.gradcam(model, feats, method="fused")
    assert calls["softmax"] == 1 and torch.allclose(cam, torch.softmax(want, 0), atol=1e-7) and torch.allclose(cam.sum(0), torch.ones(3))
    # the comparison path: the reference's three lines through the module's autograd Function
    n = calls["gradcam"]
    jr = heatmaps.gradcam(model, feats, raw=True, method="jacrev")
    assert calls["gradcam"] == n and torch.allclose(jr, want, atol=1e-6)
    assert torch.allclose(heatmaps.gradcam(model, feats, method="jacrev"), torch.softmax(want, 0), atol=1e-6)
    old = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision("medium")
        heatmaps.gradcam(model, feats, raw=True)
        assert calls["acts"][-1] == torch.bfloat16
    finally:
        torch.set_float32_matmul_precision(old)
    assert all(p.grad is None for p in model.parameters()) and feats.grad is None and not feats.requires_grad
    assert model.fp16_overflow_events == 0
    # a torch model takes the generic route; "fused" is refused for it
    class Lin(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(16, 3)

        def forward(self, bags, *, coords=None, mask=None):
            return self.fc(bags.mean(1))

    lin = Lin()
    got = heatmaps.gradcam(lin, feats, raw=True)
    assert torch.allclose(got, ((feats @ lin.fc.weight.detach().t()) / (7 * 16)).abs(), atol=1e-7) and all(p.grad is None for p in lin.parameters())
    with pytest.raises(ValueError):
        heatmaps.gradcam(lin, feats, method="fused")
    with pytest.raises(ValueError):
        heatmaps.gradcam(model, feats, method="rollout")
    with pytest.raises(ValueError):
        heatmaps.gradcam(model, feats, torch.zeros(6, 2))
    with pytest.raises(ValueError):
        heatmaps.gradcam_single(model, feats)                                               # dim_output == 3
    with pytest.raises(ValueError):
        heatmaps.gradcam_single(lin, feats)
    one = VisionTransformer(dim_output=1, dim_input=16, dim_model=16, n_layers=1, n_heads=2, dim_feedforward=16, dropout=0.0, use_alibi=False).eval()
    w1 = ((feats @ one.mlp_head[0].weight.detach().t()) / (7 * 16)).abs()[:, 0]
    assert torch.allclose(heatmaps.gradcam_single(one, feats), w1, atol=1e-7)
    assert torch.allclose(heatmaps.gradcam_single(one, feats, method="jacrev"), w1, atol=1e-6)


def test_cpu_tensors_raise():
    model = VisionTransformer(dim_output=2, dim_input=16, dim_model=16, n_layers=1, n_heads=2, dim_feedforward=16, dropout=0.0, use_alibi=False).eval()
    feats, coords = torch.randn(5, 16), torch.zeros(5, 2)
    for call in (lambda: heatmaps.gradcam(model, feats, coords), lambda: heatmaps.gradcam(model, feats, method="jacrev"),
                 lambda: heatmaps.gradcam_single(model, feats), lambda: heatmaps.tile_scores(model, feats, coords),
                 lambda: heatmaps.slide_heatmap(model, feats, coords, task="classification"),
                 lambda: heatmaps.vals_to_im(torch.randn(5, 2), torch.zeros(5, 2, dtype=torch.long))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    import stamp_amd
    assert stamp_amd.gradcam is heatmaps.gradcam and stamp_amd.slide_heatmap is heatmaps.slide_heatmap
