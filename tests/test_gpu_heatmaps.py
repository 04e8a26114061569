"""Heat-map scores on the GPU (stamp_amd.heatmaps): the reference's fixtures, parity of the fused Grad-CAM path and of the existing jacrev path against
fp64 autograd at a slide-like size, tile scores, memory, the generic route, the fp16 guard and determinism.

Every parity statement is about `cam_raw`, the scores BEFORE the softmax over the tiles: they are small, so the soft-maxed map stays within a per cent of
the uniform 1 / N whatever the gradient is and proves nothing alone.  Each parity test also asserts that its inputs discriminate (the oracle's maps of
class 0 and class 1 differ by >= 0.5 relative L2, five times the largest error accepted below)."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.mil_vit import mil_vit_forward
from stamp_amd import heatmaps
from stamp_amd.mil import TransMIL, VisionTransformer

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
FIXTURES = [("plain", False), ("alibi", True)]


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / (b.double().cpu().norm() + 1e-30)).item()


def _perturb(model, scale=0.05):
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1 and "class_token" not in n and "bias_scale" not in n:
                p.add_(scale * torch.randn_like(p))


def _load(tag, alibi, gpu, prefix="w:", dim_output=None):
    z = np.load(G / f"heatmaps_{tag}.npz")
    C, F, D, L, H, FF = (int(v) for v in z["hparams"])
    model = VisionTransformer(dim_output=dim_output or C, dim_input=F, dim_model=D, n_layers=L, n_heads=H, dim_feedforward=FF, dropout=0.0, use_alibi=alibi).eval()
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}, strict=True)
    return z, model.to(gpu)


# ---- 4. the reference's fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,alibi", FIXTURES)
def test_reference_fixture(gpu, tag, alibi):
    """tests/golden/heatmaps_*.npz hold what the reference's own functions returned (tools/make_golden.py `golden_heatmaps`).  cam_raw: 0.1 relative L2
    (all classes and each class; 16-bit operands on a 64-wide zero-padded head -- the fixture's classes differ by > 0.8), cam: the softmax's
    bound on that error, scores: 5e-3 absolute (the floor of the logit bar 5e-3 * max(1, |logits|max); softmax is 1-Lipschitz in the max norm),
    `vals_to_im`: bit-exact (it is a copy)."""
    z, model = _load(tag, alibi, gpu)
    feats, cu, cn = (torch.from_numpy(z[k]).to(gpu) for k in ("feats", "coords_um", "coords_norm"))
    ref_raw, ref_cam = torch.from_numpy(z["cam_raw"]), torch.from_numpy(z["cam"])
    assert _rel(ref_raw[:, 0], ref_raw[:, 1]) >= 0.5
    raw = heatmaps.gradcam(model, feats, cu, raw=True)
    assert raw.shape == ref_raw.shape and raw.dtype == torch.float32
    errs = [_rel(raw, ref_raw)] + [_rel(raw[:, c], ref_raw[:, c]) for c in range(raw.shape[1])]
    print(f"{tag}: fused cam_raw vs reference fixture, all / per class: {['%.3e' % e for e in errs]}")
    assert max(errs) < 0.1, errs
    cam = heatmaps.gradcam(model, feats, cu)
    assert cam.shape == ref_cam.shape
    assert torch.allclose(cam.sum(0).cpu(), torch.ones(cam.shape[1]), atol=1e-5)
    assert (cam.cpu() - torch.softmax(raw.cpu(), 0)).abs().max() < 1e-7          # the library's softmax over the tiles
    eps = (raw.cpu() - ref_raw).abs().max().item()                       # softmax(x + d) / softmax(x) lies in [e^-2eps, e^2eps] for |d| <= eps
    assert (cam.cpu() - ref_cam).abs().max() <= ref_cam.max() * np.expm1(2 * eps) + 1e-7
    # half-precision features take the same path
    assert _rel(heatmaps.gradcam(model, feats.half(), cu, raw=True), ref_raw) < 0.1
    assert all(p.grad is None for p in model.parameters()) and not feats.requires_grad
    # the single-output model
    _, one = _load(tag, alibi, gpu, prefix="single:", dim_output=1)
    single = heatmaps.gradcam_single(one, feats, cu)
    assert single.shape == (feats.shape[0],) and _rel(single, torch.from_numpy(z["cam_single"])) < 0.1
    with pytest.raises(ValueError):
        heatmaps.gradcam_single(model, feats, cu)
    # tile scores
    sc = heatmaps.tile_scores(model, feats, cu)
    assert (sc.cpu() - torch.from_numpy(z["scores"])).abs().max() < 5e-3, (sc.cpu() - torch.from_numpy(z["scores"])).abs().max()
    # the 2-D arrangement of the REFERENCE's values: a copy, bit for bit
    im = heatmaps.vals_to_im(ref_cam.to(gpu), cn)
    assert im.shape == z["cam_2d"].shape and torch.equal(im.cpu(), torch.from_numpy(z["cam_2d"]))
    assert torch.equal(heatmaps.grid_coords(cu), cn)
    s, a, c = heatmaps.category_maps(ref_cam.to(gpu), torch.from_numpy(z["scores"]).to(gpu))
    for got, key in ((s, "support"), (a, "attention"), (c, "category_score")):
        assert torch.allclose(got.cpu(), torch.from_numpy(z[key]), rtol=1e-5, atol=1e-7), key
    # the whole slide
    hm = heatmaps.slide_heatmap(model, feats, cu, task="classification")
    assert torch.equal(hm.gradcam, cam) and torch.equal(hm.scores, sc) and torch.equal(hm.coords_norm, cn) and hm.gradcam_2d.shape == z["cam_2d"].shape
    assert (hm.slide_score.cpu() - torch.softmax(torch.from_numpy(z["slide_logits"]), 0)).abs().max() < 5e-3 * max(1.0, float(np.abs(z["slide_logits"]).max()))
    assert hm.support.shape == hm.attention.shape == hm.category_score.shape == (cam.shape[1], cam.shape[0])
    hr = heatmaps.slide_heatmap(one, feats, cu, task="regression")
    assert torch.equal(hr.gradcam, single) and hr.gradcam_2d.shape == z["cam_2d"].shape[:2] and hr.slide_score.dim() == 0
    assert float(hr.gradcam_2d.min()) == 0.0 and abs(float(hr.gradcam_2d.max()) - 1.0) < 1e-4 and abs(float(hr.tile_relevance.max()) - 1.0) < 1e-6


def test_vals_to_im_duplicates_shapes_and_bounds(gpu):
    """Several tiles on one cell: the highest tile index wins (the reference's indexed assignment on the CPU); 1-D and n-D values; empty cells are zero;
    a coordinate outside the grid is an error, not a fault."""
    xy = torch.tensor([[0, 0], [2, 1], [0, 0], [1, 0], [2, 1], [2, 1]], device=gpu)
    vals = torch.arange(1.0, 13.0, device=gpu).reshape(6, 2)
    im = heatmaps.vals_to_im(vals, xy)
    want = torch.zeros(2, 3, 2)
    want[0, 0], want[0, 1], want[1, 2] = vals[2].cpu(), vals[3].cpu(), vals[5].cpu()
    assert torch.equal(im.cpu(), want)
    flat = torch.zeros(6, 2)                                   # the reference's own lines on the CPU
    cpu_xy = xy.cpu()
    flat[cpu_xy[:, 1] * 3 + cpu_xy[:, 0]] = vals.cpu()
    assert torch.equal(im.cpu(), flat.reshape(2, 3, 2))
    assert torch.equal(heatmaps.vals_to_im(vals[:, 0], xy).cpu(), want[..., 0])
    v3 = torch.randn(6, 2, 3, device=gpu)
    assert heatmaps.vals_to_im(v3, xy).shape == (2, 3, 2, 3) and torch.equal(heatmaps.vals_to_im(v3, xy)[1, 2], v3[5])
    assert heatmaps.vals_to_im(vals.half(), xy).dtype == torch.float16
    # many duplicates, many times: always the last
    n = 100_000
    xy2 = torch.randint(0, 40, (n, 2), device=gpu)
    v2 = torch.arange(n, device=gpu, dtype=torch.float32)[:, None]
    im2 = heatmaps.vals_to_im(v2, xy2)
    last = torch.full((int(xy2[:, 1].max()) + 1, int(xy2[:, 0].max()) + 1), -1, dtype=torch.long)
    cx = xy2.cpu()
    for t in range(n - 4000, n):                                # (every cell of the 40 x 40 grid is named again in the last 4000 tiles with near certainty)
        last[cx[t, 1], cx[t, 0]] = t
    hit = last >= 0
    assert torch.equal(im2.cpu()[..., 0][hit], last[hit].float())
    assert torch.equal(im2, heatmaps.vals_to_im(v2, xy2))
    bad = xy.clone()
    bad[1, 0] = -1
    with pytest.raises(RuntimeError, match="outside"):
        heatmaps.vals_to_im(vals, bad)


# ---- 5. parity at a slide-like size --------------------------------------------------------------------------------------------------------
N_SLIDE, F_SLIDE = 4096, 1024
_ORACLE: dict = {}


def _slide_case(alibi, C, gpu):
    """The default head (dim 512, 8 heads, feed-forward 512, 2 layers) with perturbed 1-D parameters, N = 4096 tiles on a 256-um grid."""
    torch.manual_seed(11 + int(alibi))
    model = VisionTransformer(dim_output=C, dim_input=F_SLIDE, dim_model=512, n_layers=2, n_heads=8, dim_feedforward=512, dropout=0.0, use_alibi=alibi).eval()
    _perturb(model)
    feats = torch.randn(N_SLIDE, F_SLIDE).half().float()
    cells = torch.randperm(80 * 64)[:N_SLIDE]
    coords = torch.stack([cells % 80, cells // 80], dim=1).float() * 256.0
    if alibi:           # the scaler buffers as a training run leaves them: the mean tile distance
        with torch.no_grad():
            md = torch.cdist(coords, coords).mean()
            for n, b in model.named_buffers():
                if n.endswith("running_mean"):
                    b.fill_(md)
    return model, feats, coords


def _oracle(alibi, gpu):
    """(cam_raw [N, C] fp64, logits [C] fp64, one-tile-bag logits [N, C] fp64) of the C = 3 slide case, computed once per head."""
    if alibi not in _ORACLE:
        model, feats, coords = _slide_case(alibi, 3, gpu)
        sd = {k: v.clone().double() for k, v in model.state_dict().items()}
        x = feats.double()
        c64 = coords.double()
        f = lambda b: mil_vit_forward(b.unsqueeze(0), c64.unsqueeze(0), None, sd, n_heads=8, use_alibi=alibi, dtype=torch.float64).squeeze(0)  # noqa: E731
        jac = torch.autograd.functional.jacobian(f, x)
        with torch.no_grad():
            logits = f(x)
            tile_logits = mil_vit_forward(x.unsqueeze(-2), c64.unsqueeze(-2), torch.zeros(N_SLIDE, 1, dtype=torch.bool), sd, n_heads=8, use_alibi=alibi,
                                          dtype=torch.float64)
        _ORACLE[alibi] = ((x * jac).mean(-1).abs().t().contiguous(), logits, tile_logits)
    return _ORACLE[alibi]


@pytest.mark.parametrize("precision", ["medium", "high"])
@pytest.mark.parametrize("alibi", [False, True])
def test_fused_gradcam_parity_at_slide_size(gpu, alibi, precision):
    """N = 4096 tiles, F = 1024, default head, C = 3, both operand types: e_new (fused) and e_old (method="jacrev", the existing path) are the relative L2
    errors of cam_raw against fp64 autograd through the oracle, all classes together and the worst single class.  Required: e_new <= 2 * e_old (the two
    paths round in different places -- a 16-bit z - b here, a 16-bit dz operand there -- and neither is exact), e_new < 0.1 whatever e_old is, and
    e_old <= 0.05 (else the inputs cancel too much in the mean over the features to test anything)."""
    ref, ref_logits, _ = _oracle(alibi, gpu)
    d01 = _rel(ref[:, 0], ref[:, 1])
    assert d01 >= 0.5, d01
    model, feats, coords = _slide_case(alibi, 3, gpu)
    model, fg, cg = model.to(gpu), feats.to(gpu), coords.to(gpu)
    old = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision(precision)
        new = heatmaps.gradcam(model, fg, cg, raw=True)
        jr = heatmaps.gradcam(model, fg, cg, raw=True, method="jacrev")
        logits = model(fg[None], coords=cg[None], mask=None)[0]          # the forward both paths start from (the module's autograd forward)
        cam = heatmaps.gradcam(model, fg, cg)
    finally:
        torch.set_float32_matmul_precision(old)
    assert model.fp16_overflow_events == 0
    e_new = [_rel(new, ref)] + [_rel(new[:, c], ref[:, c]) for c in range(3)]
    e_old = [_rel(jr, ref)] + [_rel(jr[:, c], ref[:, c]) for c in range(3)]
    print(f"heatmap parity alibi={alibi} precision={precision} ({'bf16' if precision == 'medium' else 'fp16'} operands): "
          f"e_new all {e_new[0]:.3e} worst class {max(e_new[1:]):.3e} | e_old all {e_old[0]:.3e} worst class {max(e_old[1:]):.3e} | class0-vs-1 {d01:.2f}")
    assert max(e_old) <= 0.05, e_old
    assert e_new[0] <= 2 * e_old[0] and max(e_new[1:]) <= 2 * max(e_old[1:]), (e_new, e_old)
    assert max(e_new) < 0.1, e_new
    assert (logits.detach().cpu().double() - ref_logits).abs().max() < 5e-3 * max(1.0, ref_logits.abs().max().item())
    assert (cam.cpu() - torch.softmax(new.cpu(), 0)).abs().max() < 1e-7 and torch.isfinite(cam).all()


# ---- 6. tile scores ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alibi", [False, True])
def test_tile_scores_at_slide_size(gpu, alibi):
    _, _, tile_logits = _oracle(alibi, gpu)
    model, feats, coords = _slide_case(alibi, 3, gpu)
    model, fg, cg = model.to(gpu), feats.to(gpu), coords.to(gpu)
    tol = 5e-3 * max(1.0, tile_logits.abs().max().item())          # softmax is 1-Lipschitz in the max norm: the logit bar carries over
    want = torch.softmax(tile_logits, 1)
    sc = heatmaps.tile_scores(model, fg, cg)
    assert sc.shape == (N_SLIDE, 3)
    print(f"tile scores alibi={alibi}: max abs error {(sc.cpu().double() - want).abs().max().item():.3e} (bar {tol:.3e})")
    assert (sc.cpu().double() - want).abs().max() < tol
    with torch.no_grad():
        direct = torch.softmax(model(fg.unsqueeze(-2), coords=cg.unsqueeze(-2), mask=torch.zeros(N_SLIDE, 1, dtype=torch.bool, device=gpu)), 1)
    assert torch.equal(sc, direct)
    chunked = heatmaps.tile_scores(model, fg, cg, tiles_per_call=1000)
    assert chunked.shape == sc.shape and (chunked.cpu().double() - want).abs().max() < tol
    assert torch.equal(sc, heatmaps.tile_scores(model, fg, cg))


# ---- 7. memory ----------------------------------------------------------------------------------------------------------------------------------
def test_fused_gradcam_needs_no_jacobian_memory(gpu):
    """Same inputs with C = 4: the fused call's peak is lower than the jacrev call's by at least 0.9 * C * N * F * 4 bytes, the Jacobian that no longer exists."""
    C = 4
    model, feats, coords = _slide_case(False, C, gpu)
    model, fg, cg = model.to(gpu), feats.to(gpu), coords.to(gpu)
    heatmaps.gradcam(model, fg, cg, raw=True)                        # (the library's cached scratch buffers then exist for both)
    heatmaps.gradcam(model, fg, cg, raw=True, method="jacrev")
    peaks = {}
    for method in ("fused", "jacrev"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        heatmaps.gradcam(model, fg, cg, raw=True, method=method)
        torch.cuda.synchronize()
        peaks[method] = torch.cuda.max_memory_allocated()
        print(f"gradcam peak memory {method}: {peaks[method] / 2**20:.1f} MiB (allocated before the call {base / 2**20:.1f} MiB)")
    assert peaks["jacrev"] - peaks["fused"] >= 0.9 * C * N_SLIDE * F_SLIDE * 4, peaks


# ---- 8. the generic route -----------------------------------------------------------------------------------------------------------------------
def test_generic_route_is_the_references_lines(gpu):
    from torch.func import jacrev

    torch.manual_seed(5)
    model = TransMIL(dim_output=3, dim_input=128, dim_hidden=64).eval().to(gpu)
    feats, coords = torch.randn(300, 128, device=gpu), torch.rand(300, 2, device=gpu) * 5000
    got = heatmaps.gradcam(model, feats, coords, raw=True)
    jac = jacrev(lambda bags: model.forward(bags.unsqueeze(0), coords=coords.unsqueeze(0), mask=None).squeeze(0))(feats)
    want = (feats * jac).mean(-1).abs().permute(-1, -2)
    assert got.shape == (300, 3) and torch.allclose(got, want, rtol=1e-5, atol=0)
    assert torch.equal(got, want)                                   # TransMIL's backward is deterministic
    cam = heatmaps.gradcam(model, feats, coords)
    assert torch.equal(cam, torch.softmax(want.permute(-1, -2), dim=-1).permute(-1, -2))
    with pytest.raises(ValueError):
        heatmaps.gradcam(model, feats, coords, method="fused")
    assert all(p.grad is None for p in model.parameters())


# ---- 9. the fp16 guard -----------------------------------------------------------------------------------------------------------------------
def test_fp16_overflow_reruns_on_bf16(gpu):
    """fp32 features beyond fp16's range at float32_matmul_precision "high": the staged fp16 operands overflow, the guard (one 4-byte read) sees non-finite
    logits and the slide runs again on bf16 operands -- the very computation "medium" asks for.  An overflow in arithmetic, answered by a re-run."""
    torch.manual_seed(9)
    model = VisionTransformer(dim_output=3, dim_input=256, dim_model=256, n_layers=2, n_heads=4, dim_feedforward=256, dropout=0.0, use_alibi=False).eval().to(gpu)
    feats = torch.randn(200, 256, device=gpu)
    old = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision("high")
        ok = heatmaps.gradcam(model, feats, raw=True)
        assert model.fp16_overflow_events == 0 and torch.isfinite(ok).all()
        big = heatmaps.gradcam(model, feats * 1e5, raw=True)
        assert model.fp16_overflow_events == 1 and torch.isfinite(big).all()
        torch.set_float32_matmul_precision("medium")
        assert torch.equal(big, heatmaps.gradcam(model, feats * 1e5, raw=True))
        assert model.fp16_overflow_events == 1
    finally:
        torch.set_float32_matmul_precision(old)


# ---- 10. determinism ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alibi", [False, True])
def test_determinism(gpu, alibi):
    torch.manual_seed(3)
    model = VisionTransformer(dim_output=4, dim_input=384, dim_model=256, n_layers=2, n_heads=4, dim_feedforward=512, dropout=0.1, use_alibi=alibi).eval().to(gpu)
    feats = torch.randn(1500, 384, device=gpu)
    cells = torch.randperm(50 * 40)[:1500]
    coords = (torch.stack([cells % 50, cells // 50], dim=1).float() * 224.0).to(gpu)
    a, b = heatmaps.gradcam(model, feats, coords), heatmaps.gradcam(model, feats, coords)
    assert torch.equal(a, b)
    assert torch.equal(heatmaps.gradcam(model, feats, coords, raw=True), heatmaps.gradcam(model, feats, coords, raw=True))
    assert torch.equal(heatmaps.tile_scores(model, feats, coords), heatmaps.tile_scores(model, feats, coords))
    cn = heatmaps.grid_coords(coords)
    assert torch.equal(heatmaps.vals_to_im(a, cn), heatmaps.vals_to_im(a, cn))
