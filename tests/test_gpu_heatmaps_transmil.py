"""TransMIL heat maps on the GPU: `method="library"` (transmil_core.forward_train -> amds_transmil_gradcam -> amds_softmax_over_tiles) against the reference
fixture, the fp64 oracle and the existing jacrev route; the tile scores past the forward's bag limit; memory; the call contract.

The parity rule, everywhere: relative L2 per class, e_new <= max(2 * e_old, bar) with e_old the jacrev route's error against the same reference measured in
the same test and bar the per-gradient bar this backward already carries -- 1e-4 at "highest", 2e-4 at "high" (tests/test_gpu_transmil_train.py).  Both
routes run the same launches down to layer1's LayerNorm backward; they differ in the last step alone (an fp32 row-dot against h - b here, a dbags GEMM and
torch's feats * jac mean there)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.transmil import transmil_forward
from stamp_amd import _lib, heatmaps, ops, transmil_core
from stamp_amd.mil import TransMIL

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
BAR = {"highest": 1e-4, "high": 2e-4}


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / (b.double().cpu().norm() + 1e-30)).item()


def _per_class(got, ref):
    """got, ref [N, C] (or [N]) -> relative L2 of every class."""
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    if got.dim() == 1:
        return [_rel(got, ref)]
    return [_rel(got[:, c], ref[:, c]) for c in range(ref.shape[1])]


def _rule(what, new, old, ref, precision):
    e_new, e_old = _per_class(new, ref), _per_class(old, ref)
    print(f"{what} [{precision}]: e_new {['%.3e' % e for e in e_new]} | e_old (jacrev) {['%.3e' % e for e in e_old]} | bar {BAR[precision]:.0e}")
    for n_, o_ in zip(e_new, e_old):
        assert n_ <= max(2 * o_, BAR[precision]), (what, e_new, e_old)
    return e_new, e_old


def _oracle_cam(model, feats):
    """fp64 autograd through the oracle: |mean_f feats * d logit_c / d feats| [N, C]."""
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    x = feats.detach().cpu().double()
    jac = torch.autograd.functional.jacobian(lambda b: transmil_forward(b.unsqueeze(0), sd, dtype=torch.float64).squeeze(0), x)
    return (x * jac).mean(-1).abs().t().contiguous()


def _model(C_, F, D, seed, gpu):
    torch.manual_seed(seed)
    model = TransMIL(dim_output=C_, dim_input=F, dim_hidden=D).eval()
    with torch.no_grad():           # class rows that differ, as in the fixture
        model._fc2.weight.mul_(4.0)
    return model.to(gpu)


# ---- 1. the reference's fixture ------------------------------------------------------------------------------------------------------------------
def _load(gpu):
    z = np.load(G / "heatmaps_transmil.npz")
    Cn, F, D = (int(v) for v in z["hparams"])
    model, one = TransMIL(dim_output=Cn, dim_input=F, dim_hidden=D).eval(), TransMIL(dim_output=1, dim_input=F, dim_hidden=D).eval()
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}, strict=True)
    one.load_state_dict({k[len("single:"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("single:")}, strict=True)
    return z, model.to(gpu), one.to(gpu)


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("N", [61, 50, 49])
def test_reference_fixture(gpu, N, precision):
    """tests/golden/heatmaps_transmil.npz holds what the reference's own TransMIL and heat-map functions returned: N = 61 / 50 / 49 tiles on an 8 x 8 grid
    (3 / 14 / 0 wrap-padded tiles).  cam_raw, cam_single, the soft-maxed map and the whole `slide_heatmap`, each under the module docstring's rule."""
    z, model, one = _load(gpu)
    feats, cu = torch.from_numpy(z[f"feats_{N}"]).to(gpu), torch.from_numpy(z[f"coords_um_{N}"]).to(gpu)
    ref_raw, ref_cam, ref_single = (torch.from_numpy(z[f"{k}_{N}"]) for k in ("cam_raw", "cam", "cam_single"))
    with ops.float32_matmul_precision(precision):
        raw = heatmaps.gradcam(model, feats, cu, raw=True, method="library")
        raw_old = heatmaps.gradcam(model, feats, cu, raw=True, method="jacrev")
        cam = heatmaps.gradcam(model, feats, cu, method="library")
        cam_old = heatmaps.gradcam(model, feats, cu, method="jacrev")
        single = heatmaps.gradcam_single(one, feats, cu, method="library")
        single_old = heatmaps.gradcam_single(one, feats, cu, method="jacrev")
        hm = heatmaps.slide_heatmap(model, feats, cu, task="classification", method="library")
        hm_old = heatmaps.slide_heatmap(model, feats, cu, task="classification", method="jacrev")
        hr = heatmaps.slide_heatmap(one, feats, cu, task="regression", method="library")
    assert raw.shape == ref_raw.shape and raw.dtype == torch.float32 and single.shape == (N,)
    _rule(f"fixture N={N} cam_raw", raw, raw_old, ref_raw, precision)
    _rule(f"fixture N={N} cam_single", single, single_old, ref_single, precision)
    _rule(f"fixture N={N} cam", cam, cam_old, ref_cam, precision)
    _rule(f"fixture N={N} slide_heatmap.gradcam", hm.gradcam, hm_old.gradcam, ref_cam, precision)
    assert torch.allclose(cam.sum(0).cpu(), torch.ones(cam.shape[1]), atol=1e-5)
    assert (cam.cpu() - torch.softmax(raw.cpu(), 0)).abs().max() < 1e-7          # the library's softmax over the tiles
    assert torch.equal(hm.gradcam, cam) and torch.equal(hr.gradcam, single)
    tol = 2e-3 * max(1.0, float(np.abs(z[f"slide_logits_{N}"]).max()))          # the logit bar of tests/test_gpu_transmil_train.py; softmax is 1-Lipschitz
    assert (hm.slide_score.cpu() - torch.softmax(torch.from_numpy(z[f"slide_logits_{N}"]), 0)).abs().max() < tol
    assert (hm.scores.cpu() - torch.from_numpy(z[f"scores_{N}"])).abs().max() < 2e-3
    assert hm.support.shape == hm.attention.shape == hm.category_score.shape == (cam.shape[1], N) and hr.slide_score.dim() == 0
    assert all(p.grad is None for p in model.parameters()) and not feats.requires_grad


# ---- 2. edge geometry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("N,D", [(1, 64), (2, 64), (3, 64), (5, 64), (13, 72)])
def test_edge_geometry(gpu, N, D, precision):
    """N = 1, 2, 3, 5: add = 0, 2, 1, 4 wrap-padded tiles (N = 2: every tile wrapped once; N = 1: no wrap at all, the sequence is the class token and one
    tile); dim_hidden 72: rows of 72 columns, lanes 9.. of the row-dot wave skip (N = 13: 4 x 4 grid, add = 3).  Reference: fp64 autograd through the oracle."""
    model = _model(3, 40, D, 100 + N, gpu)
    feats = torch.randn(N, 40, generator=torch.Generator().manual_seed(N)).to(gpu)
    ref = _oracle_cam(model, feats)
    with ops.float32_matmul_precision(precision):
        new = heatmaps.gradcam(model, feats, raw=True, method="library")
        old = heatmaps.gradcam(model, feats, raw=True, method="jacrev")
    assert new.shape == (N, 3)
    _rule(f"edge N={N} dim_hidden={D}", new, old, ref, precision)


@pytest.mark.parametrize("precision", ["highest", "high"])
def test_two_bags_through_the_core(gpu, precision):
    """n_bags = 2 through transmil_core.gradcam: cam_raw [C, 2 * T], bag b's tiles at columns b * T ..  The bags of one call are NOT independent: the
    pseudo-inverse starts from maxima over all bags and heads (trans_mil.py:26-28), so the reference is the batch's own -- dlogits = e_c for every bag is
    the gradient of sum_b logit_c[b], here through fp64 autograd on the oracle and through jacrev on the module (e_old), both on the two-bag batch."""
    from torch.func import jacrev

    T, F = 11, 40           # 4 x 4 grid, add = 5
    model = _model(3, F, 64, 7, gpu)
    bags = torch.randn(2, T, F, generator=torch.Generator().manual_seed(8)).to(gpu)
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    x = bags.cpu().double()
    jac = torch.autograd.functional.jacobian(lambda b: transmil_forward(b, sd, dtype=torch.float64).sum(0), x)          # [C, 2, T, F]
    ref = (x * jac).mean(-1).abs().reshape(3, 2 * T).t()
    with ops.float32_matmul_precision(precision):
        _, saved = transmil_core.forward_train(model._get(gpu), bags, (F, 64, 3), training=False)
        cam = transmil_core.gradcam(saved)
        assert cam.shape == (3, 2 * T) and torch.equal(cam, transmil_core.gradcam(saved))
        with torch.enable_grad():
            jg = jacrev(lambda b: model(b).sum(0))(bags)
        old = (bags * jg).mean(-1).abs().reshape(3, 2 * T).t()
    _rule("two bags", cam.t(), old, ref, precision)
    assert _rel(ref[:T], ref[T:]) >= 0.5          # (the two bags' maps differ: a swap of the bags could not pass)


# ---- 3. parity at a slide-like size ------------------------------------------------------------------------------------------------------------
N_SLIDE, F_SLIDE, D_SLIDE = 1024, 256, 128
_ORACLE: dict = {}


def _slide_case(gpu):
    model = _model(3, F_SLIDE, D_SLIDE, 21, gpu)
    feats = torch.randn(N_SLIDE, F_SLIDE, generator=torch.Generator().manual_seed(22))
    return model, feats


@pytest.mark.parametrize("precision", ["highest", "high"])
def test_library_gradcam_parity_at_slide_size(gpu, precision):
    """N = 1024 (32 x 32 grid, no wrap; n = 1025 front-padded to 1088), F = 256, dim_hidden 128, C = 3 against fp64 autograd through the oracle; at "high"
    `_fc1` runs as a bf16 x 3 product and the arena's h is the PRE-activation.  e_new <= 2 * e_old per class, and e_old <= 0.05 and the oracle's class-0 and
    class-1 maps >= 0.5 apart (conditions on the inputs: checked on the CPU when the case was written, 0.78)."""
    model, feats = _slide_case(gpu)
    if "ref" not in _ORACLE:
        _ORACLE["ref"] = _oracle_cam(model, feats)
    ref = _ORACLE["ref"]
    d01 = _rel(ref[:, 0], ref[:, 1])
    assert d01 >= 0.5, d01
    fg = feats.to(gpu)
    with ops.float32_matmul_precision(precision):
        new = heatmaps.gradcam(model, fg, raw=True, method="library")
        old = heatmaps.gradcam(model, fg, raw=True, method="jacrev")
    e_new, e_old = _per_class(new, ref), _per_class(old, ref)
    print(f"slide-size parity [{precision}]: e_new {['%.3e' % e for e in e_new]} | e_old {['%.3e' % e for e in e_old]} | class0-vs-1 {d01:.2f}")
    assert max(e_old) <= 0.05, e_old
    for n_, o_ in zip(e_new, e_old):
        assert n_ <= 2 * o_, (e_new, e_old)


# ---- 4. memory ---------------------------------------------------------------------------------------------------------------------------------------
def test_library_gradcam_needs_no_jacobian_memory(gpu):
    """N = 4096, F = 1024, dim_hidden 128, C = 4, both routes warmed once: the library call's peak is lower than the jacrev call's by at least
    0.9 * C * N * F * 4 bytes, the Jacobian that no longer exists."""
    Cn, N, F = 4, 4096, 1024
    model = _model(Cn, F, 128, 31, gpu)
    feats = torch.randn(N, F, device=gpu)
    heatmaps.gradcam(model, feats, raw=True, method="library")
    heatmaps.gradcam(model, feats, raw=True, method="jacrev")
    peaks = {}
    for method in ("library", "jacrev"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        heatmaps.gradcam(model, feats, raw=True, method=method)
        torch.cuda.synchronize()
        peaks[method] = torch.cuda.max_memory_allocated()
        print(f"TransMIL gradcam peak memory {method}: {peaks[method] / 2**20:.1f} MiB (allocated before the call {base / 2**20:.1f} MiB)")
    assert peaks["jacrev"] - peaks["library"] >= 0.9 * Cn * N * F * 4, peaks


# ---- 5. tile scores past the forward's bag limit ---------------------------------------------------------------------------------------------------
def test_tile_scores_past_the_bag_limit(gpu):
    """N = 8200 one-tile bags: amds_transmil_forward takes 8191 per call, so the default chunk splits the slide at 8191."""
    N = 8200
    model = _model(3, 32, 64, 41, gpu)
    feats = torch.randn(N, 32, device=gpu)
    sc = heatmaps.tile_scores(model, feats)
    assert sc.shape == (N, 3) and sc.dtype == torch.float32
    with torch.no_grad():
        for a, e in ((0, 8191), (8191, N)):
            direct = torch.softmax(model(feats[a:e].unsqueeze(-2), coords=None, mask=torch.zeros(e - a, 1, dtype=torch.bool, device=gpu)), 1)
            assert torch.equal(sc[a:e], direct), (a, e)
    assert torch.equal(sc, heatmaps.tile_scores(model, feats, tiles_per_call=1000))
    with pytest.raises(ValueError, match="8191"):
        heatmaps.tile_scores(model, feats, tiles_per_call=9000)
    cu = torch.stack([torch.arange(300) % 20, torch.arange(300) // 20], 1).float().to(gpu) * 256.0          # `slide_heatmap` passes the chunk through
    hm = heatmaps.slide_heatmap(model, feats[:300], cu, task="classification", method="library", tiles_per_call=128)
    assert torch.equal(hm.scores, heatmaps.tile_scores(model, feats[:300], tiles_per_call=128))
    with pytest.raises(ValueError, match="8191"):
        heatmaps.slide_heatmap(model, feats[:300], cu, task="classification", tiles_per_call=9000)


@pytest.mark.parametrize("precision", ["highest", "high"])
def test_tile_scores_chunking_is_bit_invariant(gpu, precision):
    """The same slide with tiles_per_call=1000 (and 4096, and 8191) equals the default chunking bit for bit, although a TransMIL bag's logits depend on the bags
    that share its call (the pseudo-inverse starts from maxima over ALL bags and heads of a call, trans_mil.py:26-28; two plain chunkings of this slide differ by
    3.3e-4 in the probabilities, on every row): the groups whose maxima are shared are fixed at 8191 tiles, and a smaller `tiles_per_call` runs a group staged
    (amds_transmil_forward_staged) with the group's maxima.  Also the staged forward itself on bags of 50 tiles, against the one call."""
    N = 8200
    model = _model(3, 32, 64, 41, gpu)
    feats = torch.randn(N, 32, device=gpu)
    with ops.float32_matmul_precision(precision):
        sc = heatmaps.tile_scores(model, feats)
        for step in (1000, 4096, 8191):
            ch = heatmaps.tile_scores(model, feats, tiles_per_call=step)
            print(f"tile scores [{precision}], default chunk against tiles_per_call={step}: max abs difference {(sc - ch).abs().max().item():.3e}, rows that differ "
                  f"{int((sc != ch).any(1).sum())} of {N}")
            assert torch.equal(sc, ch), step
        bags = torch.randn(20, 50, 32, device=gpu)
        w, dims = model._c_weights(gpu), (32, 64, 3)
        one = transmil_core.forward_infer(w, dims, bags)
        for step in (7, 10, 19, 20):
            assert torch.equal(transmil_core.forward_infer_grouped(w, dims, bags, step), one), step
        halves = torch.cat([transmil_core.forward_infer(w, dims, bags[:10]), transmil_core.forward_infer(w, dims, bags[10:])])
        assert not torch.equal(halves, one)          # (the coupling is there: two plain half-batches differ -- the maxima lie in one of them at most)


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("N,step", [(4096, 1000), (8191, 4096)])
def test_staged_group_keeps_the_one_calls_kernels(gpu, N, step, precision):
    """dim_hidden 128, F = 32: the two products over the rows of all bags of a call pick their kernel by the row count -- below "highest" `_fc1` is a bf16 x 3
    amds_bgemm_f32 product when bags x tiles is a multiple of 128 (4096: yes; 8191: no) and the exact Linear otherwise, and to_qkv's 64 padded rows per bag make
    whole 128-row tiles for an even bag count alone.  A staged group repeats the ONE call's choices whatever its sub-calls would choose for themselves
    (tiles_per_call 1000 is no multiple of 128; 4096 is one, 8191 is not): bit for bit the module's own call."""
    model = _model(3, 32, 128, 61, gpu)
    feats = torch.randn(N, 32, device=gpu)
    with ops.float32_matmul_precision(precision):
        with torch.no_grad():
            direct = torch.softmax(model(feats.unsqueeze(-2), coords=None, mask=torch.zeros(N, 1, dtype=torch.bool, device=gpu)), 1)
        assert torch.equal(heatmaps.tile_scores(model, feats, tiles_per_call=8191), direct)
        got = heatmaps.tile_scores(model, feats, tiles_per_call=step)
        print(f"staged group N={N} tiles_per_call={step} [{precision}]: max abs difference {(got - direct).abs().max().item():.3e}, rows that differ "
              f"{int((got != direct).any(1).sum())} of {N}")
        assert torch.equal(got, direct)
    if N == 4096:          # a sub-call outside the group's row class (128 rows of `_fc1`: no whole 256-row tile) is refused, nothing launched
        cfg = _lib.TransMilCfg(32, 128, 3)
        ws = torch.empty(_lib.lib().amds_transmil_workspace_bytes(C.byref(cfg), 128, 1), dtype=torch.uint8, device=gpu)
        mx = torch.zeros(4, dtype=torch.int32, device=gpu)
        rc = _lib.lib().amds_transmil_forward_staged(C.byref(cfg), C.byref(model._c_weights(gpu)), feats.data_ptr(), 2, None, 128, 1, N, 0, mx.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), ops._stream())
        assert rc == -1 and b"kernel choices" in _lib.lib().amds_last_error() and int(mx.abs().sum()) == 0


# ---- 6. contract -----------------------------------------------------------------------------------------------------------------------------------------
def test_contract(gpu):
    model = _model(3, 40, 64, 51, gpu).train()
    feats = torch.randn(61, 40, device=gpu)
    a, b = heatmaps.gradcam(model, feats, method="library"), heatmaps.gradcam(model, feats, method="library")
    assert torch.equal(a, b)
    assert torch.equal(heatmaps.gradcam(model, feats, raw=True, method="library"), heatmaps.gradcam(model, feats, raw=True, method="library"))
    assert model.training and all(p.grad is None for p in model.parameters()) and not feats.requires_grad
    model.eval()
    heatmaps.gradcam(model, feats.half(), method="library")                       # 16-bit features are staged to fp32 by the forward
    assert not model.training
    with pytest.raises(ValueError, match="library"):
        heatmaps.gradcam(torch.nn.Linear(40, 3).to(gpu), feats, method="library")
    with pytest.raises(ValueError):
        heatmaps.gradcam_single(model, feats, method="library")                   # dim_output == 3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        heatmaps.gradcam(model, feats.cpu(), method="library")
    with pytest.raises(ValueError):
        heatmaps.gradcam(model, feats[:, :39], method="library")
    # the C entry: a short workspace is AMDS_ERR_WORKSPACE before anything is launched; the lean plan never exceeds the training plan
    lib = _lib.lib()
    _, saved = transmil_core.forward_train(model._get(gpu), feats.unsqueeze(0), (40, 64, 3), training=False)
    need = lib.amds_transmil_gradcam_workspace_bytes(C.byref(saved["cfg"]), 1, 61)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    cam = torch.full((3, 61), -7.0, device=gpu)
    arena = saved["arena"]

    def call(ws_bytes, arena_bytes=arena.numel(), bags=1):
        return lib.amds_transmil_gradcam(C.byref(saved["cfg"]), C.byref(saved["w"]), bags, 61, arena.data_ptr(), arena_bytes, cam.data_ptr(), ws.data_ptr(), ws_bytes,
                                         ops._stream())

    assert call(need - 1) == -2 and b"workspace" in lib.amds_last_error()         # AMDS_ERR_WORKSPACE
    assert call(need, arena.numel() - 1) == -2
    assert call(need, bags=0) == 0
    torch.cuda.synchronize()
    assert bool((cam == -7.0).all())                                              # nothing was launched
    assert call(need) == 0
    torch.cuda.synchronize()
    assert torch.equal(cam, transmil_core.gradcam(saved))
    for Cn, F, D, Bb, T in ((3, 40, 64, 1, 61), (3, 40, 72, 1, 13), (3, 40, 64, 2, 11), (3, 40, 64, 1, 1), (3, 256, 128, 1, 1024), (4, 1024, 128, 1, 4096),
                            (2, 1024, 512, 1, 8192), (1000, 1, 8, 3, 1)):
        cfg = _lib.TransMilCfg(F, D, Cn)
        lean, full = (f(C.byref(cfg), Bb, T) for f in (lib.amds_transmil_gradcam_workspace_bytes, lib.amds_transmil_train_workspace_bytes))
        assert 0 < lean <= full, (Cn, F, D, Bb, T, lean, full)
