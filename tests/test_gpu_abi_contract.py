"""The workspace contract of the whole-model library calls (family A of the C-ABI contract tests; tests/guarded.py).

include/amdstamp.h says of every `ws`: contents on entry are ignored, nothing outside [ws, ws + *_workspace_bytes) is written.  Each case runs
its call on a guarded workspace of EXACTLY the requested size, once filled with 0x00 and once with 0xFF bytes (NaN in every float format, -1 in a
counter) -- saved arenas, flat gradient buffers and d(bags) likewise -- and asserts: the declared outputs are bit-identical between the two runs and
finite, no guard byte changed, and the 0x00 run meets the reference bar of the call's own parity test (restated next to each case, tolerance unchanged).
Then the same small call runs on a workspace a BIGGER call has just used (the grow-only `ops.scratch` of a long-lived process) and must give the bits of
the small call alone; and with `ws_bytes` one byte short -- the real buffer keeps its size -- the call must return an error and write nothing."""
import contextlib
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import guarded as G
from stamp_amd import _lib, mil_core, ops

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"


def test_helper_flags_a_scribbled_band_on_the_device(gpu):
    """No kernel involved: the test itself writes one byte behind a device buffer, and one in front of another."""
    v, h = G.guarded((5, 7), torch.float16, gpu, ld=8, pattern=0xFF)
    v.zero_()
    h.assert_bands_intact()
    h.buf[h.start + h.body] = 1
    with pytest.raises(G.GuardViolation, match="PAST the buffer's end"):
        h.assert_bands_intact()
    _, h0 = G.guarded((64,), torch.float32, gpu, pattern=0x00)
    h0.buf[h0.start - 1] = 1
    with pytest.raises(G.GuardViolation, match="BEFORE the buffer"):
        h0.assert_bands_intact()


# ---- the three checks every case goes through ------------------------------------------------------------------------------------------------
def _hooked(monkeypatch, run, **kw):
    def call(pattern):
        with G.scratch_hook(monkeypatch, pattern, **kw) as log:
            outs = run()
            torch.cuda.synchronize()
        assert any(t != "alloc" for t, _ in log.requests), "the call did not take its workspace from ops.scratch"
        return G.Result(outs, log.handles)
    return call


def _check_case(monkeypatch, run, run_big, bar, short=True):
    alone = G.run_contract(_hooked(monkeypatch, run))
    bar(alone)
    with G.scratch_hook(monkeypatch, 0xFF, persistent=True) as log:          # big, then small on the big call's leftovers
        run_big()
        after_big = {k: v.detach().clone() for k, v in run().items()}
        torch.cuda.synchronize()
    log.assert_bands_intact()
    assert max(n for t, n in log.requests if t != "alloc") > min(n for t, n in log.requests if t != "alloc"), "the big shape asked for no more workspace"
    for k, v in alone.items():
        assert torch.equal(after_big[k], v), f"{k}: the small call's result depends on what ran before it on the same workspace"
    if not short:
        return
    with G.scratch_hook(monkeypatch, 0xFF, short_by=1) as log:                # ws_bytes = need - 1 behind a full-sized buffer
        with pytest.raises(RuntimeError, match="libamdstamp"):
            run()
        torch.cuda.synchronize()
    log.assert_bands_intact()
    for h in log.handles:
        if h.name.startswith("scratch"):
            assert bool((h.view == 0xFF).all()), f"{h.name}: written although ws_bytes was one byte short"


@contextlib.contextmanager
def _cls_tail(on):
    was = ops.set_mil_cls_tail(on)
    try:
        yield
    finally:
        ops.set_mil_cls_tail(was)


def _perturb(model, skip=("class_token", "bias_scale", "scale_distance")):
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1 and not any(s in n for s in skip):
                p.add_(0.05 * torch.randn_like(p))


# ---- MIL `vit` head: inference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,masked,tail", [("plain", False, True), ("alibi", False, True), ("plain", True, True), ("alibi", True, True), ("plain", False, False),
                                             ("alibi", False, False)])
def test_mil_vit_forward(gpu, monkeypatch, tag, masked, tail):
    """amds_mil_vit_forward on the reference's fixture (test_gpu_mil_seam.py: 5e-3 of the logit scale), plain / ALiBi / masked, class-row tail on and off."""
    from stamp_amd.mil import VisionTransformer
    z = np.load(GOLD / f"mil_vit_{tag}.npz")
    Cn, F, D, L, H, FF = (int(v) for v in z["hparams"])
    model = VisionTransformer(dim_output=Cn, dim_input=F, dim_model=D, n_layers=L, n_heads=H, dim_feedforward=FF, dropout=0.0, use_alibi=tag == "alibi").eval()
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}, strict=True)
    model = model.to(gpu)
    pk = model._infer_pack(gpu)
    bags, coords, mask = (torch.from_numpy(z[k]).to(gpu) for k in ("bags", "coords", "mask"))
    g = torch.Generator().manual_seed(1)
    big = (torch.randn(4, 300, F, generator=g).to(gpu), (torch.rand(4, 300, 2, generator=g) * 2000).to(gpu), (torch.rand(4, 300, generator=g) > 0.5).to(gpu))
    ref = z["logits_mask" if masked else "logits_nomask"]

    def run(b=bags, c=coords, m=mask):
        with torch.no_grad(), _cls_tail(tail):
            return {"logits": mil_core.forward_infer(pk, b, c, m if masked else None)}

    def bar(o):
        assert np.abs(o["logits"].cpu().numpy() - ref).max() < 5e-3 * max(1.0, float(np.abs(z["logits_nomask"]).max()))

    _check_case(monkeypatch, run, lambda: run(*big), bar)


@pytest.mark.parametrize("alibi", [False, True])
def test_mil_vit_forward_ragged(gpu, monkeypatch, alibi):
    """amds_mil_vit_forward_ragged, bags of 1 / 77 / 300 tiles at the reference's odd dimensions, against the oracle bag by bag (test_gpu_mil_ragged.py: 6e-3)."""
    from oracle.mil_vit import mil_vit_forward
    from test_gpu_mil_ragged import REFDIMS, _bags, _model
    m = _model(REFDIMS, alibi, seed=3)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(gpu)
    lengths = [1, 77, 300]
    bags, coords = _bags(lengths, REFDIMS["dim_input"], seed=4)
    bigb, bigc = _bags([500, 129, 64, 1000], REFDIMS["dim_input"], seed=5)
    refs = [mil_vit_forward(b.float()[None], c[None], None, sd, n_heads=4, use_alibi=alibi)[0] for b, c in zip(bags, coords)]

    def run(bs=bags, cs=coords):
        with torch.no_grad():
            return {"logits": m.forward_ragged([b.to(gpu) for b in bs], coords=[c.to(gpu) for c in cs])}

    def bar(o):
        for i, ref in enumerate(refs):
            assert (o["logits"][i].cpu() - ref).abs().max() < 6e-3 * max(1.0, ref.abs().max().item()), (i, o["logits"][i], ref)

    _check_case(monkeypatch, run, lambda: run(bigb, bigc), bar)


# ---- MIL `vit` head: training forward + backward, Grad-CAM ----------------------------------------------------------------------------------
def _train_case(gpu, alibi):
    """The shapes, weights and bars of test_gpu_train.py's two training-step parity tests (3 bags of 200 / 150 tiles, 256-d, 4 heads, bf16 operands); eval-mode
    forward (no dropout, no running-mean update), d(logits) = the gradient of the weighted cross-entropy, as the trainer forms it."""
    from oracle.mil_vit import mil_vit_forward
    from stamp_amd.mil import VisionTransformer
    torch.manual_seed(7 if alibi else 5)
    Bb, Tn, Fd, Cn, H = 3, 150 if alibi else 200, 256, 2, 4
    model = VisionTransformer(dim_output=Cn, dim_input=Fd, dim_model=256, n_layers=2, n_heads=H, dim_feedforward=256, dropout=0.0, use_alibi=alibi)
    _perturb(model)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    bags, coords = torch.randn(Bb, Tn, Fd).half(), torch.rand(Bb, Tn, 2) * 3000.0
    if alibi:       # the scalers as a train-mode forward leaves them BEFORE use (this batch's distances folded in), as in the existing test
        from oracle.mil_vit import running_mean_update
        cc = torch.cat([coords.new_zeros(Bb, 1, 2), coords], dim=1)
        dist = torch.cdist(cc, cc)
        for k in [k for k in sd if k.endswith("scale_distance.running_mean")]:
            n_key = k[: -len("running_mean")] + "items_so_far"
            sd[k], sd[n_key] = running_mean_update(sd[k], sd[n_key], dist)
    targets, weights = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0]]), torch.tensor([0.7, 0.3])
    if alibi:       # fp32 autograd through the pinned oracle, as test_mil_vit_alibi_training_step_matches_autograd
        params = {k: v.clone().requires_grad_(not mil_core.is_buffer(k)) for k, v in sd.items()}
        ref_logits = mil_vit_forward(bags.float(), coords, None, params, n_heads=H, use_alibi=True)
        torch.nn.functional.cross_entropy(ref_logits, targets, weight=weights).backward()
        ref_g = {k: v.grad.double() for k, v in params.items() if v.grad is not None}
        ref_logits = ref_logits.detach().double()
    else:
        from test_gpu_train import _oracle_loss_and_grads
        _, ref_logits, ref_g = _oracle_loss_and_grads(sd, bags.float(), targets, weights, H)
    dsd = {k: v.to(gpu, torch.float32) for k, v in sd.items()}
    pk = mil_core.PackedVit(model.dims, lambda n: dsd[n], torch.bfloat16, train=True)
    g = torch.Generator().manual_seed(2)
    big = (torch.randn(4, 400, Fd, generator=g).half().to(gpu), (torch.rand(4, 400, 2, generator=g) * 3000).to(gpu))

    def run(b=bags.to(gpu), c=coords.to(gpu), tg=targets.to(gpu)):
        logits, saved = mil_core.forward_train(pk, b, c if alibi else None, training=False)
        lg = logits.detach().clone().requires_grad_(True)
        tgt = tg if lg.shape[0] == tg.shape[0] else torch.nn.functional.one_hot(torch.arange(lg.shape[0], device=gpu) % Cn, Cn).float()
        torch.nn.functional.cross_entropy(lg, tgt, weight=weights.to(gpu)).backward()
        Gd, dbags = mil_core.backward(pk, saved, lg.grad, need_params=True, need_bags=True, split_k=4)
        return {"logits": logits, "dbags": dbags, **{"grad:" + k: v for k, v in Gd.items()}}

    def bar(o):
        assert (o["logits"].cpu().double() - ref_logits).abs().max() < 3e-2 * max(1.0, ref_logits.abs().max().item())
        for k, r in ref_g.items():
            gk = o["grad:" + k].cpu().double()
            if alibi and "key_encoders" in k and k.endswith(".bias"):          # true gradient 0: small against the sibling value-bias gradient
                assert gk.norm() < 5e-2 * ref_g[k.replace("key_encoders", "value_encoders")].norm(), k
                continue
            floor = 0.0
            if alibi and ("query_encoders" in k or "key_encoders" in k):
                floor = 0.05 * ref_g[k.replace("query_encoders", "value_encoders").replace("key_encoders", "value_encoders")].norm().item()
            rel = ((gk - r).norm() / max(r.norm().item(), floor, 1e-12)).item()
            assert rel < ((5e-2 if k.endswith("bias_scale") else 2e-2) if alibi else 5e-2), (k, rel)

    return run, lambda: run(*big), bar


@pytest.mark.parametrize("alibi", [False, True])
def test_mil_vit_train_forward_backward(gpu, monkeypatch, alibi):
    """amds_mil_vit_train_forward (saved arena poisoned) + amds_mil_vit_train_backward (workspace, flat gradient buffer and dbp poisoned)."""
    _check_case(monkeypatch, *_train_case(gpu, alibi))


@pytest.mark.parametrize("alibi", [False, True])
def test_mil_vit_train_forward_backward_with_dropout(gpu, monkeypatch, alibi):
    """The same two calls with every dropout site live (p = 0.25, one seed): the arena and workspace regions that exist only when p > 0.  No reference here (the
    masked step's parity is tests/test_gpu_mil_seam.py's): the bar is the contract itself -- bit-identical, finite, bands intact, the small step's bits after a big one."""
    from stamp_amd.mil import VisionTransformer
    torch.manual_seed(11)
    Fd, Cn = 256, 2
    model = VisionTransformer(dim_output=Cn, dim_input=Fd, dim_model=256, n_layers=2, n_heads=4, dim_feedforward=256, dropout=0.25, use_alibi=alibi)
    _perturb(model)
    dsd = {k: v.detach().to(gpu, torch.float32) for k, v in model.state_dict().items()}
    pk = mil_core.PackedVit(model.dims, lambda n: dsd[n], torch.bfloat16, train=True)
    g = torch.Generator().manual_seed(12)
    mk = lambda Bb, Tn: (torch.randn(Bb, Tn, Fd, generator=g).half().to(gpu), (torch.rand(Bb, Tn, 2, generator=g) * 3000).to(gpu), torch.randn(Bb, Cn, generator=g).to(gpu))  # noqa: E731
    small, big = mk(3, 150), mk(4, 400)

    def run(b, c, dl):
        logits, saved = mil_core.forward_train(pk, b, c if alibi else None, training=True, seed=1234)
        Gd, dbags = mil_core.backward(pk, saved, dl, need_params=True, need_bags=True, split_k=4)
        return {"logits": logits, "dbags": dbags, **{"grad:" + k: v for k, v in Gd.items()}}

    _check_case(monkeypatch, lambda: run(*small), lambda: run(*big), lambda o: None)
    assert not torch.equal(run(*small)["logits"], mil_core.forward_train(pk, small[0], small[1] if alibi else None, training=False)[0])       # the masks were live


@pytest.mark.parametrize("tag,alibi", [("plain", False), ("alibi", True)])
def test_mil_vit_gradcam(gpu, monkeypatch, tag, alibi):
    """amds_mil_vit_gradcam behind its eval-mode training forward, on the reference's fixture (test_gpu_heatmaps.py: 0.1 relative L2 on cam_raw)."""
    from stamp_amd import heatmaps
    from test_gpu_heatmaps import _load, _rel
    z, model = _load(tag, alibi, gpu)
    feats, cu = (torch.from_numpy(z[k]).to(gpu) for k in ("feats", "coords_um"))
    ref_raw = torch.from_numpy(z["cam_raw"])
    g = torch.Generator().manual_seed(3)
    bigf, bigc = torch.randn(500, feats.shape[1], generator=g).to(gpu), (torch.rand(500, 2, generator=g) * 20000).to(gpu)

    def run(f=feats, c=cu):
        return {"cam_raw": heatmaps.gradcam(model, f, c, raw=True, method="fused")}

    def bar(o):
        assert max([_rel(o["cam_raw"], ref_raw)] + [_rel(o["cam_raw"][:, c], ref_raw[:, c]) for c in range(ref_raw.shape[1])]) < 0.1

    _check_case(monkeypatch, run, lambda: run(bigf, bigc), bar)
    assert model.fp16_overflow_events == 0          # nothing above went through the Python re-run on bf16


# ---- TransMIL -------------------------------------------------------------------------------------------------------------------------------
def test_transmil_forward(gpu, monkeypatch):
    """amds_transmil_forward on the reference's 50-tile fixture (test_gpu_mil.py: rtol = atol = 2e-3)."""
    from stamp_amd.mil import TransMIL
    z = np.load(GOLD / "transmil_t50.npz")
    dim_out, dim_in, dim_h = (int(v) for v in z["hparams"])
    model = TransMIL(dim_output=dim_out, dim_input=dim_in, dim_hidden=dim_h).eval()
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}, strict=True)
    model = model.to(gpu)
    bags = torch.from_numpy(z["bags"]).to(gpu)
    big = torch.randn(3, 300, dim_in, generator=torch.Generator().manual_seed(4)).to(gpu)

    def run(b=bags):
        with torch.no_grad():
            return {"logits": model(b)}

    _check_case(monkeypatch, run, lambda: run(big), lambda o: np.testing.assert_allclose(o["logits"].cpu().numpy(), z["logits"], rtol=2e-3, atol=2e-3))


def test_transmil_forward_ragged(gpu, monkeypatch):
    """amds_transmil_forward_ragged: 1 / 50 / 300 tiles = three different (pad, np) at 32 landmarks, each row against the fp64 oracle of its bag alone
    (test_gpu_transmil_ragged.py: 2e-3 of the logit scale)."""
    from test_gpu_transmil_ragged import _model, _oracle_rows
    m = _model(24, 64)
    g = torch.Generator().manual_seed(1)
    bags = [(torch.randn(t, 24, generator=g) * 16).round().clamp(-63, 63) / 16 for t in (1, 50, 300)]
    bigs = [torch.randn(t, 24, generator=g) for t in (700, 300, 65, 2)]
    ref = _oracle_rows(m, bags)
    m = m.to(gpu)

    def run(bs=bags):
        with torch.no_grad():
            return {"logits": m.forward_ragged([b.to(gpu) for b in bs])}

    def bar(o):
        err = (o["logits"].double().cpu() - ref).abs()
        for i in range(len(bags)):
            assert err[i].max().item() < 2e-3 * max(1.0, ref[i].abs().max().item()), (i, err[i])

    _check_case(monkeypatch, run, lambda: run(bigs), bar)


def test_transmil_train_forward_backward(gpu, monkeypatch):
    """amds_transmil_train_forward / _backward through the module's autograd function at (2, 50, 96, 64) (test_gpu_transmil_train.py: logits 2e-3, every
    gradient 1e-4 relative L2 against fp64 autograd through the oracle)."""
    from test_gpu_transmil_train import _oracle, _rel, _setup
    model, bags, targets = _setup(2, 50, 96, 64, 2, seed=50)
    _, ref_logits, ref_g, ref_dx = _oracle(model, bags, targets)
    model = model.to(gpu).eval()
    big = torch.randn(3, 300, 96, generator=torch.Generator().manual_seed(6)).to(gpu)

    def run(b=bags.to(gpu), tg=targets.to(gpu)):
        for p in model.parameters():
            p.grad = None
        x = b.clone().requires_grad_(True)
        logits = model(x)
        tgt = tg if tg.shape[0] == logits.shape[0] else torch.nn.functional.one_hot(torch.arange(logits.shape[0], device=gpu) % 2, 2).float()
        torch.nn.functional.cross_entropy(logits, tgt).backward()
        return {"logits": logits.detach(), "dbags": x.grad, **{"grad:" + n: p.grad for n, p in model.named_parameters()}}

    def bar(o):
        assert (o["logits"].cpu().double() - ref_logits).abs().max() < 2e-3 * max(1.0, ref_logits.abs().max().item())
        assert _rel(o["dbags"].cpu(), ref_dx) < 1e-4
        for n, r in ref_g.items():
            assert _rel(o["grad:" + n].cpu(), r) < 1e-4, n

    _check_case(monkeypatch, run, lambda: run(big), bar)


def test_nystrom_attn_fwd_bwd(gpu, monkeypatch):
    """amds_nystrom_attn_fwd / _bwd on the fixture's batch of two bags (one pseudo-inverse scale for the batch, like the reference).  Forward against the
    reference's fixture of the block (nys_x -> nys_out, the bar of the TransMIL fixture it is part of: rtol = atol = 2e-3), backward against fp64 autograd
    through the oracle's block (the TransMIL backward's bar: 1e-4 relative L2)."""
    from oracle import transmil as ot
    from stamp_amd import transmil_core as tc
    z = np.load(GOLD / "transmil_t50.npz")
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    Cd = int(z["hparams"][2])
    y0, out_ref = torch.from_numpy(z["nys_x"]), z["nys_out"]
    dx0 = torch.randn(*y0.shape, generator=torch.Generator().manual_seed(8))
    pd = {k: v.double().requires_grad_(k.startswith("layer1.attn.")) for k, v in sd.items()}
    yd = y0.double().requires_grad_(True)
    ot.nystrom_attention(yd, pd, "layer1.attn.", heads=8, landmarks=Cd // 2).backward(dx0.double())
    P = tc._Nys(lambda k: sd[k].to(gpu).float().contiguous(), "layer1")
    ybig = torch.randn(2, 300, Cd, generator=torch.Generator().manual_seed(9))

    def run(y=y0, dx=dx0):
        y, dx = y.to(gpu).contiguous(), dx.to(gpu).contiguous()
        x_res = torch.zeros_like(y)
        S = tc.nystrom_forward(y, P, x_res, 0.0, 0, 1)
        dy, Gd = tc.nystrom_backward(S, P, dx)
        return {"out": x_res, "dy": dy, **{"grad:" + k: v for k, v in Gd.items()}}

    def bar(o):
        from test_gpu_transmil_train import _rel
        np.testing.assert_allclose(o["out"].cpu().numpy(), out_ref, rtol=2e-3, atol=2e-3)
        assert _rel(o["dy"].cpu(), yd.grad) < 1e-4
        for k in ("attn.to_qkv.weight", "attn.to_out.0.weight", "attn.to_out.0.bias", "attn.res_conv.weight"):
            assert _rel(o["grad:" + k].cpu(), pd["layer1." + k].grad.reshape(o["grad:" + k].shape)) < 1e-4, k

    _check_case(monkeypatch, run, lambda: run(ybig, torch.ones_like(ybig)), bar)


def test_transmil_train_and_nystrom_with_dropout(gpu, monkeypatch):
    """amds_transmil_train_forward / _backward in train mode (Dropout(0.1) behind both to_out, one seed) and amds_nystrom_attn_fwd / _bwd at p = 0.1: the contract alone
    is the bar (bit-identical, finite, bands intact, same bits after a bigger call); parity with the masks is tests/test_gpu_transmil_train.py's."""
    from stamp_amd import transmil_core as tc
    from test_gpu_transmil_train import _setup
    model, bags, targets = _setup(2, 50, 96, 64, 2, seed=51)
    model = model.to(gpu).train()
    big = torch.randn(3, 300, 96, generator=torch.Generator().manual_seed(6)).to(gpu)

    def run(b=bags.to(gpu)):
        torch.manual_seed(99)                                  # the module draws its dropout seed from torch's CPU generator
        for p in model.parameters():
            p.grad = None
        x = b.clone().requires_grad_(True)
        logits = model(x)
        tgt = torch.nn.functional.one_hot(torch.arange(logits.shape[0], device=gpu) % 2, 2).float()
        torch.nn.functional.cross_entropy(logits, tgt).backward()
        return {"logits": logits.detach(), "dbags": x.grad, **{"grad:" + n: p.grad for n, p in model.named_parameters()}}

    _check_case(monkeypatch, run, lambda: run(big), lambda o: None)
    sd = {k: v.detach().float().contiguous() for k, v in model.state_dict().items()}
    P = tc._Nys(lambda k: sd[k], "layer1")
    g = torch.Generator().manual_seed(7)
    y0, dx0, ybig = torch.randn(2, 70, 64, generator=g).to(gpu), torch.randn(2, 70, 64, generator=g).to(gpu), torch.randn(2, 300, 64, generator=g).to(gpu)

    def run_nys(y=y0, dx=dx0):
        x_res = torch.zeros_like(y)
        S = tc.nystrom_forward(y, P, x_res, 0.1, 4242, 1)
        dy, Gd = tc.nystrom_backward(S, P, dx)
        return {"out": x_res, "dy": dy, **{"grad:" + k: v for k, v in Gd.items()}}

    _check_case(monkeypatch, run_nys, lambda: run_nys(ybig, torch.ones_like(ybig)), lambda o: None)


# ---- the other heads and stages that run on ops.scratch --------------------------------------------------------------------------------------
def test_barspoon_forward(gpu, monkeypatch):
    """amds_barspoon_forward on the reference's fixture "a" (test_gpu_barspoon.py: 5e-3 of the logit scale)."""
    from stamp_amd.barspoon import EncDecTransformer
    z, tag = np.load(GOLD / "barspoon.npz"), "a"
    sd = {k[len(tag) + 3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{tag}_w:")}
    hp = [int(v) for v in z[f"{tag}_hparams"]]
    targets = {str(t): int(n) for t, n in zip(z[f"{tag}_targets"], z[f"{tag}_nout"])}
    model = EncDecTransformer(z[f"{tag}_x"].shape[2], targets, d_model=hp[0], num_encoder_heads=hp[1], num_decoder_heads=hp[2], num_encoder_layers=hp[3],
                              num_decoder_layers=hp[4], dim_feedforward=hp[5], positional_encoding=bool(hp[6])).eval()
    model.load_state_dict(sd, strict=True)
    x, pos = torch.from_numpy(z[f"{tag}_x"]).to(gpu), torch.from_numpy(z[f"{tag}_pos"]).to(gpu)
    g = torch.Generator().manual_seed(10)
    bx, bpos = torch.randn(x.shape[0] + 1, 4 * x.shape[1] + 3, x.shape[2], generator=g).to(gpu), None
    bpos = (torch.rand(bx.shape[0], bx.shape[1], 2, generator=g) * 50000).to(gpu)

    def run(a=x, p=pos):
        with torch.no_grad():
            return dict(model(a, p))

    def bar(o):
        for j, t in enumerate(targets):
            ref = z[f"{tag}_logits_{j}"]
            assert np.abs(o[t].cpu().numpy() - ref).max() < 5e-3 * max(1.0, np.abs(ref).max()), t

    _check_case(monkeypatch, run, lambda: run(bx, bpos), bar)


def test_ticon_tile_forward(gpu, monkeypatch):
    """amds_ticon_tile_forward on the reference's fixture (test_gpu_seams.py: rtol = atol = 2e-5)."""
    from stamp_amd.ticon import HipTiconTile
    z = np.load(GOLD / "ticon.npz")
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    m = HipTiconTile(sd, key="hoptimus1", device=gpu)
    emb = torch.from_numpy(z["emb_hoptimus1"]).to(gpu)
    big = torch.randn(40 * emb.shape[0] + 1, emb.shape[1], generator=torch.Generator().manual_seed(11)).to(gpu)
    _check_case(monkeypatch, lambda e=emb: {"out": m(e)}, lambda: m(big),
                lambda o: np.testing.assert_allclose(o["out"].cpu().numpy(), z["out_hoptimus1"], rtol=2e-5, atol=2e-5))


def test_resize_center_crop(gpu, monkeypatch):
    """amds_tile_resize_crop_u8 at (100 -> 257, crop 224): Pillow's bicubic resize + torchvision's crop, bit for bit (test_gpu_tiling.py)."""
    from PIL import Image
    from stamp_amd.tiling import resize_center_crop
    S, resized, crop = 100, 257, 224
    rng = np.random.default_rng(S + resized)
    tiles = rng.integers(0, 256, (3, S, S, 3), dtype=np.uint8)
    tiles[1] = (np.indices((S, S)).sum(0) % 256)[..., None].astype(np.uint8)
    t_dev = torch.from_numpy(tiles).to(gpu)
    big = torch.from_numpy(rng.integers(0, 256, (9, S, S, 3), dtype=np.uint8)).to(gpu)
    c0 = int(round((resized - crop) / 2.0))

    def bar(o):
        for i in range(3):
            ref = np.asarray(Image.fromarray(tiles[i], "RGB").resize((resized, resized), Image.BICUBIC))[c0:c0 + crop, c0:c0 + crop]
            assert np.array_equal(o["out"][i].cpu().numpy(), ref), i

    _check_case(monkeypatch, lambda t=t_dev: {"out": resize_center_crop(t, resized, crop)}, lambda: resize_center_crop(big, resized, crop), bar)


def test_proj_head_l2norm(gpu, monkeypatch):
    """amds_proj_head_l2norm on the reference's KEEP head fixture (test_gpu_seams.py: rtol 2e-5, atol 2e-6), called on ops.scratch as the extractor does."""
    z = np.load(GOLD / "keep_head.npz")
    hsd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    feats = torch.from_numpy(z["feats"]).to(gpu)
    w = [hsd[f"visual_head.{k}"].to(gpu).contiguous() for k in ("0.weight", "0.bias", "2.weight", "2.bias")]
    lib = _lib.lib()
    big = torch.randn(900, 128, generator=torch.Generator().manual_seed(12)).to(gpu)

    def run(x=feats):
        rows = x.shape[0]
        out, ho = G.guarded((rows, 96), torch.float32, gpu, pattern=0xFF, name="out")
        nb = lib.amds_proj_head_l2norm_workspace_bytes(rows, 128, 96)
        ws = ops.scratch("keep_head", gpu, nb)
        _lib.check(lib.amds_proj_head_l2norm(x.data_ptr(), ops._DT[x.dtype], *[t.data_ptr() for t in w], out.data_ptr(), rows, 128, 96, ws.data_ptr(), ws.numel(),
                                             ops._stream()), "head")
        torch.cuda.synchronize()
        ho.assert_bands_intact()
        return {"out": out}

    _check_case(monkeypatch, run, lambda: run(big), lambda o: np.testing.assert_allclose(o["out"].cpu().numpy(), z["out"], rtol=2e-5, atol=2e-6))


def _gap_case(gpu, F, L, D, seed):
    from oracle.gated_attention import KEYS
    from test_gpu_seams import _gap_sd
    sd, g = _gap_sd(F, L, D, seed=seed)
    return sd, g, {k: sd[v].to(gpu).contiguous() for k, v in KEYS.items()}


def test_gated_attn_pool(gpu, monkeypatch):
    """amds_gated_attn_pool at 65 rows (one past a 64-row unit) against the oracle (test_gpu_seams.py: rtol 1e-4, atol 1e-4 / 1e-5)."""
    from oracle.gated_attention import gated_attention_pool
    sd, g, w = _gap_case(gpu, 768, 512, 256, seed=65)
    x = torch.randn(65, 768, generator=g)
    ref = gated_attention_pool(x, sd)
    xd, big = x.to(gpu), torch.randn(3000, 768, generator=g).to(gpu)

    def run(a=xd):
        out, araw = ops.gated_attn_pool(a, w, return_attn=True)
        return {"out": out, "attn_raw": araw}

    def bar(o):
        np.testing.assert_allclose(o["attn_raw"].cpu().numpy(), ref["attention_raw"].reshape(-1).numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(o["out"].cpu().numpy(), ref["WSI_feature"].reshape(-1).numpy(), rtol=1e-4, atol=1e-5)

    _check_case(monkeypatch, run, lambda: run(big), bar, short=False)     # (the wrapper passes the size it asked for, not the tensor's: one byte short goes through the C ABI)
    lib = _lib.lib()
    need = lib.amds_gated_attn_pool_workspace_bytes(65, 768, 512, 256)
    ws, h = G.guarded((need,), torch.uint8, gpu, pattern=0xFF, name="ws")
    out = torch.empty(768, device=gpu)
    rc = lib.amds_gated_attn_pool(xd.data_ptr(), C.byref(ops._gap_weights(w)), out.data_ptr(), None, 65, 768, 512, 256, ws.data_ptr(), need - 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool((ws == 0xFF).all())
    h.assert_bands_intact()


@pytest.mark.parametrize("mode", ["slab", "split"])
def test_gated_attn_pool_batched(gpu, monkeypatch, mode):
    """amds_gated_attn_pool_batched, ragged bags around the 16- / 64-row unit edges, both decompositions (test_gpu_seams.py: rtol 1e-4, atol 1e-4 / 3e-5)."""
    from oracle.gated_attention import gated_attention_pool
    sd, g, w = _gap_case(gpu, 384, 256, 256, seed=384)
    lens = [1, 64, 63, 65, 17, 300, 16]
    xs = [torch.randn(n, 384, generator=g) for n in lens]
    refs = [gated_attention_pool(x, sd) for x in xs]
    xcat = torch.cat(xs).to(gpu)
    blens = [700, 129, 1024, 5, 640]
    bcat = torch.randn(sum(blens), 384, generator=g).to(gpu)

    def run(a=xcat, ls=lens):
        out, araw = ops.gated_attn_pool_batched(a, ls, w, return_attn=True, mode=mode)
        return {"out": out, "attn_raw": araw}

    def bar(o):
        at = 0
        for i, (n, ref) in enumerate(zip(lens, refs)):
            np.testing.assert_allclose(o["attn_raw"][at:at + n].cpu().numpy(), ref["attention_raw"].reshape(-1).numpy(), rtol=1e-4, atol=1e-4, err_msg=f"bag {i}")
            np.testing.assert_allclose(o["out"][i].cpu().numpy(), ref["WSI_feature"].reshape(-1).numpy(), rtol=1e-4, atol=3e-5, err_msg=f"bag {i}")
            at += n

    _check_case(monkeypatch, run, lambda: run(bcat, blens), bar, short=False)
    lib = _lib.lib()
    need = lib.amds_gated_attn_pool_batched_workspace_bytes(sum(lens), len(lens), 384, 256, 256)
    ws, h = G.guarded((need,), torch.uint8, gpu, pattern=0xFF, name="ws")
    out = torch.empty(len(lens), 384, device=gpu)
    offs = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0).to(gpu)
    rc = lib.amds_gated_attn_pool_batched(xcat.data_ptr(), offs.data_ptr(), len(lens), sum(lens), C.byref(ops._gap_weights(w)), out.data_ptr(), None, 384, 256, 256,
                                          ops.GAP_MODES[mode], ws.data_ptr(), need - 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool((ws == 0xFF).all())
    h.assert_bands_intact()


# ---- the tile encoders keep their workspace on the model object ------------------------------------------------------------------------------
def _encoder_contract(gpu, model, need_of, forward, big_chunk, bar, diag_zero=None):
    """`model._ws` is the workspace the wrapper hands the library: the test puts a guarded buffer of exactly the requested size there."""
    def call(pattern, chunk=None, reuse=None):
        if reuse is None:
            ws, h = G.guarded((need_of(model.chunk),), torch.uint8, gpu, band_bytes=G.FLAT_BAND_BYTES, pattern=pattern, name="model._ws")
        else:
            ws, h = reuse
        model._ws = ws[:need_of(model.chunk)]
        if hasattr(model, "_ws_chunk"):
            model._ws_chunk = None          # the range counters are the caller's to zero (amds_vit_workspace_diag_offset): the wrapper does, for a new buffer
        outs = forward()
        torch.cuda.synchronize()
        return G.Result(outs, [h])

    alone = G.run_contract(call)
    bar(alone)
    small_chunk = model.chunk
    ws, h = G.guarded((need_of(big_chunk),), torch.uint8, gpu, band_bytes=G.FLAT_BAND_BYTES, pattern=0xFF, name="model._ws (big)")
    model.chunk, model._ws = big_chunk, ws
    if hasattr(model, "_ws_chunk"):
        model._ws_chunk = None
    forward(big=True)
    model.chunk = small_chunk
    after = call(0xFF, reuse=(ws, h)).outputs
    h.assert_bands_intact()
    for k, v in alone.items():
        assert torch.equal(after[k], v), f"{k}: the small call's result depends on what ran before it on the same workspace"
    model._ws = None


def test_vit_forward_tokens(gpu):
    """amds_vit_forward_tokens on `test_tiny` (test_gpu_vit.py: 2e-3 relative L2 against the oracle, fp16)."""
    from oracle.vit_tile_encoder import extract_features
    from stamp_amd.vit import PRESETS, HipViT, random_vit_state_dict
    from test_gpu_vit import _rel
    cfg = PRESETS["test_tiny"]
    sd = random_vit_state_dict(cfg, seed=1, init="moderate")
    tiles = torch.randint(0, 256, (5, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    ref_f, ref_t = extract_features(tiles, sd, cfg, return_tokens=True)
    model = HipViT(cfg, sd, device=gpu, act_dtype=torch.float16, chunk=2)
    td = tiles.to(gpu)
    bigt = torch.randint(0, 256, (7, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(gpu)
    lib = _lib.lib()

    def forward(big=False):
        f, t = model(bigt if big else td, return_tokens=True)
        return {"feats": f, "tokens": t, "feats_default": model(bigt if big else td)}

    def bar(o):
        assert _rel(o["tokens"].cpu(), ref_t) < 2e-3 and _rel(o["feats"].cpu().float(), ref_f.float()) < 2e-3
        assert _rel(o["feats_default"].cpu().float(), ref_f.float()) < 2e-3

    _encoder_contract(gpu, model, lambda chunk: lib.amds_vit_workspace_bytes(C.byref(model._cfg_c), chunk), forward, 7, bar)
    need = lib.amds_vit_workspace_bytes(C.byref(model._cfg_c), 2)
    ws, h = G.guarded((need,), torch.uint8, gpu, pattern=0xFF, name="ws")
    feats = torch.empty(5, cfg.dim, dtype=torch.float16, device=gpu)
    rc = lib.amds_vit_forward_tokens(C.byref(model._cfg_c), C.byref(model._w_c), td.data_ptr(), feats.data_ptr(), None, 5, 2, ws.data_ptr(), need - 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool((ws == 0xFF).all())
    h.assert_bands_intact()


def test_swin_forward(gpu):
    """amds_swin_forward on `test_swin_tiny` against the reference's golden features (test_gpu_swin.py: 1e-3 relative L2, 3e-3 max / max)."""
    from stamp_amd.swin import SWIN_PRESETS, HipSwin, random_swin_state_dict
    from test_gpu_swin import _rel
    z = np.load(GOLD / "ctranspath_tiny.npz")
    cfg = SWIN_PRESETS["test_swin_tiny"]
    model = HipSwin(cfg, random_swin_state_dict(cfg, int(z["seed"])), device=gpu, chunk=3)
    tiles, ref = torch.from_numpy(z["tiles"]).to(gpu), torch.from_numpy(z["feats"])
    bigt = torch.randint(0, 256, (8, cfg.img, cfg.img, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(gpu)
    lib = _lib.lib()

    def forward(big=False):
        f16, f32 = model(bigt if big else tiles, return_f32=True)
        return {"feats_f16": f16, "feats_f32": f32}

    def bar(o):
        f32 = o["feats_f32"].cpu()
        assert _rel(f32, ref) < 1e-3 and ((f32 - ref).abs().max() / ref.abs().max()).item() < 3e-3
        assert torch.equal(o["feats_f16"].cpu(), f32.half())

    _encoder_contract(gpu, model, lambda chunk: lib.amds_swin_workspace_bytes(C.byref(model._cfg_c), chunk), forward, 8, bar)
    need = lib.amds_swin_workspace_bytes(C.byref(model._cfg_c), 3)
    ws, h = G.guarded((need,), torch.uint8, gpu, pattern=0xFF, name="ws")
    feats = torch.empty(tiles.shape[0], cfg.out_dim, dtype=torch.float16, device=gpu)
    rc = lib.amds_swin_forward(C.byref(model._cfg_c), C.byref(model._w_c), tiles.data_ptr(), feats.data_ptr(), None, tiles.shape[0], 3, ws.data_ptr(), need - 1,
                               ops._stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool((ws == 0xFF).all())
    h.assert_bands_intact()
