"""TICON slide mode on the GPU: amds_attention_distbias alone against fp64, `HipTiconSlide` against the reference's float64 run
(tests/golden/ticon_slide.npz), bit-level invariants, the C-ABI contract of amds_ticon_slide_forward (tests/guarded.py), the file helper and the
fp16 range guard."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import guarded as G
from chains.ticon_slide import MODELS, distbias_attention, load_fixture
from stamp_amd import _lib, h5io, ops
from stamp_amd.encoder import STAMP_FORMAT_VERSION
from stamp_amd.ticon import HipTiconSlide, HipTiconTile, alibi_slopes, contextualise_features

pytestmark = pytest.mark.gpu

CASES = [(tag, name) for tag in MODELS for name in ("b2_hoptimus1", "b2_conchv15", "n70", "n1")]
_MODELS: dict = {}


def _model(gpu, tag, key, dtype=torch.float16, **kw):
    k = (tag, key, dtype, tuple(sorted(kw.items())))
    if k not in _MODELS:
        m = load_fixture()[tag]
        _MODELS[k] = HipTiconSlide(m["sd"], key=key, device=gpu, dtype=dtype, heads=m["heads"], **kw)
    return _MODELS[k]


# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------------------
def _kernel_case(B, T, H, dt, coord_mode="grid"):
    g = torch.Generator().manual_seed(B * 100000 + T * 10 + H)
    qkv = torch.randn(B * T, 3 * H * 64, generator=g).to(dt)
    coords = torch.randint(0, 40, (B, T, 2), generator=g).float()
    if coord_mode == "equal":
        coords = coords[:, :1].expand(B, T, 2).contiguous()
    elif coord_mode == "far":
        coords = coords * 1000.0
    slopes = torch.tensor(alibi_slopes(H), dtype=torch.float32)
    q, k, v = qkv.double().reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    ref = distbias_attention(q, k, v, coords.double(), slopes, 0.125).transpose(1, 2).reshape(B * T, H * 64)
    return qkv, coords, slopes, ref, (q, k, v)


def _distbias(gpu, qkv, coords, slopes, B, T, H):
    q, c, s = qkv.to(gpu), coords.to(gpu), slopes.to(gpu)
    out = torch.empty(B * T, H * 64, dtype=qkv.dtype, device=gpu)
    _lib.check(_lib.lib().amds_attention_distbias(q.data_ptr(), c.data_ptr(), s.data_ptr(), out.data_ptr(), B, T, H, ops._DT[qkv.dtype], ops._stream()), "attention_distbias")
    return out


def _bar(out, ref, dt):
    eps = 2 ** -7 if dt == torch.bfloat16 else 2 ** -10
    assert bool(torch.isfinite(out).all())
    err = (out.cpu().double() - ref).abs().max().item()
    bar = 4 * eps * max(1.0, ref.abs().max().item())
    print(f"max abs err {err:.3e} (bar {bar:.3e})")
    assert err < bar, (err, bar)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,T,H", [(1, 1, 1), (2, 7, 2), (1, 64, 1), (1, 65, 1), (2, 129, 3), (1, 200, 6), (1, 1025, 24)])
def test_distbias_attention_vs_fp64(gpu, dt, B, T, H):
    """One key, a partial first tile, exactly one tile, one tile + 1, a 128-query block + 1, a non-power-of-two head count, the MIL training length;
    integer grid coordinates in [0, 40).  Bar: that of test_attention_backward_vs_autograd's forward."""
    qkv, coords, slopes, ref, _ = _kernel_case(B, T, H, dt)
    _bar(_distbias(gpu, qkv, coords, slopes, B, T, H), ref, dt)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_distbias_attention_zero_bias_is_plain_attention(gpu, dt):
    """All coordinates equal: the bias is 0 and the result meets the same bar against plain softmax attention."""
    B, T, H = 1, 200, 6
    qkv, coords, slopes, ref, (q, k, v) = _kernel_case(B, T, H, dt, "equal")
    plain = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(B * T, H * 64)
    out = _distbias(gpu, qkv, coords, slopes, B, T, H)
    _bar(out, plain, dt)
    _bar(out, ref, dt)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_distbias_attention_far_keys_underflow(gpu, dt):
    """Coordinates x 1000: the weights of far keys underflow; the result is finite and within the bar."""
    B, T, H = 1, 200, 6
    qkv, coords, slopes, ref, _ = _kernel_case(B, T, H, dt, "far")
    _bar(_distbias(gpu, qkv, coords, slopes, B, T, H), ref, dt)


def test_distbias_attention_bad_arguments(gpu):
    lib = _lib.lib()
    t = torch.zeros(64 * 3 * 64, dtype=torch.float16, device=gpu)
    c = torch.zeros(64, 2, device=gpu)
    s = torch.zeros(4, device=gpu)
    o = torch.full((64, 64), 7.0, dtype=torch.float16, device=gpu)
    st = ops._stream()
    assert lib.amds_attention_distbias(None, c.data_ptr(), s.data_ptr(), o.data_ptr(), 1, 64, 1, 0, st) == -1
    assert lib.amds_attention_distbias(t.data_ptr(), None, s.data_ptr(), o.data_ptr(), 1, 64, 1, 0, st) == -1
    assert lib.amds_attention_distbias(t.data_ptr(), c.data_ptr(), None, o.data_ptr(), 1, 64, 1, 0, st) == -1
    assert lib.amds_attention_distbias(t.data_ptr(), c.data_ptr(), s.data_ptr(), o.data_ptr(), 1, 0, 1, 0, st) == -1
    assert lib.amds_attention_distbias(t.data_ptr(), c.data_ptr(), s.data_ptr(), o.data_ptr(), 1, 64, 1, 2, st) == -1          # fp32 operands
    assert lib.amds_attention_distbias(t.data_ptr(), c.data_ptr(), s.data_ptr(), o.data_ptr(), 1, 1 << 22, 8, 0, st) == -1     # past the 2 GB span
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------
def _rel(got, want):
    got, want = got.double().cpu().reshape(-1, want.shape[-1]), want.reshape(-1, want.shape[-1])
    whole = ((got - want).norm() / want.norm()).item()
    rows = ((got - want).norm(dim=1) / want.norm(dim=1)).max().item()
    return whole, rows


@pytest.mark.parametrize("tag,name", CASES)
def test_model_fp16_vs_reference_fp64(gpu, tag, name):
    """fp16 operands against the reference's float64 run: whole tensor <= 1e-3 relative L2 (the bar for stored features; rounding every Linear's
    operands to fp16 costs 2.5e-4 in emulation), worst row <= 2e-3 (emulated 3.2e-4)."""
    c = load_fixture()[tag]["cases"][name]
    out = _model(gpu, tag, c["key"])(c["emb"].to(gpu), c["coords"].to(gpu))
    assert out.shape == c["out64"].shape and out.dtype == torch.float32
    whole, rows = _rel(out, c["out64"])
    print(f"{tag}/{name} fp16: whole {whole:.3e}, worst row {rows:.3e}")
    assert whole <= 1e-3 and rows <= 2e-3, (whole, rows)


@pytest.mark.parametrize("tag,name", CASES)
def test_model_bf16_vs_reference_fp64(gpu, tag, name):
    """bf16 operands: <= 1e-2 whole tensor, 1.5e-2 worst row (emulated 2.5e-3 and 3.6e-3)."""
    c = load_fixture()[tag]["cases"][name]
    out = _model(gpu, tag, c["key"], torch.bfloat16)(c["emb"].to(gpu), c["coords"].to(gpu))
    whole, rows = _rel(out, c["out64"])
    print(f"{tag}/{name} bf16: whole {whole:.3e}, worst row {rows:.3e}")
    assert whole <= 1e-2 and rows <= 1.5e-2, (whole, rows)


def test_model_fp16_inputs_and_outputs(gpu):
    """fp16 embeddings give the bits of their fp32 copies (they are fp16 numbers); out_dtype=float16 is the rounded fp32 result."""
    c = load_fixture()["a"]["cases"]["n70"]
    emb, coords = c["emb"].to(gpu), c["coords"].to(gpu)
    want = _model(gpu, "a", c["key"])(emb, coords)
    assert torch.equal(_model(gpu, "a", c["key"])(emb.half(), coords), want)
    got16 = _model(gpu, "a", c["key"], out_dtype=torch.float16)(emb, coords)
    assert got16.dtype == torch.float16 and torch.equal(got16, want.half())


def test_one_tile_matches_tile_mode(gpu):
    fx = load_fixture()["b"]
    c = fx["cases"]["n1"]
    emb = c["emb"].to(gpu)
    slide = _model(gpu, "b", c["key"])(emb, c["coords"].to(gpu))
    tile = HipTiconTile(fx["sd"], key=c["key"], device=gpu)(emb)
    rel = ((slide - tile).norm() / tile.norm()).item()
    print(f"N = 1 against HipTiconTile: {rel:.3e}")
    assert rel <= 1e-3


@pytest.mark.parametrize("tag", MODELS)
def test_bit_level_invariants(gpu, tag):
    """Two identical calls give the same bits; slide b of a B = 2 call gives the bits of its own B = 1 call; [N, in_dim] is [1, N, in_dim]."""
    fx = load_fixture()[tag]
    c = fx["cases"][f"b2_{fx['keys'][0]}"]
    m = _model(gpu, tag, c["key"])
    emb, coords = c["emb"].to(gpu), c["coords"].to(gpu)
    both = m(emb, coords)
    assert torch.equal(m(emb, coords), both)
    for b in range(2):
        alone = m(emb[b:b + 1], coords[b:b + 1])
        assert torch.equal(alone[0], both[b]), f"slide {b} depends on its neighbour in the batch"
        flat = m(emb[b], coords[b])
        assert flat.shape == (150, fx["dim"]) and torch.equal(flat, alone[0])


# ---- the C-ABI contract -----------------------------------------------------------------------------------------------------------------------------
def _hooked(monkeypatch, run, **kw):
    def call(pattern):
        with G.scratch_hook(monkeypatch, pattern, **kw) as log:
            outs = run()
            torch.cuda.synchronize()
        assert any(t != "alloc" for t, _ in log.requests), "the call did not take its workspace from ops.scratch"
        return G.Result(outs, log.handles)
    return call


@pytest.mark.parametrize("tag", MODELS)
def test_slide_forward_workspace_contract(gpu, monkeypatch, tag):
    """Guard bands around `out` and the workspace, the workspace pre-filled with 0x00 and with 0xFF (NaN) bytes: same bits, finite, bands intact, and the
    0x00 run meets the model bar.  Then the small call on the leftovers of a bigger one, and ws_bytes one byte short: an error, nothing written."""
    fx = load_fixture()[tag]
    c = fx["cases"]["n70"]
    m = _model(gpu, tag, c["key"])
    emb, coords = c["emb"].to(gpu), c["coords"].to(gpu)
    run = lambda: {"out": m(emb, coords)}  # noqa: E731
    alone = G.run_contract(_hooked(monkeypatch, run))
    whole, rows = _rel(alone["out"], c["out64"])
    assert whole <= 1e-3 and rows <= 2e-3, (whole, rows)
    g = torch.Generator().manual_seed(5)
    big_e, big_c = torch.randn(2, 300, emb.shape[1], generator=g).to(gpu), torch.rand(2, 300, 2, generator=g).to(gpu) * 20
    with G.scratch_hook(monkeypatch, 0xFF, persistent=True) as log:
        m(big_e, big_c)
        after_big = run()["out"].clone()
        torch.cuda.synchronize()
    log.assert_bands_intact()
    sizes = log.bytes_for("ticon_slide")
    assert max(sizes) > min(sizes), "the big shape asked for no more workspace"
    assert torch.equal(after_big, alone["out"]), "the small call's result depends on what ran before it on the same workspace"
    with G.scratch_hook(monkeypatch, 0xFF, short_by=1) as log:
        with pytest.raises(RuntimeError, match="libamdstamp"):
            run()
        torch.cuda.synchronize()
    log.assert_bands_intact()
    for h in log.handles:
        assert bool((h.buf == 0xFF).all()), f"{h.name}: written although ws_bytes was one byte short"


def test_slide_forward_bad_arguments_launch_nothing(gpu):
    """Null pointers and bad shapes: an error code, and neither `out` nor the workspace is touched."""
    fx = load_fixture()["b"]
    c = fx["cases"]["n70"]
    m = _model(gpu, "b", c["key"])
    lib = _lib.lib()
    emb, coords = c["emb"].to(gpu).contiguous(), c["coords"].to(gpu).contiguous()
    N = emb.shape[0]
    need = lib.amds_ticon_slide_workspace_bytes(C.byref(m._cfg), 1, N)
    assert need > 0 and need % 256 == 0
    ws, hw = G.guarded((need,), torch.uint8, gpu, band_bytes=G.FLAT_BAND_BYTES, pattern=0xFF, name="ws")
    out, ho = G.guarded((N, fx["dim"]), torch.float32, gpu, pattern=0xFF, name="out")
    st = ops._stream()

    def call(cfg=m._cfg, w=m._w, e=emb.data_ptr(), edt=_lib.F32, co=coords.data_ptr(), o=out.data_ptr(), odt=_lib.F32, B=1, T=N, wsp=ws.data_ptr(), wsb=need):
        return lib.amds_ticon_slide_forward(C.byref(cfg) if cfg is not None else None, C.byref(w) if w is not None else None, e, edt, co, o, odt, B, T, wsp, wsb, st)

    for kw in ({"cfg": None}, {"w": None}, {"e": None}, {"co": None}, {"o": None}, {"wsp": None}):
        assert call(**kw) == -1, kw
    assert call(T=0) == -1 and call(T=-3) == -1 and call(B=-1) == -1 and call(B=70000) == -1
    assert call(edt=_lib.BF16) == -1 and call(odt=_lib.BF16) == -1
    assert call(wsb=need - 1) == -2
    assert call(wsp=ws.data_ptr() + 16, wsb=need) == -1                      # not 256-byte aligned
    assert call(T=1 << 24) == -1                                             # a slide's q | k | v rows past 2 GB
    for field, bad in (("heads", 5), ("heads", 1), ("dim", 98), ("hidden", 511), ("dtype", _lib.F32), ("in_dim", 0), ("depth", -1)):
        cfg = _lib.TiconSlideCfg(m._cfg.in_dim, m._cfg.dim, m._cfg.heads, m._cfg.hidden, m._cfg.depth, m._cfg.dtype)
        setattr(cfg, field, bad)
        assert call(cfg=cfg) == -1, (field, bad)
        assert lib.amds_ticon_slide_workspace_bytes(C.byref(cfg), 1, N) == 0
    w = _lib.TiconSlideWeights.from_buffer_copy(m._w)
    w.slopes = None
    assert call(w=w) == -1
    blocks = (_lib.TiconSlideBlock * m.depth)(*[_lib.TiconSlideBlock.from_buffer_copy(b) for b in m._blocks])
    blocks[m.depth - 1].fc2_w = None                                         # the LAST block: nothing may have been launched for the earlier ones
    w = _lib.TiconSlideWeights.from_buffer_copy(m._w)
    w.blocks_host = blocks
    assert call(w=w) == -1
    assert call(B=0) == 0                                                    # an empty batch is no error and no work
    torch.cuda.synchronize()
    hw.assert_bands_intact()
    ho.assert_bands_intact()
    assert bool((hw.view == 0xFF).all()) and bool((ho.buf == 0xFF).all())
    assert call() == 0                                                       # and the same buffers serve a good call
    torch.cuda.synchronize()
    hw.assert_bands_intact()
    ho.assert_bands_intact()
    assert torch.equal(out, m(emb, coords))


# ---- the file helper and the range guard ------------------------------------------------------------------------------------------------------------
def test_contextualise_features_round_trip(gpu, tmp_path):
    fx = load_fixture()["a"]
    c = fx["cases"]["n70"]
    m = _model(gpu, "a", c["key"])
    tile_um = 256.0
    coords_um = (c["coords"] / 37.5 * tile_um).numpy().astype(np.float32)          # the fixture's grid cells, one tile apart
    feats = c["emb"].half().numpy()
    src, dst = tmp_path / "slide.h5", tmp_path / "slide_ticon.h5"
    h5io.write_tile_features(src, feats, coords_um, extractor="h_optimus_1-test", tile_size_um=tile_um, tile_size_px=224, code_hash="00000000", stamp_version=STAMP_FORMAT_VERSION)
    contextualise_features(m, src, dst)
    got, ci, attrs = h5io.read_tile_features(dst)
    assert attrs["extractor"] == "h_optimus_1-test+ticon" and attrs["feat_type"] == "tile"
    assert np.array_equal(ci.coords_um, coords_um) and ci.tile_size_um == tile_um and ci.tile_size_px == 224
    direct = m(torch.from_numpy(feats).to(gpu), torch.from_numpy(coords_um).to(gpu) * (1.0 / tile_um))
    assert got.shape == (70, fx["dim"]) and np.array_equal(got, direct.cpu().numpy())
    contextualise_features(m, src, dst, coord_scale=37.5 / tile_um)                 # the fixture's own coordinates
    got2, _, _ = h5io.read_tile_features(dst)
    whole, rows = _rel(torch.from_numpy(got2), c["out64"])
    assert whole <= 1e-3 and rows <= 2e-3, (whole, rows)
    assert not np.array_equal(got2, got)


def test_fp16_overflow_is_handled_by_the_bf16_rerun(gpu):
    """Input projection scaled so that its hidden leaves the fp16 range: check=True returns finite features (bf16 operands from then on, one
    warning), check=False shows the overflow, and a model that is non-finite on bf16 operands as well raises FeatureRangeError."""
    from stamp_amd.vit import FeatureRangeError
    fx = load_fixture()["b"]
    c = fx["cases"]["n70"]
    p = f"input_proj_dict.input_proj_{c['key']}."
    sd = dict(fx["sd"])
    sd[p + "fc1.weight"], sd[p + "fc1.bias"] = sd[p + "fc1.weight"] * 3e4, sd[p + "fc1.bias"] * 3e4
    emb, coords = c["emb"].to(gpu), c["coords"].to(gpu)
    raw = HipTiconSlide(sd, key=c["key"], device=gpu, heads=fx["heads"], check=False)(emb, coords)
    assert not bool(torch.isfinite(raw).all()), "the scaled model was meant to overflow fp16"
    m = HipTiconSlide(sd, key=c["key"], device=gpu, heads=fx["heads"], check=True)
    with pytest.warns(RuntimeWarning, match="bf16"):
        out = m(emb, coords)
    assert m.dtype == torch.bfloat16 and bool(torch.isfinite(out).all())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert torch.equal(m(emb, coords), out)                                      # stays on bf16, no second warning
    sd[p + "fc1.bias"] = sd[p + "fc1.bias"].clone()
    sd[p + "fc1.bias"][0] = float("inf")
    with pytest.warns(RuntimeWarning, match="bf16"), pytest.raises(FeatureRangeError):
        HipTiconSlide(sd, key=c["key"], device=gpu, heads=fx["heads"])(emb, coords)
