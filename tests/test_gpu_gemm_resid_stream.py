"""The streamed RESIDUAL epilogue on the two fp16 planes (gemm_4w16.h STREAM with AMDS_EPI_RESIDUAL: amds_gemm_lnfold_planes, f16), one tile per workgroup
(AMDS_GEMM_RESID_PERSIST=0 or AMDS_GEMM_PERSIST=0) and in the persistent tile walk (AMDS_GEMM_RESID_PERSIST=1 here), against the one-phase form of the same library (AMDS_GEMM_RESID_STREAM=0, read at every call).

Every element goes through the same operations in the same order in all three forms, so the planes' bar is torch.equal: no tolerance.  The partial row
sums are added in another order than in the one-phase form (each wave reduces its 64 columns in registers, the two 128-column halves of a slot meet in
LDS), so they are held to the fp64 sums of the fp32 value at the tolerance of test_gemm_lnfold_planes (rtol 2e-5, atol 1e-3), and to torch.equal between
the two streamed forms and between calls: their order of additions is fixed.  Operands sit in guarded allocations (tests/guarded.py): poison 0x00 and
0xFF, bands and pitch padding untouched.

On a 256-CU part a small problem has fewer tiles than workgroups and nothing would loop: AMDS_GEMM_PERSIST_WGS=8 (unless stated) makes 18 tiles a walk of
2-3 tiles per workgroup.  Shapes: (1300, 768) = 6 x 3 tiles with a ragged last row tile, (257, 1024) = a row tile with one row, (513, 512) = 6 tiles,
fewer than the grid, (2048, 256) = 8 tiles, exactly the grid.  K = 64 ... 320 is 1 ... 5 K tiles: both stage parities per output tile, and the case
where the last K tile is also the first."""

import pytest
import torch

import guarded as G
from guarded import Bufs, cur_stream as _st, ptr as _p
from stamp_amd import _lib, ops

pytestmark = pytest.mark.gpu
SWITCH, RPERSIST, PERSIST, WGS = "AMDS_GEMM_RESID_STREAM", "AMDS_GEMM_RESID_PERSIST", "AMDS_GEMM_PERSIST", "AMDS_GEMM_PERSIST_WGS"
SHAPES = [(1300, 768), (257, 1024), (513, 512), (2048, 256)]
FORMS = ("persist", "one_tile", "one_phase")        # streamed in the tile walk | streamed, AMDS_GEMM_RESID_PERSIST=0 | AMDS_GEMM_RESID_STREAM=0


@pytest.fixture
def env(monkeypatch):
    for k in (SWITCH, RPERSIST, PERSIST, WGS):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(WGS, "8")
    monkeypatch.setenv(RPERSIST, "1")
    return monkeypatch


def _operands(gpu, M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).half()
    a[:, 0] += (torch.arange(M) * 0.01).half()                # rows differ: a tile stored at another tile's place cannot pass
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    w[:, 0] += (torch.arange(N) * 0.003).half()               # ... and so do columns
    bias = torch.randn(N, generator=g)
    scale = 0.5 + torch.rand(N, generator=g)
    x0 = (torch.randn(M, N, generator=g) * torch.logspace(-3, 1, N)).to(gpu)      # columns from 1e-3 to 10, as test_gemm_lnfold_planes builds them
    hi, lo, _ = ops.ln_stats_split(x0, 1e-6)
    return a.to(gpu), w.to(gpu), bias.to(gpu), scale.to(gpu), hi, lo


def _planes(a, w, hi, lo, ld, bias, scale, rowpart, what):
    M, K = a.shape
    N = w.shape[0]
    _lib.check(_lib.lib().amds_gemm_lnfold_planes(_p(a), a.stride(0), _p(w), w.stride(0), M, N, K, _p(hi), _p(lo), ld, _p(bias), _p(scale), _p(rowpart), _st()),
               what)


def _launches():
    return _lib.lib().amds_gemm_persist_launches()


def _update(a, w, hi0, lo0, bias, scale):
    """One update of fresh copies of the start planes -> (hi, lo, rowpart)."""
    hi, lo = hi0.clone(), lo0.clone()
    rp = ops.gemm_lnfold_planes(a, w, hi, lo, bias=bias, scale=scale)
    return hi, lo, rp


def _want_rowpart(x):
    """fp64 sums of the fp32 value in the slot layout of test_gemm_lnfold_planes: slot tn * 2 + p = columns [64 p, 64 p + 64) of both halves of tile tn."""
    M, N = x.shape
    slab = x.view(M, N // 256, 2, 2, 64).permute(0, 1, 3, 2, 4).reshape(M, N // 128, 128).double()
    return torch.stack([slab.sum(-1), (slab * slab).sum(-1)], -1)


@pytest.mark.parametrize("M,N", SHAPES)
def test_streamed_equals_one_phase(gpu, env, M, N):
    """K = 64 ... 320 (and 1024 once), with and without LayerScale, pitch N and N + 8, both poison bytes: the planes of both streamed forms equal the
    one-phase form's bit for bit and are the fp16 split of the fp32 value the fp32-row epilogue forms; rowpart is that value's sums, the same bits in
    both streamed forms; nothing outside the planes is written; the persistent launch counter moves for the tile walk only."""
    for K in (64, 128, 192, 256, 320) + ((1024,) if (M, N) == (1300, 768) else ()):
        a0, w0, bias0, scale0, hi0, lo0 = _operands(gpu, M, N, K, M * 7 + N + K)
        for use_scale in (True, False):
            sc0 = scale0 if use_scale else None
            ref = hi0.float() + lo0.float()
            ops.gemm(a0, w0, _lib.EPI_RESIDUAL, bias=bias0, scale=sc0, out=ref, cfg=12)         # fp32 rows: the value both plane forms must form
            want = _want_rowpart(ref)
            for pad in (0, 8):
                if K == 1024 and pad:
                    continue
                tag = (M, N, K, use_scale, pad)

                def call(pattern):
                    b = Bufs(gpu, pattern)
                    a, w, bias = b.inp(a0, name="A"), b.inp(w0, name="W"), b.inp(bias0, name="bias")
                    scale = b.inp(scale0, name="scale") if use_scale else None
                    outs = {}
                    for form in FORMS:
                        hi, lo = b.inp(hi0, ld=N + pad, name=f"hi_{form}"), b.inp(lo0, ld=N + pad, name=f"lo_{form}")
                        rp = b.out((M, N // 128, 2), torch.float32, name=f"rowpart_{form}")
                        if form == "one_phase":
                            env.setenv(SWITCH, "0")
                        env.setenv(RPERSIST, "0" if form == "one_tile" else "1")
                        n0 = _launches()
                        _planes(a, w, hi, lo, N + pad, bias, scale, rp, f"{form} {tag}")
                        assert _launches() == n0 + (form == "persist"), (tag, form)        # the persistent instantiation ran exactly when expected
                        env.delenv(SWITCH, raising=False)
                        outs.update({f"hi_{form}": hi, f"lo_{form}": lo, f"rp_{form}": rp})
                    return b.result(**outs)

                o = G.run_contract(call)
                for form in ("persist", "one_tile"):
                    assert torch.equal(o[f"hi_{form}"], o["hi_one_phase"]) and torch.equal(o[f"lo_{form}"], o["lo_one_phase"]), (tag, form)
                assert torch.equal(o["hi_persist"], ref.half()) and torch.equal(o["lo_persist"], (ref - ref.half().float()).half()), tag
                assert torch.equal(o["rp_persist"], o["rp_one_tile"]), tag
                for form in FORMS:
                    assert torch.allclose(o[f"rp_{form}"].double(), want, rtol=2e-5, atol=1e-3), (tag, form)


@pytest.mark.parametrize("M,N,K", [(1300, 768, 128), (1300, 768, 192), (257, 1024, 64)])
def test_repeated_calls_and_grid_caps_give_the_same_bits(gpu, env, M, N, K):
    """The tile loop is a new synchronisation structure for this epilogue (slab stage against the next tile's LDS-DMA, the row sums' LDS area against the
    next tile's): 50 calls on the same start planes, planes and rowpart bit-equal every time and equal to the one-tile streamed form (fixed order of
    additions: no atomics); and once each with the grid capped at 16 workgroups and uncapped -- other tile-to-workgroup assignments."""
    a, w, bias, scale, hi0, lo0 = _operands(gpu, M, N, K, 23)
    env.setenv(RPERSIST, "0")
    hi_r, lo_r, rp_r = _update(a, w, hi0, lo0, bias, scale)
    env.setenv(RPERSIST, "1")
    assert bool(torch.isfinite(rp_r).all())
    n0 = _launches()
    for it in range(50):
        hi, lo, rp = _update(a, w, hi0, lo0, bias, scale)
        assert torch.equal(hi, hi_r) and torch.equal(lo, lo_r) and torch.equal(rp, rp_r), it
    for cap in ("16", None):
        env.setenv(WGS, cap) if cap else env.delenv(WGS)
        hi, lo, rp = _update(a, w, hi0, lo0, bias, scale)
        assert torch.equal(hi, hi_r) and torch.equal(lo, lo_r) and torch.equal(rp, rp_r), cap
    assert _launches() == n0 + 52


def test_switches(gpu, env):
    """AMDS_GEMM_PERSIST=0 turns the tile walk off for this launch too, AMDS_GEMM_RESID_STREAM=0 implies one tile per workgroup: by the library's launch
    counter no persistent instantiation runs, and the planes keep their bits."""
    M, N, K = 1300, 768, 128
    a, w, bias, scale, hi0, lo0 = _operands(gpu, M, N, K, 5)

    def run():
        n0 = _launches()
        hi, lo, rp = _update(a, w, hi0, lo0, bias, scale)
        return hi, lo, rp, _launches() - n0

    hi_r, lo_r, rp_r, n = run()
    assert n == 1
    env.setenv(PERSIST, "0")
    hi, lo, rp, n = run()
    assert n == 0 and torch.equal(hi, hi_r) and torch.equal(lo, lo_r) and torch.equal(rp, rp_r)
    env.delenv(PERSIST)
    env.setenv(SWITCH, "0")
    hi, lo, rp, n = run()
    assert n == 0 and torch.equal(hi, hi_r) and torch.equal(lo, lo_r)


def test_rows_do_not_depend_on_the_rows_below(gpu, env):
    """The first 513 rows of an M = 1300 call, planes and rowpart, equal an M = 513 call on the same rows."""
    M, m, N, K = 1300, 513, 768, 192
    a, w, bias, scale, hi0, lo0 = _operands(gpu, M, N, K, 31)
    hi, lo, rp = _update(a, w, hi0, lo0, bias, scale)
    hi_s, lo_s, rp_s = _update(a[:m].contiguous(), w, hi0[:m].contiguous(), lo0[:m].contiguous(), bias, scale)
    assert torch.equal(hi[:m], hi_s) and torch.equal(lo[:m], lo_s) and torch.equal(rp[:m], rp_s)


def test_chain_of_48_updates_in_place(gpu, env):
    """48 successive in-place updates (a 24-block trunk): the planes stay bit-equal to the one-phase form's 48."""
    M, N, K = 1300, 768, 128
    a, w, bias, scale, hi0, lo0 = _operands(gpu, M, N, K, 37)
    scale = scale * 0.1
    hi_s, lo_s, hi_o, lo_o = hi0.clone(), lo0.clone(), hi0.clone(), lo0.clone()
    for _ in range(48):
        ops.gemm_lnfold_planes(a, w, hi_s, lo_s, bias=bias, scale=scale)
    env.setenv(SWITCH, "0")
    for _ in range(48):
        ops.gemm_lnfold_planes(a, w, hi_o, lo_o, bias=bias, scale=scale)
    env.delenv(SWITCH)
    assert bool(torch.isfinite(hi_s.float()).all()) and not torch.equal(hi_s, hi0)
    assert torch.equal(hi_s, hi_o) and torch.equal(lo_s, lo_o)


def test_vit_large_with_the_switch_on_and_off(gpu, env):
    """ViT-L/14, 6 tiles, as test_residual_planes_against_fp32_rows sets it up.  The streamed form changes the row sums in rounding only, so the two
    settings are two accepted forms of the same computation: each below 1e-3 from the oracle, the streamed one at most 1.05 x (tokens) / 1.1 x (stored
    feature) the one-phase form's error -- the factors that test uses between the plane and the fp32-row forms; chunk 4 and chunk 6 agree bit for bit,
    and so do two calls and the tile walk against one tile per workgroup."""
    from oracle.vit_tile_encoder import extract_features
    from stamp_amd.vit import PRESETS, HipViT, random_vit_state_dict

    def rel(x, y):
        return ((x.double() - y.double()).norm() / y.double().norm()).item()

    env.delenv(WGS)
    env.delenv(RPERSIST)                                        # the product's default
    cfg = PRESETS["vit_large_patch14_224"]
    sd = random_vit_state_dict(cfg, seed=0, init="moderate")
    tiles = torch.randint(0, 256, (6, 224, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))
    ref_f, ref_t = extract_features(tiles[:4], sd, cfg, return_tokens=True)
    model = HipViT(cfg, sd, device=gpu, chunk=4)
    assert model.ln_fold
    f_on, t_on = model(tiles.to(gpu), return_tokens=True)
    d_on = model(tiles.to(gpu))
    assert torch.equal(d_on, model(tiles.to(gpu)))
    assert torch.equal(d_on, HipViT(cfg, sd, device=gpu, chunk=6)(tiles.to(gpu)))
    env.setenv(PERSIST, "0")
    assert torch.equal(d_on, model(tiles.to(gpu)))              # every GEMM one tile per workgroup: same bits
    env.delenv(PERSIST)
    env.setenv(SWITCH, "0")
    f_off, t_off = model(tiles.to(gpu), return_tokens=True)
    d_off = model(tiles.to(gpu))
    env.delenv(SWITCH)
    e_on, e_off = rel(t_on[:4].cpu(), ref_t), rel(t_off[:4].cpu(), ref_t)
    c_on, c_off = rel(d_on[:4].cpu().float(), ref_f.float()), rel(d_off[:4].cpu().float(), ref_f.float())
    print(f"ViT-L/14 streamed vs one-phase residual epilogue: tokens {rel(t_on, t_off):.2e}, stored feature {rel(d_on.float(), d_off.float()):.2e}; "
          f"vs oracle: tokens {e_on:.3e} / {e_off:.3e}, stored feature {c_on:.3e} / {c_off:.3e}")
    assert e_on < 1e-3 and c_on < 1e-3
    assert e_on <= 1.05 * e_off and c_on <= 1.1 * c_off
