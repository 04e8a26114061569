"""Bands and pitch of the GEMM entry points (family B of the C-ABI contract tests; tests/guarded.py).

Every operand sits in a guarded allocation: inputs with the poison byte in their bands and pitch padding, outputs poisoned everywhere.  Each case runs
under 0x00 and 0xFF and asserts bit-identical, finite outputs, untouched bands and padding, and -- on the 0x00 run -- the fp64 bar of the kernel's own
parity test (tests/test_gpu_kernels.py, test_gpu_train.py, test_gpu_transmil_train.py, test_gpu_swin.py, test_gpu_fp8.py; restated here, unchanged).
Shapes: the smallest on each side of every tile edge (M = 1, 255, 257, 300, 513 against the 128- and 256-row tiles), pitches tight and width + 8.
What the header demands of padding is supplied: K is a multiple of 64 in most cases, so no operand has padded columns the kernel may read; one case pads K and N the
way the header prescribes (amds_cast_pad writes the zero columns, the caller the zero weight rows) and poisons everything behind that."""

import pytest
import torch

import guarded as G
from guarded import Bufs, act_eps as _eps, cur_stream as _st, ptr as _p
from stamp_amd import _lib, ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]


EPIS = ["BIAS", "BIAS_F32", "RESIDUAL", "GELU", "SWIGLU"]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [1, 255, 257, 300, 513])
@pytest.mark.parametrize("cfg", [0, 8, 10, 12, -1, -2])
def test_gemm_ex(gpu, cfg, M, dt):
    """amds_gemm_ex: N = 256, K = 64 and 192, tight and padded pitches, five epilogues.  Bars: test_gemm_epilogues (BIAS / GELU: one ulp of the act dtype at the top
    of the range; RESIDUAL: 2e-5), test_gemm_8phase_pipeline (BIAS_F32: 1e-4 (K / 1024 + 1) of the range), test_gemm_swiglu (1.05 ulp + 1e-5)."""
    lib, N = _lib.lib(), 256
    g = torch.Generator().manual_seed(M * 3 + N + cfg)
    for K in (64, 192):
        a0 = torch.randn(M, K, generator=g).to(dt)
        a0[:, 0] += torch.arange(M).to(dt) * 0.01               # a transposed / swapped C write cannot pass
        w0 = (torch.randn(N, K, generator=g) / K ** 0.5).to(dt)
        bias0, scale0 = torch.randn(N, generator=g), torch.rand(N, generator=g)
        x0 = torch.randn(M, N, generator=g)
        wp0 = ops.pack_swiglu_rows(w0.float().to(gpu)).to(dt).cpu()
        bp0 = ops.pack_swiglu_rows(bias0.to(gpu).reshape(-1, 1)).reshape(-1).cpu()
        lin = a0.double() @ w0.double().t() + bias0.double()
        for pad in (0, 8):
            for epi in EPIS:
                code = {"BIAS": _lib.EPI_BIAS, "BIAS_F32": _lib.EPI_BIAS_F32, "RESIDUAL": _lib.EPI_RESIDUAL, "GELU": _lib.EPI_BIAS_GELU, "SWIGLU": _lib.EPI_SWIGLU}[epi]
                ocols = N // 2 if epi == "SWIGLU" else N
                odt = torch.float32 if epi in ("BIAS_F32", "RESIDUAL") else dt

                def call(pattern):
                    b = Bufs(gpu, pattern)
                    a = b.inp(a0, K + pad, "A")
                    w = b.inp(wp0 if epi == "SWIGLU" else w0, K + pad, "W")
                    bias = b.inp(bp0 if epi == "SWIGLU" else bias0, name="bias")
                    scale = b.inp(scale0, name="scale") if epi == "RESIDUAL" else None
                    out = b.out((M, ocols), odt, ocols + pad, "out")
                    if epi == "RESIDUAL":
                        out.copy_(x0)
                    _lib.check(lib.amds_gemm_ex(cfg, _p(a), K + pad, _p(w), K + pad, M, N, K, ops.act_code(dt), code, _p(out), ocols + pad, _p(bias), _p(scale), None,
                                                0, 0, 0, 1.0, _st()), f"gemm cfg {cfg} {epi} K {K} pad {pad}")
                    return b.result(out=out)

                out = G.run_contract(call)["out"].double().cpu()
                tag = (cfg, M, K, pad, epi)
                if epi == "BIAS":
                    assert (out - lin).abs().max().item() < _eps(dt) * lin.abs().max().item() * 1.01, tag
                elif epi == "GELU":
                    r = torch.nn.functional.gelu(lin)
                    assert (out - r).abs().max().item() < _eps(dt) * r.abs().max().item() * 1.01 + 1e-6, tag
                elif epi == "BIAS_F32":
                    assert (out - lin).abs().max().item() < 1e-4 * max(1.0, lin.abs().max().item()) * (K / 1024 + 1), tag
                elif epi == "RESIDUAL":
                    assert (out - (x0.double() + scale0.double() * lin)).abs().max().item() < 2e-5, tag
                else:
                    H = N // 2
                    r = torch.nn.functional.silu(lin[:, :H]) * lin[:, H:]
                    assert (out - r).abs().max().item() < _eps(dt) * r.abs().max().item() * 1.05 + 1e-5, tag


def test_gemm_ex_three_column_tiles_of_128(gpu):
    """N = 384 at cfg 0: a column-tile count that is not a multiple of two (test_gemm_bias_asymmetric's (257, 384, 128), its bars)."""
    lib, (M, N, K), dt = _lib.lib(), (257, 384, 128), torch.float16
    g = torch.Generator().manual_seed(M + N + K)
    a0, w0, bias0 = torch.randn(M, K, generator=g).to(dt), (torch.randn(N, K, generator=g) / K ** 0.5).to(dt), torch.randn(N, generator=g)
    a0[:, 0] += torch.arange(M).to(dt) * 0.01
    ref = a0.double() @ w0.double().t() + bias0.double()
    for pad in (0, 8):
        def call(pattern):
            b = Bufs(gpu, pattern)
            a, w, bias, out = b.inp(a0, K + pad, "A"), b.inp(w0, K + pad, "W"), b.inp(bias0, name="bias"), b.out((M, N), torch.float32, N + pad, "out")
            _lib.check(lib.amds_gemm_ex(0, _p(a), K + pad, _p(w), K + pad, M, N, K, _lib.F16, _lib.EPI_BIAS_F32, _p(out), N + pad, _p(bias), None, None, 0, 0, 0, 1.0, _st()))
            return b.result(out=out)

        out = G.run_contract(call)["out"].double().cpu()
        assert (out - ref).abs().max().item() < 2e-3 * max(1.0, ref.abs().max().item())
        assert (out - ref).abs().mean().item() < 1e-5 * ref.abs().mean().item() + 1e-6


@pytest.mark.parametrize("dt", DTYPES)
def test_gemm_ex_on_operands_padded_by_cast_pad(gpu, dt):
    """K = 100 padded to 128 and N = 200 padded to 256, the header's precondition: amds_cast_pad produces the 16-bit operands and writes the zero columns up to ld_dst
    itself, the weight's rows 200 .. 255 are the caller's zeros; bands behind both.  Columns < 200 against fp64 on the rounded operands (BIAS_F32's bar of
    test_gemm_8phase_pipeline); the padded output columns are exactly the (zero) padded bias."""
    lib, (M, N, K, Np, Kp) = _lib.lib(), (257, 200, 100, 256, 128)
    g = torch.Generator().manual_seed(100)
    a0, w0, bias0 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    ref = a0.to(dt).double() @ w0.to(dt).double().t() + bias0.double()

    def call(pattern):
        b = Bufs(gpu, pattern)
        a32, w32 = b.inp(a0, K + 4, "A fp32"), b.inp(w0, K + 4, "W fp32")
        a16, w16 = b.out((M, Kp), dt, name="A"), b.out((Np, Kp), dt, name="W")
        w16[N:] = 0
        bias = b.inp(torch.cat([bias0, torch.zeros(Np - N)]), name="bias")
        _lib.check(lib.amds_cast_pad(_p(a32), K + 4, _p(a16), Kp, M, K, ops.act_code(dt), _st()), "cast_pad A")
        _lib.check(lib.amds_cast_pad(_p(w32), K + 4, _p(w16), Kp, N, K, ops.act_code(dt), _st()), "cast_pad W")
        out = b.out((M, Np), torch.float32, Np + 8, "out")
        _lib.check(lib.amds_gemm_ex(-1, _p(a16), Kp, _p(w16), Kp, M, Np, Kp, ops.act_code(dt), _lib.EPI_BIAS_F32, _p(out), Np + 8, _p(bias), None, None, 0, 0, 0, 1.0, _st()), "gemm")
        return b.result(out=out, a16=a16, w16=w16)

    o = {k_: v.cpu() for k_, v in G.run_contract(call).items()}
    assert torch.equal(o["a16"][:, :K], a0.to(dt)) and bool((o["a16"][:, K:] == 0).all()) and bool((o["w16"][:N, K:] == 0).all())
    assert (o["out"][:, :N].double() - ref).abs().max().item() < 1e-4 * max(1.0, ref.abs().max().item()) * (Kp / 1024 + 1)
    assert bool((o["out"][:, N:] == 0).all())


def _slab_sums(ref, M, N):
    slab = ref.view(M, N // 256, 2, 2, 64).permute(0, 1, 3, 2, 4).reshape(M, N // 128, 128).double()
    return torch.stack([slab.sum(-1), (slab * slab).sum(-1)], -1)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,N,K,use_scale", [(515, 512, 1024, False), (256, 256, 64, True)])
def test_gemm_lnfold_producer(gpu, dt, M, N, K, use_scale):
    """amds_gemm_lnfold, producer form: out, the 16-bit copy xh and the partial row sums rowpart under bands (test_gemm_lnfold_producer's bars; the fp32 rows
    against fp64 at the RESIDUAL epilogue's 2e-5 (K / 1024 + 1))."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(5)
    a0, w0 = torch.randn(M, K, generator=g).to(dt), (torch.randn(N, K, generator=g) / K ** 0.5).to(dt)
    bias0, scale0, x0 = torch.randn(N, generator=g), 0.5 + torch.rand(N, generator=g), torch.randn(M, N, generator=g)
    ref = x0.double() + (scale0.double() if use_scale else 1.0) * (a0.double() @ w0.double().t() + bias0.double())
    for pad in (0, 8):
        def call(pattern):
            b = Bufs(gpu, pattern)
            a, w, bias = b.inp(a0, K + pad, "A"), b.inp(w0, K + pad, "W"), b.inp(bias0, name="bias")
            scale = b.inp(scale0, name="scale") if use_scale else None
            out, xh, rowpart = b.out((M, N), torch.float32, N + pad, "out"), b.out((M, N), dt, N + pad, "xh"), b.out((M, N // 128, 2), torch.float32, name="rowpart")
            out.copy_(x0)
            _lib.check(lib.amds_gemm_lnfold(_p(a), K + pad, _p(w), K + pad, M, N, K, ops.act_code(dt), _lib.EPI_RESIDUAL, _p(out), N + pad, _p(bias), _p(scale), _p(xh),
                                            _p(rowpart), None, None, _st()), "lnfold producer")
            return b.result(out=out, xh=xh, rowpart=rowpart)

        o = G.run_contract(call)
        assert (o["out"].double().cpu() - ref).abs().max().item() < 2e-5 * (K / 1024 + 1)
        assert torch.equal(o["xh"], o["out"].to(dt))
        assert torch.allclose(o["rowpart"].double().cpu(), _slab_sums(o["out"].cpu(), M, N), rtol=2e-5, atol=1e-3)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("epi", ["bias", "gelu", "swiglu"])
@pytest.mark.parametrize("M,D,N", [(515, 1024, 512), (256, 64, 256)])
def test_gemm_lnfold_consumer(gpu, dt, epi, M, D, N):
    """amds_gemm_lnfold, consumer form, against Linear(LayerNorm(x)) in fp64 (test_gemm_lnfold_consumer: 8e-4 / 6e-3 relative L2, no massive channel here)."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(M, D, generator=g) * 3.0 + 0.4
    gamma, beta = 1.0 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    W, bvec = torch.randn(N, D, generator=g) / D ** 0.5, 0.1 * torch.randn(N, generator=g)
    y64 = torch.nn.functional.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-6) @ W.double().t() + bvec.double()
    if epi == "swiglu":
        want = torch.nn.functional.silu(y64[:, :N // 2]) * y64[:, N // 2:]
        Wp, bp = ops.pack_swiglu_rows(W.to(gpu)).cpu(), ops.pack_swiglu_rows(bvec.to(gpu).view(-1, 1)).view(-1).cpu()
    else:
        want, Wp, bp = (torch.nn.functional.gelu(y64) if epi == "gelu" else y64), W, bvec
    code = {"bias": _lib.EPI_BIAS, "gelu": _lib.EPI_BIAS_GELU, "swiglu": _lib.EPI_SWIGLU}[epi]
    Wf = (Wp * gamma[None, :]).to(dt)
    colsum0, bf0 = Wf.float().sum(1), bp + Wp @ beta
    ocols = N // 2 if epi == "swiglu" else N
    for pad in (0, 8):
        def call(pattern):
            b = Bufs(gpu, pattern)
            xin = b.inp(x, D + pad, "x")
            xh, rs = b.out((M, D), dt, D + pad, "xh"), b.out((M, 2), torch.float32, name="rowstat")
            _lib.check(lib.amds_ln_stats_cast(_p(xin), D + pad, M, D, 1e-6, _p(xh), D + pad, _p(rs), ops.act_code(dt), _st()), "ln_stats_cast")
            w, bias, colsum = b.inp(Wf, D + pad, "W"), b.inp(bf0, name="bias"), b.inp(colsum0, name="colsum")
            out = b.out((M, ocols), dt, ocols + pad, "out")
            _lib.check(lib.amds_gemm_lnfold(_p(xh), D + pad, _p(w), D + pad, M, N, D, ops.act_code(dt), code, _p(out), ocols + pad, _p(bias), None, None, None, _p(rs),
                                            _p(colsum), _st()), "lnfold consumer")
            return b.result(out=out, xh=xh, rowstat=rs)

        o = G.run_contract(call)
        assert torch.equal(o["xh"].cpu(), x.to(dt))
        e = ((o["out"].double().cpu() - want).norm() / want.norm()).item()
        assert e < (6e-3 if dt == torch.bfloat16 else 8e-4), e


@pytest.mark.parametrize("M,N,K,use_scale", [(515, 512, 1024, False), (256, 256, 64, True)])
def test_gemm_lnfold_planes(gpu, M, N, K, use_scale):
    """amds_ln_stats_split + amds_gemm_lnfold_planes + amds_planes_to_f32, the two fp16 planes and rowpart under bands (test_gemm_lnfold_planes' statements)."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(5)
    a0, w0 = torch.randn(M, K, generator=g).half(), (torch.randn(N, K, generator=g) / K ** 0.5).half()
    bias0, scale0 = torch.randn(N, generator=g), 0.5 + torch.rand(N, generator=g)
    x0 = torch.randn(M, N, generator=g) * torch.logspace(-3, 1, N)
    hi0 = x0.half()
    xin = hi0.float() + (x0 - hi0.float()).half().float()
    ref = xin.double() + (scale0.double() if use_scale else 1.0) * (a0.double() @ w0.double().t() + bias0.double())
    for pad in (0, 8):
        def call(pattern):
            b = Bufs(gpu, pattern)
            x, a, w, bias = b.inp(x0, N + pad, "x"), b.inp(a0, K + pad, "A"), b.inp(w0, K + pad, "W"), b.inp(bias0, name="bias")
            scale = b.inp(scale0, name="scale") if use_scale else None
            hi, lo = b.out((M, N), torch.float16, N + pad, "hi"), b.out((M, N), torch.float16, N + pad, "lo")
            rs, rowpart = b.out((M, 2), torch.float32, name="rowstat"), b.out((M, N // 128, 2), torch.float32, name="rowpart")
            _lib.check(lib.amds_ln_stats_split(_p(x), N + pad, M, N, 1e-6, _p(hi), _p(lo), N + pad, _p(rs), _st()), "ln_stats_split")
            hi_in, lo_in = hi.clone(), lo.clone()
            _lib.check(lib.amds_gemm_lnfold_planes(_p(a), K + pad, _p(w), K + pad, M, N, K, _p(hi), _p(lo), N + pad, _p(bias), _p(scale), _p(rowpart), _st()), "planes")
            x32 = b.out((M, N), torch.float32, N + pad, "x32")
            _lib.check(lib.amds_planes_to_f32(_p(hi), _p(lo), N + pad, 1, _p(x32), N + pad, M, N, _st()), "planes_to_f32")
            return b.result(hi=hi, lo=lo, rowstat=rs, rowpart=rowpart, x32=x32, hi_in=hi_in, lo_in=lo_in)

        o = {k: v.cpu() for k, v in G.run_contract(call).items()}
        assert torch.equal(o["hi_in"], hi0) and torch.equal(o["lo_in"], (x0 - hi0.float()).half())
        assert torch.equal(o["x32"], o["hi"].float() + o["lo"].float())
        assert (o["x32"].double() - ref).abs().max().item() < 2e-5 * (K / 1024 + 1) * max(1.0, ref.abs().max().item())
        assert torch.allclose(o["rowpart"].double(), _slab_sums(o["x32"], M, N), rtol=2e-5, atol=1e-3)
        mean, rstd = x0.double().mean(1), 1.0 / torch.sqrt(x0.double().var(1, unbiased=False) + 1e-6)
        assert torch.allclose(o["rowstat"][:, 0].double(), rstd, rtol=1e-4) and torch.allclose(o["rowstat"][:, 1].double(), -mean * rstd, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("K,N,epi,ln", [(96, 288, "bias", True), (96, 384, "gelu", True), (96, 96, "res", False), (192, 576, "bias", True), (192, 768, "gelu", True),
                                        (192, 192, "res", False), (384, 96, "res", False), (384, 192, "f32", False)])
def test_gemm_rowstream(gpu, K, N, epi, ln):
    """amds_gemm_rowstream at M = 77, every (K, epilogue, LayerNorm) combination the Swin stages use (test_gemm_rowstream's cases and bars: 1e-3 relative L2 with
    the fused LayerNorm, 3e-5 sqrt(K) on the fp32 outputs)."""
    lib, M, dt = _lib.lib(), 77, torch.float16
    g = torch.Generator().manual_seed(K + N + M)
    w0, bias0 = (torch.randn(N, K, generator=g) / K ** 0.5).to(dt), torch.randn(N, generator=g) * 0.3
    gam, bet = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    a0 = (torch.randn(M, K, generator=g) * 2 + 0.5) if ln else torch.randn(M, K, generator=g).to(dt)
    x0 = torch.randn(M, N, generator=g)
    h = torch.nn.functional.layer_norm(a0.double(), (K,), gam.double(), bet.double(), 1e-5) if ln else a0.double()
    y = h @ w0.double().t()
    ref = {"bias": y + bias0.double(), "gelu": torch.nn.functional.gelu(y + bias0.double()), "res": x0.double() + y + bias0.double(), "f32": y}[epi]
    code = {"bias": _lib.EPI_BIAS, "gelu": _lib.EPI_BIAS_GELU, "res": _lib.EPI_RESIDUAL, "f32": _lib.EPI_BIAS_F32}[epi]
    for pad in (0, 8):
        def call(pattern):
            b = Bufs(gpu, pattern)
            a, w = b.inp(a0, K + pad, "A"), b.inp(w0, K + pad, "W")
            bias = b.inp(bias0, name="bias") if epi != "f32" else None
            gw, gb = (b.inp(gam, name="gamma"), b.inp(bet, name="beta")) if ln else (None, None)
            out = b.out((M, N), dt if ln else torch.float32, N + pad, "out")
            if epi == "res":
                out.copy_(x0)
            _lib.check(lib.amds_gemm_rowstream(_p(a), K + pad, _p(gw), _p(gb), 1e-5, _p(w), K + pad, M, N, K, _lib.F16, code, _p(out), N + pad, _p(bias), _st()), "rowstream")
            return b.result(out=out)

        out = G.run_contract(call)["out"].double().cpu()
        if ln:
            assert ((out - ref).norm() / ref.norm()).item() < 1e-3, pad
        else:
            assert (out - ref).abs().max().item() < 3e-5 * K ** 0.5, pad


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("tokens,N,K,split_k,pitch", [(77, 512, 256, 2, 0), (1000, 256, 512, 4, 64)])
def test_wgrad_tn_and_gemm_batched(gpu, dt, tokens, N, K, split_k, pitch):
    """amds_wgrad_tn on token-major operands and amds_gemm_batched on their transposes (test_wgrad_tn_token_major_operands: the summed partials within 1e-3 of the
    range of the fp64 product; the two routes bit-identical split by split)."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(tokens + N)
    dy0, x0 = torch.randn(tokens, N, generator=g).to(dt), torch.randn(tokens, K, generator=g).to(dt)
    ref = dy0.double().t() @ x0.double()
    chunk = (tokens + 64 * split_k - 1) // (64 * split_k) * 64
    Tp = chunk * split_k
    dyT0, xT0 = torch.zeros(N, Tp, dtype=dt), torch.zeros(K, Tp, dtype=dt)            # the transposed, zero-padded copies the batched form reads
    dyT0[:, :tokens], xT0[:, :tokens] = dy0.t(), x0.t()

    def call(pattern):
        b = Bufs(gpu, pattern)
        dy, x = b.inp(dy0, N + pitch, "dy"), b.inp(x0, K + pitch, "x")
        part = b.out((split_k, N, K), torch.float32, name="part")
        _lib.check(lib.amds_wgrad_tn(_p(dy), N + pitch, _p(x), K + pitch, tokens, N, K, split_k, ops.act_code(dt), _p(part), _st()), "wgrad_tn")
        dyT, xT = b.inp(dyT0, Tp + pitch, "dyT"), b.inp(xT0, Tp + pitch, "xT")
        part2 = b.out((split_k, N, K), torch.float32, name="part2")
        _lib.check(lib.amds_gemm_batched(_p(dyT), Tp + pitch, chunk, _p(xT), Tp + pitch, chunk, N, K, chunk, split_k, ops.act_code(dt), _lib.EPI_BIAS_F32, _p(part2), K,
                                         N * K, None, 1.0, _st()), "gemm_batched")
        nb = lib.amds_colsum_workspace_bytes(split_k, N * K)
        ws, dw = b.out((max(nb, 1),), torch.uint8, name="colsum ws"), b.out((N, K), torch.float32, name="dW")
        _lib.check(lib.amds_colsum(_p(part), N * K, _p(dw), split_k, N * K, _lib.F32, 0, _p(ws), nb, _st()), "colsum")
        return b.result(part=part, part2=part2, dW=dw)

    o = G.run_contract(call)
    assert (o["dW"].double().cpu() - ref).abs().max().item() < 1e-3 * ref.abs().max().item()
    assert (o["part2"].double().sum(0).cpu() - ref).abs().max().item() < 1e-3 * ref.abs().max().item()


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("n,Cd", [(70, 64), (300, 128)])
def test_bgemm_f32_on_head_slices_of_a_packed_qkv(gpu, precision, n, Cd):
    """amds_bgemm_f32 / _dual addressed the way the TransMIL chain does (tests/chains/transmil.py): q k^T per (bag, head) on slices of the packed qkv [b][n][3 C], the
    band behind qkv poisoned; then a square product with two outputs.  Bars: test_bgemm_f32_high_precision_mode (1e-5 of the range at "highest", 2e-4 at "high")."""
    lib, Bb, Hh = _lib.lib(), 2, 8
    d = Cd // Hh
    g = torch.Generator().manual_seed(n + Cd)
    qkv0 = torch.randn(Bb, n, 3 * Cd, generator=g)
    q, k = (qkv0[..., i * Cd:(i + 1) * Cd].reshape(Bb, n, Hh, d).permute(0, 2, 1, 3).double() for i in range(2))
    ref = 0.5 * q @ k.transpose(-1, -2)
    sq0 = torch.randn(Bb * Hh, n, n, generator=g) / n ** 0.5
    ref2 = sq0.double() @ sq0.double()
    tol = 1e-5 if precision == "highest" else 2e-4

    def call(pattern):
        b = Bufs(gpu, pattern)
        qkv = b.inp(qkv0.reshape(Bb * n, 3 * Cd), name="qkv")
        sim = b.out((Bb * Hh * n, n), torch.float32, name="sim")
        rc = lib.amds_bgemm_f32(_p(qkv), 3 * Cd, n * 3 * Cd, d, qkv.data_ptr() + 4 * Cd, 3 * Cd, n * 3 * Cd, d, 1, _p(sim), n, Hh * n * n, n * n, Bb, Hh, n, n, d, 0.5, 0.0,
                                None, 0, _st())
        _lib.check(rc, "bgemm_f32")
        sq = b.inp(sq0.reshape(-1, n), name="sq")
        c1, c2 = b.out((Bb * Hh * n, n), torch.float32, name="C"), b.out((Bb * Hh * n, n), torch.float32, name="C2")
        _lib.check(lib.amds_bgemm_f32_dual(_p(sq), n, n * n, 0, _p(sq), n, n * n, 0, 0, _p(c1), _p(c2), n, n * n, 0, Bb * Hh, 1, n, n, n, 1.0, 0.0, -1.0, 7.0, _st()), "dual")
        return b.result(sim=sim, C=c1, C2=c2)

    with ops.float32_matmul_precision(precision):
        o = {k_: v.double().cpu() for k_, v in G.run_contract(call).items()}
    assert (o["sim"].view(Bb, Hh, n, n) - ref).abs().max().item() < tol * max(1.0, ref.abs().max().item())
    assert (o["C"].view(-1, n, n) - ref2).abs().max().item() < tol * max(1.0, ref2.abs().max().item())
    assert (o["C2"].view(-1, n, n) - (7.0 * torch.eye(n, dtype=torch.float64) - ref2)).abs().max().item() < tol * 7.0


def test_gemm_fp8(gpu):
    """amds_quantize_rows_e4m3 + amds_gemm_fp8 at (65, 768, 384) against the fp64 product of the same e4m3 operands
    (test_gemm_fp8_matches_fp64_on_the_same_operands: 8e-4 relative L2); pitches tight and + 16 (the header asks for multiples of 16)."""
    lib, (M, N, K) = _lib.lib(), (65, 768, 384)
    g = torch.Generator().manual_seed(65)
    x0, w0, bias0 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    for pad in (0, 16):
        def call(pattern):
            b = Bufs(gpu, pattern)
            x, w, bias = b.inp(x0, K + pad, "x"), b.inp(w0, K + pad, "w"), b.inp(bias0, name="bias")
            a8, rs = b.out((M, K), torch.uint8, K + pad, "a8"), b.out((M,), torch.float32, name="rowscale")
            w8, cs = b.out((N, K), torch.uint8, K + pad, "w8"), b.out((N,), torch.float32, name="colscale")
            _lib.check(lib.amds_quantize_rows_e4m3(_p(x), K + pad, _p(a8), K + pad, _p(rs), M, K, _lib.F32, _st()), "quantize x")
            _lib.check(lib.amds_quantize_rows_e4m3(_p(w), K + pad, _p(w8), K + pad, _p(cs), N, K, _lib.F32, _st()), "quantize w")
            out = b.out((M, N), torch.float16, N + pad, "out")
            _lib.check(lib.amds_gemm_fp8(_p(a8), K + pad, _p(w8), K + pad, M, N, K, _lib.EPI_BIAS, _p(out), N + pad, _p(bias), _p(cs), _p(rs), _st()), "gemm_fp8")
            return b.result(out=out, a8=a8, w8=w8, rowscale=rs, colscale=cs)

        o = G.run_contract(call)
        sa, sw = o["rowscale"], o["colscale"]
        assert torch.equal(o["a8"].view(torch.float8_e4m3fn).float(), (x0.to(gpu) / sa[:, None]).to(torch.float8_e4m3fn).float())       # test_quantize_rows_e4m3
        acc = o["a8"].view(torch.float8_e4m3fn).to(torch.float64) @ o["w8"].view(torch.float8_e4m3fn).to(torch.float64).T
        ref = acc * sa.double()[:, None] * sw.double()[None, :] + bias0.to(gpu).double()
        assert ((o["out"].double() - ref).norm() / ref.norm()).item() < 8e-4
