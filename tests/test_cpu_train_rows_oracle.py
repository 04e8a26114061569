"""tests/train_rows_oracle.py pinned with no kernel: each reference against an independent evaluation (fp64 autograd of torch.nn.functional, torch.optim.AdamW in
fp64), a plain fp32 evaluation of each formula inside its bar on every case (the worst ratio printed: the measurement the bars' constants rest on), reference-side
mutants that must EXCEED the bar on a named case each, the keep rate of the mask restatement, the exactness of the integer-grid cases, and the boundary at which
amds_colsum's four-accumulator row lanes part ways with a plain in-order sum (rows 1 .. 48 agree, 49 does not): what include/amdstamp.h states for
amds_sum_partials_multi."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_rows_oracle as O

F64, F32 = torch.float64, torch.float32


def _close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert a.shape == b.shape and float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


def _ratio(what, got, want, bar):
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bar)
    worst = float(r.max())
    print(f"trainrows-cpu| {what} | fp32 on the CPU / bar = {worst:.3f}")
    return worst


# ---- the references against independent evaluations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(5, 4), (7, 516), (3, 2048)])
def test_layernorm_against_fp64_autograd(rows, cols):
    x, gamma, beta, dy, skip = (t.double() for t in O.ln_inputs(rows, cols))
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.layer_norm(xr, (cols,), gr, br, O.LN_EPS)
    y.backward(dy)
    f = O.layernorm_fwd(x, gamma, beta)
    _close(f["y"], y.detach())
    _close(f["mean"], x.mean(-1))
    _close(f["rstd"], 1 / torch.sqrt(x.var(-1, unbiased=False) + O.LN_EPS), 1e-9)          # (torch's two-pass variance on the mean-1e4 row)
    b = O.layernorm_bwd(dy, x, f["mean"], f["rstd"], gamma, skip)                          # fp64 statistics: the autograd gradient
    _close(b["dx"], skip + xr.grad, 1e-9)
    _close(b["t_gamma"].sum(0), gr.grad, 1e-9)
    _close(b["t_beta"].sum(0), br.grad)
    part, _ = O.ln_param_partials(b["t_gamma"])
    _close(O.ln_param_finish(part, torch.zeros_like(part), old=gamma)[0], gamma + gr.grad, 1e-9)
    assert bool((f["rstd"][1::5] == 1 / np.sqrt(O.LN_EPS)).all())                           # the constant rows: variance exactly 0


def test_gelu_against_fp64_autograd():
    z = torch.cat([torch.linspace(-12, 12, 4001, dtype=F64), torch.randn(4000, generator=O._gen(9), dtype=F64) * 3])
    zr = z.clone().requires_grad_(True)
    y = F.gelu(zr)
    y.sum().backward()
    _close(O.gelu(z)[0], y.detach(), 1e-15)
    _close(O.gelu_grad(z)[0], zr.grad, 1e-15)
    assert float(O.gelu(torch.tensor([float("inf")]))[0]) == float("inf") and bool(torch.isnan(O.gelu(torch.tensor([float("-inf")]))[0]).all())
    _close(O.relu(z), F.relu(z))


@pytest.mark.parametrize("name,hyper,step,fresh", O.ADAM_CASES)
def test_adamw_against_torch_optim(name, hyper, step, fresh):
    p, g, m, v = (t.double() for t in O.adam_inputs(1000, fresh))
    h = {k: O.f32(a) for k, a in hyper.items()}
    q = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([q], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    q.grad = g.clone()
    opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    opt.step()
    r = O.adamw(p, g, m, v, t=step, **hyper)
    _close(r["p"], q.detach(), 1e-13)
    _close(r["m"], opt.state[q]["exp_avg"], 1e-15)
    _close(r["v"], opt.state[q]["exp_avg_sq"], 1e-15)
    _close(r["p"], p * (1 - h["lr"] * h["wd"]) + r["upd"], 1e-15)


# ---- a plain fp32 evaluation of each formula sits inside its bar ------------------------------------------------------------------------------------------------------
def test_fp32_colsum_inside_the_bar():
    worst = 0.0
    for M in O.COLSUM_M:
        x = O.colsum_inputs(M, 130, "real")
        val, ab = O.colsum(x)
        worst = max(worst, _ratio(f"colsum M={M}", x.sum(0), val, O.colsum_bar(M, ab)),
                    _ratio(f"colsum M={M} in sequence", torch.from_numpy(np.cumsum(x.numpy(), 0, dtype=np.float32)[-1]), val, O.colsum_bar(M, ab)))
    assert worst < 1.0


def _ln_fwd32(x, gamma, beta):
    mean = x.sum(-1, keepdim=True) / x.shape[-1]
    d = x - mean
    rstd = 1 / torch.sqrt((d * d).sum(-1, keepdim=True) / x.shape[-1] + F32_EPS)
    return d * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


F32_EPS = torch.tensor(O.LN_EPS, dtype=F32)


@pytest.mark.parametrize("cols", O.LN_COLS)
def test_fp32_layernorm_inside_the_bars(cols):
    x, gamma, beta, dy, skip = O.ln_inputs(130, cols)
    f = O.layernorm_fwd(x, gamma, beta)
    y, mean, rstd = _ln_fwd32(x, gamma, beta)
    worst = max(_ratio(f"ln y cols={cols}", y, f["y"], f["d_y"]), _ratio(f"ln mean cols={cols}", mean, f["mean"], f["d_mean"]),
                _ratio(f"ln rstd cols={cols}", rstd, f["rstd"], f["d_rstd"]))
    m32, r32 = O.ln_stats32(x)
    b = O.layernorm_bwd(dy, x, m32, r32, gamma, skip)
    xhat = (x - m32[:, None]) * r32[:, None]
    g = dy * gamma
    s1, s2 = g.sum(-1, keepdim=True) / cols, (g * xhat).sum(-1, keepdim=True) / cols
    dx = skip + r32[:, None] * (g - s1 - xhat * s2)
    worst = max(worst, _ratio(f"ln dx cols={cols}", dx, b["dx"], b["d_dx"]))
    for key, terms32 in (("t_gamma", dy * xhat), ("t_beta", dy)):
        part, pbar = O.ln_param_partials(b[key])
        p32 = torch.stack([terms32[i:i + 64].sum(0) for i in range(0, 130, 64)])
        worst = max(worst, _ratio(f"ln {key} partials cols={cols}", p32, part, pbar))
        val, bar = O.ln_param_finish(part, pbar, old=gamma)
        worst = max(worst, _ratio(f"ln {key} finish cols={cols}", gamma + p32.sum(0), val, bar))
    assert worst < 1.0


def test_fp32_gelu_inside_the_bars_and_how_far():
    """The issue's measurement: the kernel's formula in plain fp32 sits near 0.09 of both bars over [-12, 12] plus N(0, 9) samples, torch's fp32 gelu near 0.25 of the
    forward bar.  Asserted at 0.25 / 0.5: a bar that an honest evaluation uses up has stopped telling a wrong constant from rounding."""
    z = torch.cat([torch.linspace(-12, 12, 200001), torch.randn(200000, generator=O._gen(10)) * 3])
    val, bar = O.gelu(z)
    own = 0.5 * z * (1.0 + torch.erf(z * O.INV_SQRT2))
    r_own, r_torch = _ratio("gelu, the kernel's formula", own, val, bar), _ratio("gelu, torch.nn.functional", F.gelu(z), val, bar)
    dval, dbar = O.gelu_grad(z)
    d = 0.5 * (1.0 + torch.erf(z * O.INV_SQRT2)) + z * O.INV_SQRT2PI * torch.exp(-0.5 * z * z)
    r_d = _ratio("gelu', the kernel's formula", d, dval, dbar)
    assert r_own < 0.25 and r_d < 0.25 and r_torch < 0.5, (r_own, r_d, r_torch)


@pytest.mark.parametrize("name,hyper,step,fresh", O.ADAM_CASES)
def test_fp32_adamw_inside_the_bars(name, hyper, step, fresh):
    p, g, m, v = O.adam_inputs(1 << 16, fresh)
    r = O.adamw(p, g, m, v, t=step, **hyper)
    lr, b1, b2, eps, wd = (torch.tensor(hyper[k], dtype=F32) for k in ("lr", "b1", "b2", "eps", "wd"))
    bc1, bc2 = 1 - torch.pow(b1, float(step)), 1 - torch.pow(b2, float(step))
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    p2 = p * (1 - lr * wd) - (lr / bc1) * m2 / (torch.sqrt(v2) / torch.sqrt(bc2) + eps)
    worst = max(_ratio(f"adamw p, {name}", p2, r["p"], r["d_p"]), _ratio(f"adamw m, {name}", m2, r["m"], r["d_m"]), _ratio(f"adamw v, {name}", v2, r["v"], r["d_v"]))
    assert worst < 1.0


# ---- reference-side mutants exceed the bar on a named case each -----------------------------------------------------------------------------------------------------
def _exceeds(mutant, want, bar):
    return bool(((mutant - want).abs() > bar).any())


def test_mutant_a_dropped_row_or_column_tail():
    """colsum real M=65 N=130 (the 65th row is the tail of the 16 row lanes; columns 128, 129 the scalar branch) and grid M=2049 (the last chunk is ONE row)."""
    for family, M in (("real", 65), ("grid", 2049)):
        x = O.colsum_inputs(M, 130, family)
        val, ab = O.colsum(x)
        bar = O.colsum_bar(M, ab) if family == "real" else torch.zeros_like(val)
        assert _exceeds(O.colsum(x[:-1])[0], val, bar), (family, M)
        tail = x.clone()
        tail[:, 128:] = 0
        assert _exceeds(O.colsum(tail)[0], val, bar) and not _exceeds(O.colsum(tail)[0][:128], val[:128], bar[:128])
    x, gamma, beta, dy, skip = O.ln_inputs(5, 516)                      # LayerNorm cols=516: column 512 .. 515 are the second float4 slot's only lane
    f = O.layernorm_fwd(x, gamma, beta)
    cut = x.clone().double()
    cut[:, 512:] = 0
    mean_cut = cut.sum(-1) / 516
    assert _exceeds(mean_cut, f["mean"], f["d_mean"])


def test_mutant_b_s1_without_the_division():
    for rows, cols in ((5, 4), (5, 2048)):
        x, gamma, beta, dy, skip = O.ln_inputs(rows, cols)
        m32, r32 = O.ln_stats32(x)
        b = O.layernorm_bwd(dy, x, m32, r32, gamma, skip)
        xhat = (x.double() - m32.double()[:, None]) * r32.double()[:, None]
        g = dy.double() * gamma.double()
        s1, s2 = g.sum(-1, keepdim=True), (g * xhat).sum(-1, keepdim=True) / cols          # s1 NOT divided
        assert _exceeds(skip.double() + r32.double()[:, None] * (g - s1 - xhat * s2), b["dx"], b["d_dx"]), (rows, cols)


def test_mutant_c_gelu_constant():
    z, _ = O.gelu_inputs(4096, F32)
    z = z[torch.isfinite(z)]
    val, bar = O.gelu_grad(z)
    assert _exceeds(O.gelu_grad(z, const=0.4)[0], val, bar)
    # and the forward bar tells 0.7071 from 0.7071068 (erf's argument)
    fval, fbar = O.gelu(z)
    assert _exceeds(0.5 * z.double() * (1 + torch.erf(z.double() * 0.7071)), fval, fbar)


def _keep_variant(seed, stream, idx, thr, pair=None, swap=False):
    idx = O._u64(idx)
    key = O.drop_rowkey(seed, stream, idx >> np.uint64(16))
    pr = (idx >> np.uint64(1)) if pair == "unmasked" else ((idx & np.uint64(0xFFFF)) >> np.uint64(1))
    odd = idx & np.uint64(1)
    return O.drop_keep(O.drop_pair_bits(key, pr), (odd ^ np.uint64(1)) if swap else odd, thr)


def test_mutants_d_e_pair_index_and_halves():
    """n = 65 536 + 8, p = 0.5: without `& 0xFFFF` the second mask row's pairs are 32768 + j instead of j; with the halves swapped every pair changes."""
    idx = np.arange(65536 + 8, dtype=np.int64)
    thr = O.drop_thr16(0.5)
    true = O.keep_flat(5, 3, idx, thr)
    assert np.array_equal(true, _keep_variant(5, 3, idx, thr))
    unmasked = _keep_variant(5, 3, idx, thr, pair="unmasked")
    assert np.array_equal(unmasked[:65536], true[:65536]) and not np.array_equal(unmasked[65536:], true[65536:])
    assert not np.array_equal(_keep_variant(5, 3, idx, thr, swap=True)[:8], true[:8])


def test_mutant_f_threshold_by_truncation():
    """p = 2^-17 (p * 65536 = 0.5: lroundf gives 1, truncation 0) and p = 0.1 (6553.6 -> 6554 / 6553): the keep scale moves by 1.5e-5 / 1.7e-5 of itself, 250 times
    the one rounding ReLU's bar allows."""
    assert [O.drop_thr16(p) for p in O.DROP_RATES] == [0, 1, 6554, 16384, 32768, 65535]
    assert O.drop_thr16(1.0 - 2.0 ** -24) == 65535                      # capped
    for p in (2.0 ** -17, 0.1):
        thr, trunc = O.drop_thr16(p), int(np.float32(p) * np.float32(65536.0))
        assert trunc == thr - 1
        x = torch.tensor([1.0, 3.0, 7.0], dtype=F64)
        want = x * O.drop_scale(thr)
        assert _exceeds(x * O.drop_scale(trunc), want, O.U * want.abs())
    assert [O.scale_is_pow2(p) for p in O.DROP_RATES] == [True, False, False, False, True, True]
    assert O.drop_scale(32768) == 2.0 and O.drop_scale(65535) == 65536.0 and O.drop_scale(0) == 1.0


def test_mutant_g_bias_correction_by_all_steps():
    """step 5 after 2 skipped steps: t = 3 applied steps."""
    p, g, m, v = O.adam_inputs(1000, False)
    r = O.adamw(p, g, m, v, t=3, **O.ADAM_HYPER)
    assert _exceeds(O.adamw(p, g, m, v, t=5, **O.ADAM_HYPER)["p"], r["p"], r["d_p"])


def test_mutant_h_decay_after_the_update():
    name, hyper, step, fresh = O.ADAM_CASES[2]
    p, g, m, v = O.adam_inputs(1000, fresh)
    r = O.adamw(p, g, m, v, t=step, **hyper)
    assert _exceeds(O.adamw(p, g, m, v, t=step, decay_after=True, **hyper)["p"], r["p"], r["d_p"]), name


# ---- the mask restatement --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", O.DROP_RATES)
def test_keep_rate_within_4_sigma(p):
    n = 1 << 20
    thr = O.drop_thr16(p)
    q = 1 - thr / 65536
    sigma = (n * q * (1 - q)) ** 0.5
    for seed, stream, start in ((5, 3, 0), (0xDEADBEEF12345678, 77, 1 << 40)):
        kept = int(O.keep_flat(seed, stream, start + np.arange(n, dtype=np.int64), thr).sum())
        assert abs(kept - n * q) <= 4 * sigma + 1e-9, (p, kept, n * q, sigma)
    kept = int(O.keep_rows(9, 1, np.arange(4096, dtype=np.int64)[:, None], np.arange(256, dtype=np.int64)[None, :], thr).sum())
    assert abs(kept - n * q) <= 4 * sigma + 1e-9


def test_row_form_is_the_flat_form_at_65536_columns_and_the_high_word_counts():
    thr = O.drop_thr16(0.25)
    idx = (3 << 16) + np.arange(300, dtype=np.int64)
    assert np.array_equal(O.keep_flat(7, 2, idx, thr), O.keep_rows(7, 2, 3, np.arange(300, dtype=np.int64), thr))
    lo = O.keep_rows(7, 2, 5, np.arange(4096, dtype=np.int64), thr)
    assert not np.array_equal(lo, O.keep_rows(7, 2, 5 + (1 << 32), np.arange(4096, dtype=np.int64), thr))          # row >> 32 enters the key
    assert not np.array_equal(lo, O.keep_rows(7 + (1 << 32), 2, 5, np.arange(4096, dtype=np.int64), thr))          # so does seed >> 32


def test_half_ulp_is_the_rounding_of_the_cast():
    x32 = torch.cat([torch.randn(100000, generator=O._gen(11)) * 3, torch.tensor([1.00390625, 2.0 ** -20, 2.0 ** -26, 0.0])])          # fp32 values: ONE rounding to 16 bits
    x = x32.double()
    for dt in (torch.bfloat16, torch.float16):
        err, h = (x32.to(dt).double() - x).abs(), O.half_ulp(x, dt)
        assert bool((err <= h).all()) and float((err / h.clamp_min(1e-300)).max()) > 0.99
    assert float(O.half_ulp(torch.tensor([1.5], dtype=F64), torch.bfloat16)) == 2.0 ** -8 and float(O.half_ulp(torch.tensor([0.0], dtype=F64), torch.float16)) == 2.0 ** -25


# ---- the integer-grid cases are exact in fp32 ------------------------------------------------------------------------------------------------------------------
def test_grid_cases_are_exact():
    for M in O.COLSUM_M:
        x = O.colsum_inputs(M, 130, "grid")
        O.assert_exact(O.colsum(x, old=torch.full((130,), 8.0))[1])
        assert torch.equal(x, x.bfloat16().float()) and torch.equal(x, x.half().float())
    for rows in O.LN_BWD_ROWS:
        dy = O.ln_inputs(rows, 4, "grid")[3]
        O.assert_exact(dy.abs().sum(0) + 8)
        assert torch.equal(dy, dy.round())
    z, du = O.gelu_inputs(64, torch.bfloat16, "grid")
    assert torch.equal(z.float(), z.float().round()) and bool((z.float() < 0).any()) and bool((z.float() == 0).sum() >= 2)


# ---- 49 rows: where four accumulators per row lane stop being a plain in-order sum ----------------------------------------------------------------------------------
def test_the_two_lane_orders_agree_up_to_48_rows_and_differ_at_49():
    g = np.random.default_rng(12)
    for rows in range(1, 49):
        x = g.standard_normal((rows, 200)).astype(np.float32)
        assert np.array_equal(O.colsum_lane_order(x), O.sequential_lane_order(x)), rows
    x = g.standard_normal((49, 200)).astype(np.float32)
    assert not np.array_equal(O.colsum_lane_order(x), O.sequential_lane_order(x))
    for rows in (49, 64, 200, 2048):          # both stay inside the column-sum bar
        x = g.standard_normal((rows, 200)).astype(np.float32)
        val, ab = O.colsum(torch.from_numpy(x))
        for f in (O.colsum_lane_order, O.sequential_lane_order):
            assert not _exceeds(torch.from_numpy(f(x)).double(), val, O.colsum_bar(rows, ab))
