"""Plain fp64 references of the training row kernels (stamp_amd/csrc/train.hip) and the element-wise dropout sites (stamp_amd/csrc/dropout.hip), the inputs of
their direct tests and the bars those tests hold the kernels to (test_cpu_train_rows_oracle.py pins this file to independent evaluations;
test_gpu_train_rows.py holds the kernels to it).  torch / numpy on the CPU; nothing here shares code with the kernels.

Every reference returns `(value, abs_terms)`: `abs_terms` is the same expression on |operands|, element by element -- what a rounding bound scales with.
Bars are PER ELEMENT.  Units: EPS = 2^-23 (one ulp of fp32 at 1), U = 2^-24 (one rounding).

How the bars are counted
  column sums     (M + 2) EPS sum|x| per column: a sum of M fp32 terms in ANY order is within (M - 1) U sum|x|; the bar keeps the form of
                  nystrom_oracle.sum_bar (twice that, and two terms of slack).
  LayerNorm fwd   mean   = a sum of `cols` terms and a division:            d_mean = (cols + 2) EPS sum|x| / cols
                  var    = a sum of `cols` squared deviations d = x - mean, each carrying the mean's error (2 |d| d_mean + d_mean^2) and three roundings
                           (the subtraction twice through the square, the square): d_var = (2 d_mean sum|d| + (cols + 2 + 3) EPS sum d^2) / cols + d_mean^2
                  rstd   = rsqrtf(var + eps): the addition and the division by cols (2 EPS of var + eps), half the relative error of its argument, and 8 EPS for
                           rsqrtf itself (the allowance softmax_rows_bar grants expf):  d_rstd = rstd (0.5 (d_var + 2 EPS (var + eps)) / (var + eps) + 8 EPS)
                  y      = (x - mean) rstd gamma + beta: the two input errors through the product, and three more operations of one EPS each on the
                           magnitude they round:  d_y = |gamma| (rstd d_mean + |d| d_rstd) + 3 EPS (|d rstd gamma| + |beta|)
                  16-bit y: + half an ulp of the output type AT the wanted value (`half_ulp`).
  LayerNorm bwd   takes the kernel's own fp32 mean / rstd inputs as given (the bar is about this kernel, not the forward).  xhat = (x - mean) rstd,
                  g = dy gamma, s1 = sum g / cols, s2 = sum g xhat / cols:  d_s1 = (cols + 2) EPS sum|g| / cols, d_s2 = (cols + 2) EPS sum|g xhat| / cols,
                  dx = skip + rstd (g - s1 - xhat s2):  d_dx = rstd (d_s1 + |xhat| d_s2) + 6 EPS rstd (|g| + |s1| + |xhat s2|) + EPS (|skip| + |dx|)
                  (six local roundings: g, xhat twice, xhat s2, the two subtractions -- the product with rstd and the skip add are the last term).
                  d(beta) / d(gamma) partials: sums of at most 64 rows, (64 + 2) EPS sum|terms|; their finish is the column-sum bar over the partials.
                  The 16-bit copy: d_dx times the mask multiplier, one EPS of the product with the scale, half an ulp of bf16 at the wanted value.
  GELU            forward 12 EPS 0.5 |x| (1 + |erf|); derivative EPS (11 * 0.5 (1 + |erf|) + (12 + x^2) |x phi(x)|) -- the x^2 term is __expf's argument error
                  (softmax_rows_bar).  A plain fp32 evaluation sits at 0.09 of both (test_cpu_train_rows_oracle.py asserts it): they reject a wrong constant and
                  pass an honest fp32 evaluation.  Under dropout: times the keep scale, one EPS per further product.  16-bit outputs: + half an ulp of the
                  output type at the wanted value, floor 2^-25 (half the smallest fp16 subnormal).  A 16-bit du is converted exactly.
  ReLU + dropout  exact: x * scale is one multiplication -- by a power of two (no rounding: bit for bit) when p gives one, else ONE rounding (U |want|), and for
                  a 16-bit output the rounding to it (half an ulp at the wanted value).
  AdamW           on the update upd = p_new - p_old (1 - lr wd):  |upd| (r1 + r2 / 2 + 8 EPS) + 2 EPS |p|,  r_i = 3 U / bc_i  (the host's 1 - powf(beta, step):
                  at step 1 with beta2 = 0.999 that alone is 1.8e-4 relative); m and v: 3 roundings of their terms, 3 U (|b m| + |(1 - b) g|).
                  The reference is evaluated on the fp32 VALUES of lr, betas, eps, wd: the parameters' own rounding is not the kernel's.

`half_ulp`: the issue behind these tests words the 16-bit allowance as "half an ulp of bf16 (2^-9 |want|)".  Half an ulp of bf16 at w is 2^(floor(log2 |w|) - 8),
which lies between 2^-9 |w| and 2^-8 |w|: a correctly rounded cast of 1.0039 errs by 2^-8.  The bars use the exact half ulp at the wanted value -- never more
than the rounding itself can cost, and what "half an ulp" says; 2^-9 |w| would fail a correct cast.

Two input families (`family` = "grid" | "real"):
* grid -- small integers (|x| <= 8, exact in fp32, bf16 and fp16): every partial sum is an integer and, while `abs_sum < 2^24` (`assert_exact`), exactly representable
  in fp32 in ANY summation order.  Column sums, d(beta), dropout_add / cast_bwd at power-of-two keep scales and ReLU must equal fp64 BIT FOR BIT on every route.
* real -- Gaussian operands at the model's magnitudes plus planted edges: LayerNorm rows (row % 5: 1 a constant row -- variance 0, rstd = 1 / sqrt(eps); 2 mean 1e4 and
  unit spread; 3 one spike of 90; 4 scale 1e-4 against eps 1e-5), GELU z (a grid over [-12, 12], +-0, +-inf, bf16's largest finite value).

The dropout mask: a numpy restatement of the rule as include/amdstamp.h and DESIGN.md describe it (`drop_*` below), flat and (row, k) forms.  Every mask of the GPU
tests comes from here; the library's own mask entries are held to it bit for bit."""
from __future__ import annotations

import math

import numpy as np
import torch

F64 = torch.float64
EXACT = 2.0 ** 24
EPS = 2.0 ** -23
U = 2.0 ** -24
LN_EPS = 1e-5
BF16_MAX = 3.3895313892515355e38          # 0x7F7F


def f32(x):
    """The fp32 value of a host scalar, as a Python float."""
    return float(np.float32(x))


def sum_bar(n_terms, abs_sum):
    return (n_terms + 2) * EPS * abs_sum


def assert_exact(abs_sum, unit=1.0):
    """The grid family's condition: every partial sum is a multiple of `unit` below 2^24 units."""
    worst = float(torch.as_tensor(abs_sum).max()) / unit
    assert worst < EXACT, worst


def half_ulp(want, dtype):
    """Half a unit in the last place of `dtype` at the wanted value (fp64 tensor), 0 for fp32 outputs.  Below the normal range the spacing is the subnormal quantum:
    2^-25 is half of fp16's, the floor the GELU bars name."""
    if dtype == torch.float32:
        return torch.zeros_like(want)
    prec, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    w = torch.where(torch.isfinite(want), want.abs(), torch.zeros_like(want))
    _, ex = torch.frexp(w)                                  # w = m 2^ex, m in [0.5, 1): floor(log2 w) = ex - 1
    e = torch.where(w > 0, torch.clamp(ex.to(torch.int64) - 1, min=emin), torch.full_like(ex, emin, dtype=torch.int64))
    return torch.ldexp(torch.ones_like(w), (e - prec).to(torch.int32))


def saturate(want, dtype):
    """The wanted value as `dtype` can hold it: round-to-nearest sends everything from the largest finite value plus half its ulp upwards to infinity (a kept GELU
    of 12 times the keep scale 65536 of p = 0.99999 leaves fp16's range; bf16's largest value times 4/3 leaves fp32's)."""
    big, half = {torch.float32: (3.4028234663852886e38, 2.0 ** 103), torch.bfloat16: (BF16_MAX, 2.0 ** 119), torch.float16: (65504.0, 16.0)}[dtype]
    inf = torch.full_like(want, float("inf"))
    return torch.where(want >= big + half, inf, torch.where(want <= -(big + half), -inf, want))


# ==== the dropout mask rule ====================================================================================================================================
# A tensor's flat element index idx is cut into rows of 65 536 elements: row = idx >> 16, pair = (idx & 0xFFFF) >> 1, the odd element of a pair takes the high
# 16 bits of the pair's 32 hash bits, the even one the low 16.  keep <=> those 16 bits >= thr, thr = lroundf(p * 65536) capped at 65 535; kept values are
# multiplied by 65536 / (65536 - thr) (fp32).  Attention probabilities: row = the probability row, pair = k >> 1.
_M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x, dtype=np.int64).astype(np.uint64)


def _mul32(a, c):
    return (a * np.uint64(c)) & _M32


def _fmix32(h):
    h = h ^ (h >> np.uint64(16))
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> np.uint64(13))
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> np.uint64(16))


def drop_rowkey(seed, stream, row):
    """Two murmur3 finalisers over (seed, stream, row), the high words of seed and row entering the second."""
    row = _u64(row)
    lo = np.uint64(seed & 0xFFFFFFFF) ^ (row & _M32) ^ np.uint64((stream * 0x9E3779B1) & 0xFFFFFFFF)
    a = _fmix32(lo)
    return _fmix32((a + np.uint64((seed >> 32) & 0xFFFFFFFF) + _mul32(row >> np.uint64(32), 0x7FEB352D)) & _M32)


def drop_mix(h):
    h = h ^ (h >> np.uint64(16))
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> np.uint64(16))


def drop_pair_bits(rowkey, pair):
    return drop_mix(rowkey ^ _mul32(_u64(pair), 0x9E3779B1))


def drop_keep(pair_bits, odd, thr16):
    shift = np.where(np.asarray(odd, dtype=bool), np.uint64(16), np.uint64(0))
    return ((pair_bits >> shift) & np.uint64(0xFFFF)) >= np.uint64(thr16)


def drop_thr16(p):
    t = float(np.float32(p) * np.float32(65536.0))
    r = int(math.floor(abs(t) + 0.5)) * (1 if t >= 0 else -1)          # lroundf: halves away from zero
    return min(max(r, 0), 65535)


def drop_scale(thr16):
    return float(np.float32(65536.0) / np.float32(65536 - thr16))


def keep_flat(seed, stream, idx, thr16):
    """Keep bits (bool) of the flat element indices `idx` (any integer array, < 2^63)."""
    idx = _u64(idx)
    key = drop_rowkey(seed, stream, idx >> np.uint64(16))
    return drop_keep(drop_pair_bits(key, (idx & np.uint64(0xFFFF)) >> np.uint64(1)), idx & np.uint64(1), thr16)


def keep_rows(seed, stream, row, k, thr16):
    """Keep bits of elements (row, k) of attention probabilities: the row is the key."""
    row, k = np.broadcast_arrays(_u64(row), _u64(k))
    return drop_keep(drop_pair_bits(drop_rowkey(seed, stream, row), k >> np.uint64(1)), k & np.uint64(1), thr16)


def mult_flat(seed, stream, idx, p):
    """The multiplier (0 or the fp32 keep scale) of each flat index, fp64 tensor; p = 0 keeps everything at 1."""
    thr = drop_thr16(p)
    keep = keep_flat(seed, stream, idx, thr)
    return torch.from_numpy(keep.astype(np.float64) * drop_scale(thr))


def mult_rows(seed, stream, rows, cols, p):
    thr = drop_thr16(p)
    keep = keep_rows(seed, stream, np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :], thr)
    return torch.from_numpy(keep.astype(np.float64) * drop_scale(thr))


def scale_is_pow2_value(scale):
    return math.frexp(scale)[0] == 0.5


def scale_is_pow2(p):
    return scale_is_pow2_value(drop_scale(drop_thr16(p)))


DROP_RATES = (0.0, 2.0 ** -17, 0.1, 0.25, 0.5, 0.99999)          # thr 0, 1 (0.5 rounds up), 6554 (6553.6), 16384, 32768, 65535


# ==== column sums ================================================================================================================================================
def colsum(x, old=None):
    x = x.to(F64)
    val, ab = x.sum(0), x.abs().sum(0)
    if old is not None:
        val, ab = val + old.to(F64), ab + old.to(F64).abs()
    return val, ab


def colsum_bar(M, abs_sum):
    return sum_bar(M, abs_sum)


# ==== LayerNorm ==================================================================================================================================================
def layernorm_fwd(x, gamma, beta, eps=LN_EPS):
    """-> dict: y, mean, rstd (fp64) and the bars d_y, d_mean, d_rstd (module docstring)."""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    cols = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = d * rstd * gamma + beta
    d_mean = (cols + 2) * EPS * x.abs().sum(-1, keepdim=True) / cols
    d_var = (2 * d_mean * d.abs().sum(-1, keepdim=True) + (cols + 5) * EPS * (d * d).sum(-1, keepdim=True)) / cols + d_mean ** 2
    d_rstd = rstd * (0.5 * (d_var + 2 * EPS * (var + eps)) / (var + eps) + 8 * EPS)
    d_y = gamma.abs() * (rstd * d_mean + d.abs() * d_rstd) + 3 * EPS * ((d * rstd * gamma).abs() + beta.abs())
    return dict(y=y, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), d_y=d_y, d_mean=d_mean.squeeze(-1), d_rstd=d_rstd.squeeze(-1))


def layernorm_bwd(dy, x, mean, rstd, gamma, skip=None):
    """mean, rstd: the fp32 values the kernel is handed.  -> dict: dx, d_dx, and the per-row terms of the parameter gradients t_gamma = dy xhat, t_beta = dy
    (the 64-row partials and their finish are sums of these: `ln_param_partials`)."""
    dy, x, gamma = dy.to(F64), x.to(F64), gamma.to(F64)
    mu, rs = mean.to(F64).unsqueeze(-1), rstd.to(F64).unsqueeze(-1)
    cols = x.shape[-1]
    xhat = (x - mu) * rs
    g = dy * gamma
    s1 = g.sum(-1, keepdim=True) / cols
    s2 = (g * xhat).sum(-1, keepdim=True) / cols
    core = rs * (g - s1 - xhat * s2)
    sk = torch.zeros_like(core) if skip is None else skip.to(F64)
    dx = sk + core
    d_s1 = (cols + 2) * EPS * g.abs().sum(-1, keepdim=True) / cols
    d_s2 = (cols + 2) * EPS * (g * xhat).abs().sum(-1, keepdim=True) / cols
    d_dx = rs * (d_s1 + xhat.abs() * d_s2) + 6 * EPS * rs * (g.abs() + s1.abs() + (xhat * s2).abs()) + EPS * (sk.abs() + dx.abs())
    return dict(dx=dx, d_dx=d_dx, t_gamma=dy * xhat, t_beta=dy)


def ln_param_partials(terms):
    """[rows, cols] per-row terms -> the [ceil(rows / 64), cols] block sums and their bar (sums of at most 64 rows)."""
    rows, cols = terms.shape
    nblk = (rows + 63) // 64
    pad = torch.zeros(nblk * 64 - rows, cols, dtype=F64)
    t = torch.cat([terms, pad]).view(nblk, 64, cols)
    return t.sum(1), sum_bar(64, t.abs().sum(1))


def ln_param_finish(part, part_bar, old=None):
    """The column sum of the partials (+ the old value under accumulate_params): value, bar = the partials' bars summed + the column-sum bar of the finish."""
    val, ab = colsum(part, old)
    return val, part_bar.sum(0) + colsum_bar(part.shape[0] + (old is not None), ab)


# ==== GELU, its derivative, ReLU ==================================================================================================================================
INV_SQRT2 = 0.70710678118654752440
INV_SQRT2PI = 0.39894228040143267794


def gelu(x):
    x = x.to(F64)
    erf = torch.erf(x * INV_SQRT2)
    return 0.5 * x * (1.0 + erf), 12 * EPS * 0.5 * x.abs() * (1.0 + erf.abs())


def gelu_grad(x, const=INV_SQRT2PI):
    """gelu'(x) = Phi(x) + x phi(x) -> (value, bar); x phi(x) is 0 where phi underflows (x = +-inf included: the kernel's 0 * inf there is a NaN, `nonfinite`)."""
    x = x.to(F64)
    erf = torch.erf(x * INV_SQRT2)
    xphi = x * const * torch.exp(-0.5 * x * x)
    val = 0.5 * (1.0 + erf) + xphi
    x2 = torch.where(torch.isfinite(x), x * x, torch.zeros_like(x))
    return val, EPS * (11 * 0.5 * (1.0 + erf.abs()) + (12 + x2) * xphi.abs())


def relu(x):
    x = x.to(F64)
    return torch.where(x > 0, x, torch.zeros_like(x))


# ==== AdamW ======================================================================================================================================================
def adamw(p, g, m, v, lr, b1, b2, eps, wd, t, decay_after=False):
    """One torch.optim.AdamW step (amsgrad=False) in fp64 on the fp32 values of the hyper-parameters, bias corrections for t applied steps.
    -> dict: p, m, v, upd = p_new - p_old (1 - lr wd) and the bars d_p, d_m, d_v.  decay_after: the mutant that decays the UPDATED parameter."""
    p, g, m, v = (a.to(F64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = (f32(a) for a in (lr, b1, b2, eps, wd))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    upd = -(lr / bc1) * m2 / (torch.sqrt(v2) / math.sqrt(bc2) + eps)
    pn = (p + upd) * (1.0 - lr * wd) if decay_after else p * (1.0 - lr * wd) + upd
    r1, r2 = 3 * U / bc1, 3 * U / bc2
    return dict(p=pn, m=m2, v=v2, upd=upd, d_p=upd.abs() * (r1 + r2 / 2 + 8 * EPS) + 2 * EPS * p.abs(),
                d_m=3 * U * ((b1 * m).abs() + ((1.0 - b1) * g).abs()), d_v=3 * U * ((b2 * v).abs() + (1.0 - b2) * g * g))


# ==== inputs =====================================================================================================================================================
def _gen(*key):
    seed = 29
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ints(g, shape, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


COLSUM_M = (1, 15, 16, 17, 48, 49, 63, 64, 65, 1024, 2048, 2049, 4097)
COLSUM_N = (1, 3, 4, 63, 64, 65, 130)
SUM_PARTIALS_ROWS = (1, 16, 17, 32, 48, 49, 64, 65, 200, 2048)


def colsum_inputs(M, N, family, dtype=torch.float32):
    """-> x [M, N] in `dtype` (the reference reads the rounded values)."""
    g = _gen(1, M, N)
    x = ints(g, (M, N)) if family == "grid" else torch.randn(M, N, generator=g) * 2
    return x.to(dtype)


LN_COLS = (4, 508, 512, 516, 1024, 1028, 2048)
LN_FWD_ROWS = (1, 3, 4, 5)
LN_BWD_ROWS = (1, 63, 64, 65, 130)


def ln_inputs(rows, cols, family="real"):
    """-> x, gamma, beta, dy, skip (fp32).  real: the planted rows of the module docstring; grid: the same x with an integer dy (d(beta) is then exact)."""
    g = _gen(2, rows, cols)
    x = torch.randn(rows, cols, generator=g) * 2 + 0.5
    for r in range(rows):
        kind = r % 5
        if kind == 1:
            x[r] = 1.75
        elif kind == 2:
            x[r] = 1e4 + torch.randn(cols, generator=g)
        elif kind == 3:
            x[r] = torch.randn(cols, generator=g)
            x[r, int(torch.randint(0, cols, (1,), generator=g))] = 90.0
        elif kind == 4:
            x[r] = torch.randn(cols, generator=g) * 1e-4
    gamma, beta = 1 + 0.2 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)
    dy = ints(g, (rows, cols)) if family == "grid" else torch.randn(rows, cols, generator=g)
    return x, gamma, beta, dy, torch.randn(rows, cols, generator=g)


def ln_stats32(x, eps=LN_EPS):
    """The fp32 mean / rstd a backward test hands the kernel: the fp64 statistics rounded once."""
    f = layernorm_fwd(x, torch.ones(x.shape[-1]), torch.zeros(x.shape[-1]), eps)
    return f["mean"].float(), f["rstd"].float()


def gelu_inputs(n, dtype, family="real"):
    """-> z, du in `dtype` (n >= 8).  real: a grid over [-12, 12] in the first half, N(0, 9) behind it, the planted values at the front (+-0, +-inf, bf16's largest
    finite value and its negative; as many as fit).  grid: integers in [-8, 8] (ReLU's exact family; +-0 and negatives among them)."""
    g = _gen(3, n)
    if family == "grid":
        z = ints(g, (n,))
        z[:2] = torch.tensor([0.0, -0.0])
        return z.to(dtype), ints(g, (n,)).to(dtype)
    z = torch.randn(n, generator=g) * 3
    half = n // 2
    z[:half] = torch.linspace(-12, 12, half)
    planted = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), BF16_MAX, -BF16_MAX])
    k = min(6, n - 2)
    z[1:1 + k] = planted[:k]
    return z.to(dtype), torch.randn(n, generator=g).to(dtype)


def adam_inputs(n, fresh):
    """-> p, g, m, v (fp32); fresh: the first step's zero moments."""
    gen = _gen(4, n, fresh)
    p = torch.randn(n, generator=gen)
    m = torch.zeros(n) if fresh else torch.randn(n, generator=gen) * 1e-3
    v = torch.zeros(n) if fresh else torch.rand(n, generator=gen) * 1e-5
    return p, torch.randn(n, generator=gen) * 1e-2, m, v


ADAM_HYPER = dict(lr=3e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)
# (name, hyper-parameters, step, fresh moments).  "strong decay": lr wd = 1e-3 of the update stands far above the bar, so the order of decay and update shows
# (at the trainers' lr = 3e-4, wd = 0.01 the two orders differ by 3e-6 of the update, below one rounding of p).
ADAM_CASES = (("first step", ADAM_HYPER, 1, True), ("step 7", ADAM_HYPER, 7, False),
              ("strong decay, step 1000", dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.1), 1000, False))


# ==== the two summation orders of a column of partial rows (the boundary include/amdstamp.h states for amds_sum_partials_multi) =====================================
def colsum_lane_order(x):
    """fp32 emulation of amds_colsum's one-chunk vector path on columns x [rows, n]: 16 row lanes; lane k adds rows k, k + 16, k + 32, k + 48 of each 64-row
    step into four accumulators while a whole step is left, the rest into the first; (a0 + a1) + (a2 + a3); the lanes added in order."""
    x = np.asarray(x, dtype=np.float32)
    rows = x.shape[0]
    s = np.zeros(x.shape[1], np.float32)
    for k in range(16):
        acc = [np.zeros(x.shape[1], np.float32) for _ in range(4)]
        r = k
        while r + 48 < rows:
            for u in range(4):
                acc[u] = acc[u] + x[r + 16 * u]
            r += 64
        while r < rows:
            acc[0] = acc[0] + x[r]
            r += 16
        s = s + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
    return s


def sequential_lane_order(x):
    """The same 16 lanes, each adding ALL its rows r = k, k + 16, ... in sequence into one accumulator."""
    x = np.asarray(x, dtype=np.float32)
    s = np.zeros(x.shape[1], np.float32)
    for k in range(min(16, x.shape[0])):
        a = np.zeros(x.shape[1], np.float32)
        for r in range(k, x.shape[0], 16):
            a = a + x[r]
        s = s + a
    return s
