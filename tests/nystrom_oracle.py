"""Plain fp64 references of the Nystrom / TransMIL fp32 kernels of stamp_amd/csrc/transmil.hip, torch on the CPU, and the inputs of their direct tests
(test_cpu_nystrom_oracle.py pins this file to independent evaluations; test_gpu_nystrom_kernels.py holds the kernels to it).

Every reference returns `(value, abs_sum)`: `abs_sum` is the same expression evaluated on |operands|, element by element -- what a rounding bound of the
sum scales with (`sum_bar`).  Nothing here is written for speed, and nothing shares code with the kernels or with oracle/transmil.py.

Two input families per kernel (`family` = "grid" | "real"):

* grid -- small integers (weights in [-3, 3], activations in [-8, 8], scales a power of two, |x| integers for the pinv start).  Every product and every
  partial sum is then a multiple of the builder's `unit` and, while `abs_sum / unit < 2^24`, exactly representable in fp32 in ANY summation order, with or
  without fused multiply-adds: the kernel must give the fp64 value bit for bit (within a counted number of roundings behind a division).  A missing,
  doubled or misplaced term cannot hide in a rounding bound.  The softmax's grid rows hold a power-of-two count k of equal maxima and the rest 10^4 lower:
  exp(0) = 1 and exp(-10^4) = 0 in both precisions, p is 1 / k or 0.
* real -- Gaussian operands at the model's magnitudes plus the edges the issue names (a row shifted by 1e4, a spike of 90, an all-equal row, a descending
  row), held to the elementwise rounding bound."""
from __future__ import annotations

import torch
import torch.nn.functional as F

F64 = torch.float64
EXACT = 2.0 ** 24          # integers below this magnitude are exact in fp32
EPS = 2.0 ** -23


def sum_bar(n_terms, abs_sum):
    """A sum of n fp32 terms in any order lies within n * 2^-23 * sum|terms| of the exact sum (tests/test_gpu_abi_rows.py's `_sum_bar`), elementwise."""
    return (n_terms + 2) * EPS * abs_sum


# ---- packed [b][np][k * H * d] tensors and their head slices (the addressing of tests/chains/transmil.py) --------------------------------------------------
def head_slice(t, which, H, d):
    """t [b, np, k*H*d] -> the [b, H, np, d] head slices of its `which`-th [H*d] column block (a copy)."""
    b, n, _ = t.shape
    C = H * d
    return t[..., which * C:(which + 1) * C].reshape(b, n, H, d).permute(0, 2, 1, 3).contiguous()


def put_head_slice(t, which, H, d, val):
    """The inverse: writes val [b, H, np, d] into t's column block, in place."""
    b, n, _ = t.shape
    C = H * d
    t[..., which * C:(which + 1) * C] = val.permute(0, 2, 1, 3).reshape(b, n, C)
    return t


# ---- softmax ---------------------------------------------------------------------------------------------------------------------------------------------
def softmax_rows(x):
    x = x.to(F64)
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    return p, p


def softmax_rows_bar(x):
    """|got - p_j| <= p_j * (cols + 2 |x_j - max| + 8) * 2^-23, floor 2^-126: the row sum, the rounding of the exponent's argument (an error of 2^-24 |x_j - max|
    in the argument is that relative error of exp, twice for the subtraction and the range reduction), a few ulp for expf; below the normal range fp32 keeps an
    absolute precision only."""
    x = x.to(F64)
    p, _ = softmax_rows(x)
    rel = (x.shape[-1] + 2 * (x - x.max(-1, keepdim=True).values).abs() + 8) * EPS
    return torch.clamp(rel * p, min=2.0 ** -126)


def softmax_rows_bwd(p, dp):
    """p o (dp - sum_k p_k dp_k)"""
    p, dp = p.to(F64), dp.to(F64)
    s = (p * dp).sum(-1, keepdim=True)
    sa = (p * dp).abs().sum(-1, keepdim=True)
    return p * (dp - s), p.abs() * (dp.abs() + sa)


def softmax_rows_bwd_bar(p, dp):
    """2^-23 p_j ((cols + 3) sum_k |p_k dp_k| + 3 |dp_j|): the dot product in any order, the subtraction and the product; plus one subnormal quantum (2^-149),
    since a result below the normal range is rounded to that grid whatever the arithmetic before it did."""
    p, dp = p.to(F64), dp.to(F64)
    sa = (p * dp).abs().sum(-1, keepdim=True)
    return EPS * p.abs() * ((p.shape[-1] + 3) * sa + 3 * dp.abs()) + 2.0 ** -149


# ---- landmark means --------------------------------------------------------------------------------------------------------------------------------------
def landmark_mean(qkv, which, H, d, m, l, scale):
    """out[b, h, j, :] = scale * sum_{t < l} x[b, h, j*l + t, :] on the head slices of a packed tensor."""
    x = head_slice(qkv.to(F64), which, H, d)
    b = x.shape[0]
    x = x[:, :, :m * l].reshape(b, H, m, l, d)
    return x.sum(3) * scale, x.abs().sum(3) * abs(scale)


def landmark_mean_bwd(dout, dx0, which, H, d, m, l, scale, accumulate):
    """dx[b, h, j*l + t, :] (+)= scale * dout[b, h, j, :]; the rest of the packed tensor dx0 stays.  -> the whole packed tensor."""
    dout = dout.to(F64)
    b = dout.shape[0]
    g = (dout * scale).unsqueeze(3).expand(b, H, m, l, d).reshape(b, H, m * l, d)
    old = head_slice(dx0.to(F64), which, H, d)
    val = old + g if accumulate else g
    ab = old.abs() + g.abs() if accumulate else g.abs()
    return put_head_slice(dx0.to(F64).clone(), which, H, d, val), put_head_slice(dx0.to(F64).abs(), which, H, d, ab)


# ---- the depthwise sequence convolution --------------------------------------------------------------------------------------------------------------------
def _seq_windows(v, taps):
    pad = taps // 2
    return F.pad(v, (0, 0, pad, pad)).unfold(2, taps, 1)          # [b, H, n, d, taps]: v[t + k - pad]


def dwconv_seq(v, w, out0):
    """out[b, h, t, :] = out0 + sum_k w[h, k] v[b, h, t + k - pad, :]   (v, out0: [b, H, n, d]; w: [H, taps])"""
    v, w, out0 = v.to(F64), w.to(F64), out0.to(F64)
    H, taps = w.shape
    win = _seq_windows(v, taps)
    wv = w.view(1, H, 1, 1, taps)
    return out0 + (win * wv).sum(-1), out0.abs() + (win.abs() * wv.abs()).sum(-1)


def dwconv_seq_row(v, w, out0, row):
    """The same sum for one position: out0 [b, H, d]."""
    val, ab = dwconv_seq(v, w, torch.zeros_like(v, dtype=F64))
    return out0.to(F64) + val[:, :, row], out0.to(F64).abs() + ab[:, :, row]


def dwconv_seq_wgrad(dout, v, taps):
    """dw[h, k] = sum_{b, t, c} dout[b, h, t, c] v[b, h, t + k - pad, c]"""
    dout, v = dout.to(F64), v.to(F64)
    win = _seq_windows(v, taps)
    return torch.einsum("bhtc,bhtck->hk", dout, win), torch.einsum("bhtc,bhtck->hk", dout.abs(), win.abs())


# ---- PPEG ------------------------------------------------------------------------------------------------------------------------------------------------
def ppeg(x, w7, b7, w5, b5, w3, b3, Hh, Ww):
    """x [B, 1 + Hh*Ww, C]; y = x + dw7(x) + dw5(x) + dw3(x) + the three biases on the token grid (shift and add, tap by tap), class row copied.
    w_k: [C, k*k], tap (r, q) at r*k + q multiplies x[i + r - k//2][j + q - k//2]."""
    x = x.to(F64)
    B, _, C = x.shape
    img = x[:, 1:].reshape(B, Hh, Ww, C)
    xp, xa = F.pad(img, (0, 0, 3, 3, 3, 3)), F.pad(img.abs(), (0, 0, 3, 3, 3, 3))
    y = img + (b7.to(F64) + b5.to(F64) + b3.to(F64))
    ya = img.abs() + (b7.to(F64).abs() + b5.to(F64).abs() + b3.to(F64).abs())
    for w, k in ((w7, 7), (w5, 5), (w3, 3)):
        w, o = w.to(F64), 3 - k // 2
        for r in range(k):
            for q in range(k):
                y = y + w[:, r * k + q] * xp[:, o + r:o + r + Hh, o + q:o + q + Ww]
                ya = ya + w[:, r * k + q].abs() * xa[:, o + r:o + r + Hh, o + q:o + q + Ww]
    return torch.cat([x[:, :1], y.reshape(B, Hh * Ww, C)], 1), torch.cat([x[:, :1].abs(), ya.reshape(B, Hh * Ww, C)], 1)


def ppeg_wgrad(x, dy, Hh, Ww):
    """-> [50, C]: row r*7 + q = sum_{b, i, j} dy[b, i, j] x[b, i + r - 3, j + q - 3], row 49 = sum dy (class rows take no part)."""
    x, dy = x.to(F64), dy.to(F64)
    B, _, C = x.shape
    g = dy[:, 1:].reshape(B, Hh, Ww, C)
    xp = F.pad(x[:, 1:].reshape(B, Hh, Ww, C), (0, 0, 3, 3, 3, 3))
    rows, rows_a = [], []
    for r in range(7):
        for q in range(7):
            t = g * xp[:, r:r + Hh, q:q + Ww]
            rows.append(t.sum((0, 1, 2)))
            rows_a.append(t.abs().sum((0, 1, 2)))
    rows.append(g.sum((0, 1, 2)))
    rows_a.append(g.abs().sum((0, 1, 2)))
    return torch.stack(rows), torch.stack(rows_a)


# ---- the start of the pseudo-inverse iteration and its backward -----------------------------------------------------------------------------------------------
def pinv_init(x, group):
    """z = x^T / (max row-sum |x| * max column-sum |x|), the maxima over each `group` consecutive matrices.  x: [nmat, n, n]."""
    x = x.to(F64)
    nmat, n, _ = x.shape
    ax = x.abs()
    rmax = ax.sum(-1).reshape(nmat // group, group * n).max(1).values
    cmax = ax.sum(-2).reshape(nmat // group, group * n).max(1).values
    s = (rmax * cmax).repeat_interleave(group).view(nmat, 1, 1)
    z = x.transpose(-1, -2) / s
    return z, z.abs()


def _first_max(v):
    """(first flat index of the maximum, the maximum, second largest / largest)"""
    mx = v.max()
    idx = int((v == mx).nonzero()[0])
    rest = torch.cat([v[:idx], v[idx + 1:]])
    return idx, mx, (float(rest.max() / mx) if rest.numel() else 0.0)


def pinv_init_bwd_parts(x, dz, dx0):
    """The closed form of d(pinv_init with one group)/dx for x > 0:  dx = dx0 + dz^T / s + ds * cmax on the arg-max row + ds * rmax on the arg-max column,
    s = rmax * cmax, ds = -sum(dz^T o x) / s^2; the first flat index (matrix * n + row) wins a tie."""
    x, dz, dx0 = x.to(F64), dz.to(F64), dx0.to(F64)
    nmat, n, _ = x.shape
    ri, rmax, rratio = _first_max(x.abs().sum(-1).reshape(-1))
    ci, cmax, cratio = _first_max(x.abs().sum(-2).reshape(-1))
    s = rmax * cmax
    dzt = dz.transpose(-1, -2)
    dot, dot_abs = (dzt * x).sum(), (dzt * x).abs().sum()
    ds, ds_abs = -dot / s ** 2, dot_abs / s ** 2
    t_row, t_col = torch.zeros_like(x), torch.zeros_like(x)
    t_row.view(nmat * n, n)[ri] = 1.0
    t_col[ci // n, :, ci % n] = 1.0
    terms = [dx0, dzt / s, t_row * (ds * cmax), t_col * (ds * rmax)]
    terms_abs = [dx0.abs(), dzt.abs() / s, t_row * (ds_abs * cmax), t_col * (ds_abs * rmax)]
    return dict(value=sum(terms), abs_sum=sum(terms_abs), largest=torch.stack([t.abs() for t in terms]).max(0).values, row=ri, col=ci, rmax=float(rmax),
                cmax=float(cmax), s=float(s), dot_abs=float(dot_abs), row_margin=1.0 - rratio, col_margin=1.0 - cratio)


def pinv_init_bwd(x, dz, dx0):
    p = pinv_init_bwd_parts(x, dz, dx0)
    return p["value"], p["abs_sum"]


# ==== the cases and their inputs ===================================================================================================================================
# (shapes: the smallest that select each variant and straddle each boundary inside it; the table in test_gpu_nystrom_kernels.py's docstring maps them to kernels)
def _gen(*key):
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


SOFTMAX_COLS = (4, 252, 256, 260, 512, 516, 1024, 1028, 1280, 1284, 2048, 2052, 35, 1)
SOFTMAX_ROWS = (1, 5, 8)


def softmax_inputs(rows, cols, family):
    """-> x [rows, cols] fp32, unit [rows, 1] (grid) or None.  real: row r is, in turn, Gaussian x 3 | the same + 1e4 | Gaussian with one spike of 90 | all equal |
    descending by 0.25 per element."""
    g = _gen(1, rows, cols)
    if family == "grid":
        x = torch.empty(rows, cols)
        unit = torch.empty(rows, 1)
        for r in range(rows):
            k = 1
            while 2 * k <= max(1, cols // 2):
                k *= 2
            top = float(r - 3)
            x[r] = top - 1e4
            x[r, torch.randperm(cols, generator=g)[:k]] = top
            unit[r] = 1.0 / k
        return x, unit
    x = _randn(g, rows, cols) * 3
    for r in range(rows):
        kind = r % 5
        if kind == 1:
            x[r] += 1e4
        elif kind == 2:
            x[r] = _randn(g, cols)
            x[r, int(torch.randint(0, cols, (1,), generator=g))] = 90.0
        elif kind == 3:
            x[r] = 1.75
        elif kind == 4:
            x[r] = 2.0 - 0.25 * torch.arange(cols)
    return x, None


def softmax_bwd_inputs(rows, cols, family):
    """-> p, dp [rows, cols] fp32, unit.  grid: p in {0 .. 4} / 64, dp integers: every value a multiple of 2^-12.  real: p = the fp32 softmax of softmax_inputs' rows."""
    g = _gen(2, rows, cols)
    if family == "grid":
        return _ints(g, (rows, cols), 0, 4) / 64, _ints(g, (rows, cols), -8, 8), 2.0 ** -12
    x, _ = softmax_inputs(rows, cols, "real")
    return softmax_rows(x)[0].float(), _randn(g, rows, cols), None


LANDMARK_CASES = ((1, 1, 4), (35, 2, 8), (256, 5, 64), (7, 3, 6))          # (m, l, d); b = 2, H = 3, q's slices of a packed [b][m*l][3*H*d]
LANDMARK_B, LANDMARK_H = 2, 3


def landmark_inputs(m, l, d, family):
    """-> qkv [b, m*l, 3*H*d], dout [b, H, m, d], dx0 like qkv, scale, unit"""
    g = _gen(3, m, l, d)
    b, H = LANDMARK_B, LANDMARK_H
    shape = (b, m * l, 3 * H * d)
    if family == "grid":
        return _ints(g, shape, -8, 8), _ints(g, (b, H, m, d), -8, 8), _ints(g, shape, -8, 8), 0.25, 0.25
    return _randn(g, *shape), _randn(g, b, H, m, d), _randn(g, *shape), d ** -0.5 / l, None


DWCONV_B, DWCONV_H = 2, 3          # outer x inner = 2 x 3, every head its own taps
DWCONV_WIN_CASES = tuple((n, d, 33) for n in (1, 16, 17, 33, 127, 128, 129, 300) for d in (8, 64, 72))
DWCONV_GENERIC_CASES = tuple((n, d, taps) for taps in (1, 3, 31, 35) for n, d in ((70, 8), (129, 72)))
DWCONV_ROW_CASES = tuple((n, d) for n in (1, 10, 70) for d in (8, 72))
WGRAD_WIN_CASES = tuple((n, d, 33) for n in (1, 15, 16, 17, 63, 64, 65, 200) for d in (8, 64, 72, 130))
WGRAD_GENERIC_CASES = tuple((n, d, 31) for n in (17, 70) for d in (8, 64, 256, 24, 72, 320))


def dwconv_inputs(n, d, taps, family):
    """-> qkv [b, n, 3*H*d] (v = its third block's head slices), w [H, taps], merged [b, n, H*d] (the pre-filled output, and the wgrad's dout), unit"""
    g = _gen(4, n, d, taps)
    b, H = DWCONV_B, DWCONV_H
    if family == "grid":
        return _ints(g, (b, n, 3 * H * d), -8, 8), _ints(g, (H, taps), -3, 3), _ints(g, (b, n, H * d), -8, 8), 1.0
    return _randn(g, b, n, 3 * H * d), _randn(g, H, taps) * 0.2, _randn(g, b, n, H * d), None


PPEG_GRIDS = ((1, 1), (2, 2), (3, 3), (4, 4), (7, 7), (9, 9), (3, 11), (11, 3))
PPEG_C, PPEG_B = (4, 64, 257, 320), (1, 3)
PPEG_WGRAD_GRIDS = PPEG_GRIDS + ((2, 15), (2, 16), (2, 17), (2, 33))
PPEG_WGRAD_C, PPEG_WGRAD_B = (4, 70, 130), (1, 2, 3)


def ppeg_inputs(B, Hh, Ww, C, family):
    """-> x, dy [B, 1 + Hh*Ww, C], (w7, w5, w3) [C, k*k], (b7, b5, b3) [C], unit"""
    g = _gen(5, B, Hh, Ww, C)
    shape = (B, 1 + Hh * Ww, C)
    if family == "grid":
        return (_ints(g, shape, -8, 8), _ints(g, shape, -8, 8), [_ints(g, (C, k * k), -3, 3) for k in (7, 5, 3)], [_ints(g, (C,), -3, 3) for _ in range(3)], 1.0)
    return _randn(g, *shape), _randn(g, *shape), [_randn(g, C, k * k) * 0.1 for k in (7, 5, 3)], [_randn(g, C) * 0.1 for _ in range(3)], None


PINV_N = (4, 32, 252, 256, 260, 512, 1024, 35, 1028)
PINV_GROUPS = ((6, 6), (6, 2), (6, 1))          # (nmat, group)
PINV_BWD_N = (32, 256, 288, 1024, 40, 1056)
PINV_BWD_NMAT = 3


def pinv_inputs(n, family):
    """-> x [6, n, n], signed; the maximal row planted in matrix 1, the maximal column in matrix 4.  grid: |x| integers <= 3."""
    g = _gen(6, n)
    if family == "grid":
        x = _ints(g, (6, n, n), -2, 2)
        x[1, n // 3] += torch.where(x[1, n // 3] < 0, -1.0, 1.0)
        x[4, :, n // 2] += torch.where(x[4, :, n // 2] < 0, -1.0, 1.0)
        return x
    x = torch.softmax(_randn(g, 6, n, n), -1) * torch.where(_randn(g, 6, n, n) < 0, -1.0, 1.0)          # the model's magnitudes: rows of a softmax, signs added
    x[4, :, n // 2] *= 1.25 * x.abs().sum(-2).max() / x[4, :, n // 2].abs().sum()
    x[1, n // 3] *= 1.05 * x.abs().sum(-1).max() / x[1, n // 3].abs().sum()
    return x


def pinv_bwd_inputs(n, family):
    """-> x > 0 [3, n, n], dz, dx0; the arg-max row planted in matrix 2 (row n // 3), the arg-max column in matrix 0 (column n // 2), each unique by a relative margin
    >= 1e-3 (asserted from the reference by the tests).  Raw softmax rows will not do: their sums are all 1 up to rounding and the arg-max is then noise."""
    g = _gen(7, n)
    nm = PINV_BWD_NMAT
    if family == "grid":
        x = _ints(g, (nm, n, n), 1, 2)
        x[0, :, n // 2] += 1
        x[2, n // 3] += 1
        return x, _ints(g, (nm, n, n), -1, 3), _ints(g, (nm, n, n), -8, 8) / (16.0 * n * n)          # dz off centre: ds is no accident; dx0 at dz / s's magnitude
    x = torch.softmax(_randn(g, nm, n, n), -1)
    x[0, :, n // 2] *= 1.25 * x.sum(-2).max() / x[0, :, n // 2].sum()          # the column first: the row's 5 % then moves no column sum by more than 5 % of one entry
    x[2, n // 3] *= 1.05 * x.sum(-1).max() / x[2, n // 3].sum()
    return x, (_randn(g, nm, n, n) * 2 + 1) / n, _randn(g, nm, n, n) * (2.0 / n)


def pinv_bwd_tie_inputs(n=32):
    """Two bit-identical maximal rows (matrix 1 row 5, matrix 2 row 3) and two bit-identical maximal columns (matrix 0, columns 7 and 9): integers, so every sum
    is exact and the tie is one in fp32 as well.  The first flat index wins: row 1 * n + 5, column 7."""
    g = _gen(8, n)
    x = _ints(g, (3, n, n), 1, 2)
    x[1, 5] = 3.0
    x[2, 3] = 3.0
    x[0, :, 7] = 3.0
    x[0, :, 9] = 3.0
    return x, _ints(g, (3, n, n), 0, 2), _ints(g, (3, n, n), -8, 8) / (16.0 * n * n), 1 * n + 5, 7
