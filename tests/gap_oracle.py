"""fp64 reference, planted-score case builders, per-element bars and reference-side mutants for gated-attention pooling
(stamp_amd/csrc/gap_fused.hip, gap.hip).  Pinned on the CPU by test_cpu_gap_oracle.py, used on the GPU by test_gpu_gap_forms.py.  Everything runs on the
device of its inputs.

  h = relu(x Wfc^T + bfc);  A_n = c . (tanh(Wa h_n + ba) * sigmoid(Wb h_n + bb)) + cb;  out_b = softmax_{n in bag b}(A) @ x

Family I ("grid"): integer operands, every intermediate an integer below 2^24, every transcendental evaluated only where its fp32 value is exact:
  * column k = 16 t + 4 q + e of x holds (q + 1)(e + 1) r[n, t], r a non-periodic pattern in {-3 .. 3} \\ {0}; column KF = 6 holds the row's flag s_n in {0, 1}.
  * hidden unit l reads two columns of one 16-column tile with weights (w1, w2), w1 m1 + w2 m2 = 0 for the columns' multipliers m -- the payload cancels, and any
    XOR swizzle q -> q ^ s of the 16-byte chunks, or any other pairing of k, leaves w1 m1' + w2 m2' != 0 (PROBES, asserted by test_cpu_gap_oracle.py).  Units with
    l % 7 == 3 also read the flag: h_l = s_n; the others carry a bias (5 l + l // 16) % 4: h_l = that constant.
  * gate channel d reads one flag unit (weight 64 / 160) and two constant units whose contribution is folded into the bias, so tanh sees only -32 / +32 (fp32: -1 /
    +1) and sigmoid only -128 / +32 (expf(128) = inf -> exactly 0; 1 + expf(-32) rounds to 1 -> exactly 1).  Channel kinds by d % 4: P (a = 2 s - 1, b = 1),
    G (a = 1, b = s), Z (a = 2 s - 1, b = 0), P.  c_d = 8 + 3 d % 8, so a flagged row scores 2 sum_P c + sum_G c >= 128 above an unflagged one: exp(A - m) is 1 or 0.
Family II ("real"): Gaussian operands as in test_gpu_seams.py; feature K0 -> hidden unit L0 -> gate channel D0 is a private path (every other weight on it is zero)
that carries a prescribed score: x[n, K0] = atanh(T'_n / G) with G = gamma sigmoid(beta), T' the target shifted to be non-negative.  The other channels keep
c = 0.002 N(0, 1): the realised score is the target plus ~0.01 nat of noise, and the reference evaluates whatever results.

Bars (u = 2^-24, gamma_n = n u / (1 - n u)), per element:
  family I   A_raw bit-equal to fp64; out bit-equal where the number of winning rows is a power of two, else within 2 u |out| (fused forms: the reciprocal and the
             product, gap_fused.hip:139-142, 202-203) -- the six-launch form normalises every row's weight before it sums (gap.hip:131-137, 146), so there the
             bar counts its own roundings: gamma_{min(k, 128) + chunks + 2} (reciprocal, one product and one addition per winning row of a 128-row chunk, the chunk sum).
  family II  dh <= gamma_{F+1} abs_h;  dpre <= gamma_{L+1} abs_pre + |W| dh;  da <= dpre_a + K_FN u |a|;  db <= dpre_b / 4 + (K_FN + 2) u b (the addition and the
             division of 1 / (1 + e) besides the exp; d b / b <= d e / e);  dA <= sum |c_d| (da_d b_d + |a_d| db_d) + gamma_{D+2} (sum |c a b| + |cb|);
             dout_c <= [2 max_n dA_n + (K_FN + 4) u + gamma_depth] sum_n p_n |x_nc|,  depth = ROWS + ceil(units / 4) + 6 (the association gap_fused.hip documents;
             the six-launch form: ROWS = 128, its chunks summed in sequence: depth = 128 + chunks + 6).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

U = 2.0 ** -24
# ulp allowance of tanhf / expf.  Smallest of {1, 2, 4, 8} at which the plain fp32 CPU evaluation (oracle/gated_attention.py) stays at or below 0.5 x bar on every
# element of every family-II case (test_cpu_gap_oracle.py::test_k_fn_is_the_smallest_that_fits asserts it).  Measured worst ratios at K_FN = 1: see K_FN_WORST.
K_FN = 1
K_FN_WORST = {"A_raw": 0.02, "out": 0.03}          # measured 0.0149 (f32d64 / ascending) and 0.0232 (f16d16 / diffuse), rounded up (profiles/gap_kernel_errors.txt has the figures per case)
KEYS = ("fc_w", "fc_b", "a_w", "a_b", "b_w", "b_b", "c_w", "c_b")
KF = 6                                             # the flag column of family I
K0, L0, D0 = 5, 9, 3                               # the planted path of family II
BETA = 2.0
# (column, weight) pairs inside a 16-column tile; multiplier of column 4 q + e is (q + 1)(e + 1); w1 m1 + w2 m2 = 0
PROBES = (((1, 3), (8, -2)), ((2, 8), (7, -3)), ((4, 4), (13, -1)), ((5, 3), (14, -1)), ((0, 9), (10, -1)), ((3, 3), (14, -1)))
GRID_FAMILIES = ("uniform", "winner", "two_winners", "winner_per_unit")
REAL_FAMILIES = ("diffuse", "gaussian", "ascending", "descending", "plateau")
MUTANTS = ("drop_last_row", "pad_last_unit", "skip_unit1", "no_rescale", "prev_bag_max", "offsets_minus_256", "swap_k_pairs", "drop_last_gate_block",
           "drop_cols_1024")


def gamma(n):
    return n * U / (1.0 - n * U)


def col_mult(k):
    return ((k % 16) // 4 + 1) * (k % 4 + 1)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Ref:
    A: torch.Tensor            # [rows] fp64 attention_raw
    out: torch.Tensor          # [bags, F] fp64
    abs_A: torch.Tensor        # [rows] sum_d |c_d a_d b_d| + |cb|
    dA0: torch.Tensor          # [rows] the bar of A at K_FN = 0
    abs_cab: torch.Tensor      # [rows] sum_d |c_d a_d b_d|: the bar grows by 2 u abs_cab per unit of K_FN
    abs_out: torch.Tensor      # [bags, F] sum_n p_n |x_nc|
    num: torch.Tensor          # [bags, F] sum_n exp(A_n - m) x_nc
    den: torch.Tensor          # [bags]
    nwin: torch.Tensor         # [bags] rows at the bag's maximum
    seg: torch.Tensor          # [rows] bag of every row
    lengths: torch.Tensor      # [bags]


def _w64(w):
    return {k: w[k].double() for k in KEYS}


def row_stage(x, w):
    """fp64 h, gate and score of the rows of x, with every absolute sum the bars need -> dict (A, abs_h, abs_a, abs_b, abs_cab, abs_A, dA0)."""
    w = _w64(w)
    xd = x.double()
    L, Fdim = w["fc_w"].shape
    D = w["a_w"].shape[0]
    h = torch.relu(xd @ w["fc_w"].T + w["fc_b"])
    abs_h = xd.abs() @ w["fc_w"].abs().T + w["fc_b"].abs()
    pa, pb = h @ w["a_w"].T + w["a_b"], h @ w["b_w"].T + w["b_b"]
    abs_a, abs_b = h @ w["a_w"].abs().T + w["a_b"].abs(), h @ w["b_w"].abs().T + w["b_b"].abs()
    a, b = torch.tanh(pa), torch.sigmoid(pb)
    c = w["c_w"].reshape(-1)
    t = a * b * c
    A = t.sum(1) + w["c_b"].reshape(())
    abs_cab = t.abs().sum(1)
    abs_A = abs_cab + w["c_b"].abs().reshape(())
    dh = gamma(Fdim + 1) * abs_h
    dpa = gamma(L + 1) * abs_a + dh @ w["a_w"].abs().T
    dpb = gamma(L + 1) * abs_b + dh @ w["b_w"].abs().T
    dA0 = (c.abs() * (dpa * b + a.abs() * (dpb / 4 + 2 * U * b))).sum(1) + gamma(D + 2) * abs_A
    return {"A": A, "abs_h": abs_h, "abs_a": abs_a, "abs_b": abs_b, "abs_cab": abs_cab, "abs_A": abs_A, "dA0": dA0}


def _segments(lengths, device):
    lengths = torch.as_tensor(lengths, dtype=torch.int64, device=device)
    B = lengths.numel()
    off = torch.zeros(B + 1, dtype=torch.int64, device=device)
    off[1:] = lengths.cumsum(0)
    seg = torch.repeat_interleave(torch.arange(B, device=device), lengths)
    local = torch.arange(int(off[-1]), device=device) - off[seg]
    return lengths, off, seg, local


def _seg(data, lengths, reduce="sum"):
    """Per-bag sum / max of the rows of data (bags are runs of consecutive rows): one segmented reduction, no atomics -- a 262 203-row bag does not serialise."""
    return torch.segment_reduce(data, reduce, lengths=lengths, axis=0)


def reference(x, lengths, w, mutant=None, chunk=32768):
    """fp64 gated-attention pooling of the bags of x ([rows, F], bag b = the next lengths[b] rows), vectorised over bags -> Ref (A_raw = .A, out = .out).
    `mutant` plants one fault of MUTANTS into THIS evaluation (never into a kernel)."""
    assert mutant is None or mutant in MUTANTS
    dev = x.device
    lengths, off, seg, local = _segments(lengths, dev)
    B, rows, F = lengths.numel(), x.shape[0], x.shape[1]
    assert rows == int(off[-1]) and int(lengths.min()) > 0
    if mutant == "swap_k_pairs":                   # k and k + 1 of stage 2 exchanged inside every group of 16
        perm = torch.arange(w["a_w"].shape[1], device=dev) ^ 1
        w = dict(w, a_w=w["a_w"][:, perm], b_w=w["b_w"][:, perm])
    if mutant == "drop_last_gate_block":
        cw = w["c_w"].clone()
        cw[..., -16:] = 0
        w = dict(w, c_w=cw)
    parts = [row_stage(x[i:i + chunk], w) for i in range(0, rows, chunk)]
    A, abs_A, dA0, abs_cab = (torch.cat([p[k] for p in parts]) for k in ("A", "abs_A", "dA0", "abs_cab"))
    del parts
    m = _seg(A, lengths, "max")
    nwin = _seg((A == m[seg]).double(), lengths).long()
    if mutant == "prev_bag_max":                   # exp(A - M') cancels in exact arithmetic: the fault shows in fp32's range only
        mm = torch.cat([m[:1], m[:-1]])
        e = torch.exp((A - mm[seg]).float()).double()
    elif mutant == "no_rescale":                   # every 64-row unit normalised to its own maximum, partials added as they are
        uid = off[seg] // 64 + seg + local // 64
        mu = torch.full((int(uid.max()) + 1,), -math.inf, dtype=torch.float64, device=dev).scatter_reduce(0, uid, A, "amax")
        e = torch.exp(A - mu[uid])
    else:
        e = torch.exp(A - m[seg])
    last = off[1:] - 1
    if mutant == "drop_last_row":
        e = e.clone()
        e[last[lengths > 1]] = 0
    if mutant == "pad_last_unit":                  # the lanes behind the bag's end re-read the last row: here they keep its weight
        e = e.clone()
        e[last] *= (1 + (-lengths) % 64).double()
    if mutant == "skip_unit1":
        e = torch.where((local >= 64) & (local < 128), torch.zeros_like(e), e)
    den = _seg(e, lengths)
    xe = x.double() * e[:, None]
    num, abs_num = _seg(xe, lengths), _seg(xe.abs(), lengths)
    del xe
    out, abs_out = num / den[:, None], abs_num / den[:, None]
    if mutant == "offsets_minus_256" and B > 256:
        out = torch.cat([out[:256], out[:B - 256]])
    if mutant == "drop_cols_1024":
        out = out.clone()
        out[:, 1024:] = 0
    return Ref(A, out, abs_A, dA0, abs_cab, abs_out, num, den, nwin, seg, lengths)


def evaluate_fp32(x, lengths, w):
    """The formula in plain torch fp32 (what oracle/gated_attention.py does per bag), vectorised over bags -> (A_raw, out, num, den)."""
    import torch.nn.functional as Fn
    lengths, off, seg, local = _segments(lengths, x.device)
    B = lengths.numel()
    x = x.float()
    h = Fn.relu(Fn.linear(x, w["fc_w"], w["fc_b"]))
    a = torch.tanh(Fn.linear(h, w["a_w"], w["a_b"]))
    b = torch.sigmoid(Fn.linear(h, w["b_w"], w["b_b"]))
    A = Fn.linear(a * b, w["c_w"].reshape(1, -1), w["c_b"].reshape(1)).reshape(-1)
    m = torch.full((B,), -math.inf, device=x.device).scatter_reduce(0, seg, A, "amax")
    e = torch.exp(A - m[seg])
    den = torch.zeros(B, device=x.device).index_add(0, seg, e)
    num = torch.zeros(B, x.shape[1], device=x.device).index_add(0, seg, e[:, None] * x)
    return A, num / den[:, None], num, den


# ---- bars ---------------------------------------------------------------------------------------------------------------------------------------------------
def depth_fused(lengths, rows):
    """ROWS + ceil(units / 4) + 6 per bag: the unit's rows in sequence, a wave's quarter of the units in sequence, four quarter sums, the chunk sum, 1 / den, the product."""
    units = (lengths + rows - 1) // rows
    return rows + (units + 3) // 4 + 6


def depth_unfused(lengths):
    return 128 + (lengths + 127) // 128 + 6


def real_bars(ref: Ref, depth, k_fn=None):
    """-> (bar of A_raw [rows], bar of out [bags, F]) of family II; depth: per bag (depth_fused / depth_unfused)."""
    k = K_FN if k_fn is None else k_fn
    dA = ref.dA0 + k * 2 * U * ref.abs_cab
    B = ref.lengths.numel()
    dmax = _seg(dA, ref.lengths, "max")
    depth = torch.as_tensor(depth, dtype=torch.float64, device=dA.device)
    rel = 2 * dmax + (k + 4) * U + depth * U / (1 - depth * U)
    return dA, rel[:, None] * ref.abs_out


def grid_out_bar(ref: Ref, six_launch=False):
    """Family I: 0 where the bag's winner count is a power of two (bit-equal), else 2 u |out| (fused) / gamma_{min(k, 128) + chunks + 2} |out| (six-launch form)."""
    k = ref.nwin
    pow2 = (k & (k - 1)) == 0
    if six_launch:
        n = (torch.clamp(k, max=128) + (ref.lengths + 127) // 128 + 2).double()
        rel = torch.where(pow2, torch.zeros_like(n), n * U / (1 - n * U))
        return rel[:, None] * ref.abs_out
    rel = torch.where(pow2, 0.0, 2 * U).double()
    return rel[:, None] * ref.out.abs()


# ---- family I -----------------------------------------------------------------------------------------------------------------------------------------------
def grid_weights(F, L, D, device="cpu", uniform=False):
    assert F % 16 == 0 and D % 4 == 0 and L >= 64
    T = F // 16
    fc_w, fc_b = torch.zeros(L, F), torch.zeros(L)
    flag_units = [l for l in range(L) if l % 7 == 3]
    for l in range(L):
        t = (3 * l + l // 7) % T
        for kk, wt in PROBES[(l + l // 16) % len(PROBES)]:
            fc_w[l, 16 * t + kk] = wt
        if l % 7 == 3:
            fc_w[l, KF] += 1
        else:
            fc_b[l] = (5 * l + l // 16) % 4
    const = fc_b.clone()                            # h of an unflagged unit; a flag unit holds s_n

    def plain(l):                                   # the next unit that is no flag unit
        l %= L
        return l if l % 7 != 3 else (l + 1) % L

    a_w, b_w, a_b, b_b = torch.zeros(D, L), torch.zeros(D, L), torch.zeros(D), torch.zeros(D)
    for d in range(D):
        kind = "PGZP"[d % 4]
        lf = flag_units[(11 * d + 5) % len(flag_units)]
        la = ((plain(13 * d + 1), 3), (plain(29 * d + 6), -2))
        lb = ((plain(17 * d + 2), -1), (plain(7 * d + 9), 4))
        for l, wt in la:
            a_w[d, l] += wt
        for l, wt in lb:
            b_w[d, l] += wt
        ca = float(a_w[d] @ const)
        cb = float(b_w[d] @ const)
        if kind in "PZ":
            a_w[d, lf] = 64
            a_b[d] = -32 - ca
        else:
            a_b[d] = 32 - ca
        if kind == "P":
            b_b[d] = 32 - cb
        elif kind == "G":
            b_w[d, lf] = 160
            b_b[d] = -128 - cb
        else:
            b_b[d] = -128 - cb
    c_w = torch.tensor([0.0 if uniform else 8.0 + (3 * d) % 8 for d in range(D)]).reshape(1, D)
    w = {"fc_w": fc_w, "fc_b": fc_b, "a_w": a_w, "a_b": a_b, "b_w": b_w, "b_b": b_b, "c_w": c_w, "c_b": torch.tensor([5.0])}
    return {k: v.to(device).contiguous() for k, v in w.items()}


def grid_x(lengths, F, flags):
    """x of family I: payload (q + 1)(e + 1) r[n, t], the flag in column KF.  flags: [rows] 0 / 1 on the device the case lives on."""
    dev = flags.device
    rows, T = flags.numel(), F // 16
    n = torch.arange(rows, device=dev)[:, None]
    t = torch.arange(T, device=dev)[None, :]
    r6 = (7 * n + n // 5 + 3 * t + (n * t) // 3) % 6
    r = torch.where(r6 < 3, r6 - 3, r6 - 2).float()                       # {-3, -2, -1, 1, 2, 3}
    mult = torch.tensor([float(col_mult(k)) for k in range(16)], device=dev)
    x = (r[:, :, None] * mult[None, None, :]).reshape(rows, F).contiguous()
    x[:, KF] = flags.float()
    return x


def winner_candidates(N):
    """Rows a single winner is planted at: 0, the last row, both sides of every unit boundary for ROWS = 16 and 64, the last valid row of a partial unit (= N - 1)."""
    c = {0, N - 1}
    for b in range(16, N, 16):
        c.update((b - 1, b))
    return sorted(c)


def grid_flags(lengths, family, device="cpu", variant=0):
    lengths = [int(v) for v in lengths]
    flags = torch.zeros(sum(lengths))
    o = 0
    for bi, N in enumerate(lengths):
        if family == "winner":
            if bi % 5 != 4 or len(lengths) < 5:                            # every fifth bag of a batch keeps no winner: all its rows tie at the low score
                cand = winner_candidates(N)
                flags[o + cand[(bi + variant) % len(cand)]] = 1
        elif family == "two_winners":
            flags[o] = 1
            flags[o + N - 1] = 1
        elif family == "winner_per_unit":
            for u0 in range(0, N, 16):
                nv = min(16, N - u0)
                flags[o + u0 + (5 * (u0 // 16) + 3) % nv] = 1
        else:
            assert family == "uniform"
        o += N
    return flags.to(device)


def grid_case(F, L, D, lengths, family, device="cpu", variant=0):
    w = grid_weights(F, L, D, device, uniform=family == "uniform")
    flags = grid_flags(lengths, family, device, variant)
    return grid_x(lengths, F, flags), w


def sweep_lengths():
    """Bags whose single winners (grid_flags 'winner', bag b -> candidate b) together visit every candidate row of a 75-row and a 139-row bag."""
    return [75] * len(winner_candidates(75)) + [139] * len(winner_candidates(139))


def sweep_flags(device="cpu"):
    lens = sweep_lengths()
    flags = torch.zeros(sum(lens))
    o, i75, i139 = 0, 0, 0
    for N in lens:
        cand = winner_candidates(N)
        if N == 75:
            flags[o + cand[i75]] = 1
            i75 += 1
        else:
            flags[o + cand[i139]] = 1
            i139 += 1
        o += N
    return flags.to(device)


# ---- family II ----------------------------------------------------------------------------------------------------------------------------------------------
def gaussian_weights(F, L, D, g):
    return {"fc_w": torch.randn(L, F, generator=g) / F ** 0.5, "fc_b": torch.randn(L, generator=g) * 0.1,
            "a_w": torch.randn(D, L, generator=g) / L ** 0.5, "a_b": torch.randn(D, generator=g) * 0.1,
            "b_w": torch.randn(D, L, generator=g) / L ** 0.5, "b_b": torch.randn(D, generator=g) * 0.1,
            "c_w": torch.randn(1, D, generator=g) * 2, "c_b": torch.randn(1, generator=g)}


def real_targets(lengths, family, g, rows=64):
    """Per-row target scores (<= 0, the bag's maximum at 0) of one planted family, fp64 on the CPU."""
    out = []
    for N in (int(v) for v in lengths):
        n = torch.arange(N)
        u, units = n // rows, (N + rows - 1) // rows
        noise = torch.randn(N, generator=g, dtype=torch.float64).abs()
        if family == "diffuse":
            T = -0.05 * torch.rand(N, generator=g, dtype=torch.float64)
        elif family in ("ascending", "descending"):
            step = (units - 1 - u) if family == "ascending" else u
            T = -3.0 * step.double() - noise
            first = n % rows == 0
            T[first] = -3.0 * step[first].double()                         # the first row of every unit sits exactly at the unit's maximum
        else:
            assert family == "plateau"
            T = -6.0 - noise
            T[min(3, N - 1)] = 0.0
            T[max(N - 3, 0)] = 0.0
        out.append(T - T.max())
    return torch.cat(out)


def real_case(F, L, D, lengths, family, seed, device="cpu", rows=64):
    g = torch.Generator().manual_seed(seed)
    w = gaussian_weights(F, L, D, g)
    total = int(sum(int(v) for v in lengths))
    x = torch.randn(total, F, generator=g)
    if family != "gaussian":
        T = real_targets(lengths, family, g, rows)
        span = float(-T.min())
        G = 2 * span + 2
        sig = 1 / (1 + math.exp(-BETA))
        w["fc_w"][:, K0] = 0
        w["fc_w"][L0, :] = 0
        w["fc_w"][L0, K0] = 1
        w["fc_b"][L0] = 0
        for k in ("a_w", "b_w"):
            w[k][:, L0] = 0
            w[k][D0, :] = 0
        w["a_w"][D0, L0] = 1
        w["a_b"][D0] = 0
        w["b_b"][D0] = BETA
        w["c_w"] = torch.randn(1, D, generator=g) * 0.002
        w["c_w"][0, D0] = G / sig
        x[:, K0] = torch.atanh((T + span) / G).float()                    # gamma tanh(alpha t) sigmoid(beta) = T + span, alpha = 1
    return x.to(device).contiguous(), {k: v.to(device).contiguous() for k, v in w.items()}


# ---- the geometries both test modules run ----------------------------------------------------------------------------------------------------------------------
def ragged_300():
    lens = [1 + (53 * i + (i // 7) * 11) % 90 if i % 3 else 1 + (29 * i) % 40 for i in range(300)]
    lens[0], lens[299], lens[150] = 90, 1, 90
    assert sum(lens) <= 12288 and sum(lens) > 8192 and max(lens) == 90 and min(lens) == 1
    return lens


UNIT_LENGTHS = [1, 15, 16, 17, 63, 64, 65,                               # rows per bag
                2 * 64 - 5, 3 * 64 - 5, 4 * 64 - 5, 5 * 64 - 5, 17 * 64 - 5, 69 * 64 - 5,      # 2 .. 69 units of 64 rows
                2 * 16 - 5, 3 * 16 - 5, 4 * 16 - 5, 5 * 16 - 5, 17 * 16 - 5, 69 * 16 - 5]      # 2 .. 69 units of 16 rows
SMALL_LENGTHS = [1, 17, 65, 2 * 64 - 5, 3 * 64 - 5, 5 * 64 - 5, 3 * 16 - 5]
BIG_BAG = 4097 * 64 - 5

# name -> (F, L, D, lengths, forms that take it, families).  forms: "pool" (amds_gated_attn_pool per bag), "slab" / "split" / "auto" (the batched entry),
# "unfused" (the six-launch form per bag), "nopack" (batched, auto, packed == NULL).
ALL_FAMILIES = GRID_FAMILIES + REAL_FAMILIES
GEOMS = {
    "chief512": (768, 512, 256, UNIT_LENGTHS, ("pool", "slab", "split", "auto", "unfused", "nopack"), ALL_FAMILIES),
    "l256": (384, 256, 256, SMALL_LENGTHS + [69 * 16 - 5], ("pool", "slab", "split", "auto", "nopack"), ALL_FAMILIES),
    "sweep": (32, 256, 64, sweep_lengths(), ("slab", "split", "pool"), ("winner",)),
    "f32d64": (32, 256, 64, SMALL_LENGTHS, ("slab", "split", "auto", "unfused", "nopack"), ALL_FAMILIES),
    "f16d16": (16, 256, 16, SMALL_LENGTHS + [17 * 64 - 5], ("pool", "slab", "auto", "unfused", "nopack"), ALL_FAMILIES),
    "f48d48": (48, 512, 48, SMALL_LENGTHS, ("pool", "slab", "auto", "nopack"), ALL_FAMILIES),
    "f1040": (1040, 256, 64, SMALL_LENGTHS, ("pool", "slab", "auto", "unfused"), ALL_FAMILIES),
    "f4096": (4096, 512, 64, [5, 3, 70], ("pool", "slab", "split", "auto"), ("uniform", "winner", "two_winners", "gaussian", "diffuse")),
    "l320": (208, 320, 72, [333, 1, 129], ("unfused", "pool"), ALL_FAMILIES),
    "bags255": (32, 256, 64, [1 + (3 * i) % 5 for i in range(255)], ("slab", "split", "auto"), ("winner", "gaussian")),
    "bags256": (32, 256, 64, [1 + (3 * i) % 5 for i in range(256)], ("slab", "split", "auto"), ("winner", "gaussian")),
    "bags257": (32, 256, 64, [1 + (3 * i) % 5 for i in range(257)], ("slab", "split", "auto"), ("winner", "gaussian")),
    "ragged300": (32, 256, 64, ragged_300(), ("slab", "split", "auto", "nopack"), ("uniform", "winner", "two_winners", "winner_per_unit", "diffuse", "gaussian", "descending")),
    "bags65537": (32, 256, 16, [1] * 65537, ("slab",), ("winner", "gaussian")),
    "chunk2": (16, 256, 16, [BIG_BAG], ("pool", "slab"), ("uniform", "two_winners", "winner_per_unit", "diffuse", "plateau")),
}


def build_case(geom, family, device="cpu"):
    """-> (x, lengths, w) of one geometry and family."""
    F, L, D, lengths, _, fams = GEOMS[geom]
    assert family in fams
    if family in GRID_FAMILIES:
        if geom == "sweep":
            return grid_x(lengths, F, sweep_flags(device)), lengths, grid_weights(F, L, D, device)
        if geom == "bags65537":                    # one-row bags: every third row flagged, so A_raw tells a bag from its neighbours
            flags = (torch.arange(len(lengths), device=device) % 3 == 1).float()
            return grid_x(lengths, F, flags), lengths, grid_weights(F, L, D, device)
        x, w = grid_case(F, L, D, lengths, family, device)
        return x, lengths, w
    assert L > L0 and D > D0 and F > K0
    x, w = real_case(F, L, D, lengths, family, seed=1000 + F + L + D + len(lengths), device=device)
    return x, lengths, w
