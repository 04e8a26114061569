"""Inputs, fp64 references, a rounding model, per-tensor error metrics and reference-side mutants for the attention family
(test_cpu_attention_bars.py, test_gpu_attention_sharp.py).  Needs no GPU; every function runs on the device of its inputs.

Why: the family's parity tests feed i.i.d. Gaussian operands (a diffuse softmax: no key, mask bit, tile or rescale step carries weight) and judge all
tensors by one `k eps max(1, |ref|max)` bar, which the gradients sit far below.  Here

* the builders plant structure: `planted` (query i -> key (a i + T - 1) mod T, 12 nats), `ascending` / `descending` (one boosted key per 64-key tile,
  4 nats apart: the running maximum moves at every tile / never again), `saturated` (40 nats), `uniform` (P = 1 / T), next to the `gaussian` baseline;
* `reference` is fp64 autograd of the plain statement of each form, `flash` the same computation written out the way the kernels do it (un-normalised
  weights, saved log2-sum-exp, dS = P o (dP - D)) -- with no rounding it equals `reference` to fp64 rounding (asserted on the CPU), with `dt` given it
  applies the kernels' documented 16-bit rounding sites (the ROUNDING MODEL), with `fault` given it is one of MUTANTS;
* `errors` is per tensor: relative L2 and max-abs over the tensor's own |ref|max, no `max(1, ...)` floor; lse absolute in log2 units;
* `bars` = factor x (the rounding model's own error + the first-order fp32 accumulation error of that tensor), 4 forward, 8 backward.

The fp32 term: every kernel of the family accumulates scores, P V, dP, D and the gradient products in fp32 (MFMA accumulators, attention_flash.hip:242-246,
attention_train.hip:43, :210-211).  Where the reference is exactly representable or cancels to nothing (T = 1: dq = dk = 0; `saturated`: dS ~ 1e-15) the
16-bit model has NO error and a bar of k x 0 would judge fp32 noise against zero.  `flash` therefore also returns, per tensor, the standard probabilistic bound
sqrt(n) 2^-24 sum|terms| of its fp32 dot products (n terms each) and the effect of the score's fp32 error on P; on a tensor that 16-bit rounding touches it is a
few percent of the model's error at the most (the measured error / bar of such tensors is 1/4 forward and 1/8 backward: the kernels sit on the model).
"""
from __future__ import annotations

import math

import torch

TILE = 64            # keys per streamed tile (attention_flash.hip:17 FA_KT, attention_train.hip:20 BT_TILE)
QBLOCK = 128         # queries per workgroup: 4 waves x 32 (attention_flash.hip:7)
LOG2E = 1.4426950408889634
U32 = 2.0 ** -24     # unit round-off of fp32
FWD_FACTOR, BWD_FACTOR = 4.0, 8.0          # the project's factors between one rounding and its forward / backward bars (test_gpu_abi_attention.py)
BUILDERS = ("gaussian", "planted", "ascending", "descending", "saturated", "uniform")
FWD_TENSORS = ("out", "lse", "u", "osm")
STREAM_T = (1, 64, 65, 193, 321)           # one key; one full tile; a tile + 1; 4 tiles with one key in the last and a second query block of 65 rows; 6 tiles, 3 blocks
STREAM_BH = (2, 3)
TRAIN_SHAPE = (1, 1025, 2)                 # the training length, `planted` only


def stream_cases():
    """(builder, B, T, H) of every streaming form: all builders at STREAM_T, plus one planted case at the training length."""
    return [(n, STREAM_BH[0], T, STREAM_BH[1]) for n in BUILDERS for T in STREAM_T] + [("planted",) + TRAIN_SHAPE]


def eps(dt) -> float:
    return 2.0 ** -10 if dt == torch.float16 else 2.0 ** -7


def plant_map(T: int, a: int | None = None) -> torch.Tensor:
    """pi(i) = (a i + T - 1) mod T, a coprime to T: a permutation with pi(0) = T - 1."""
    if a is None:
        a = 67 if T > 67 else max(T // 2 + 1, 1)
        while math.gcd(a, T) != 1:
            a += 1
    assert math.gcd(a, T) == 1
    return (a * torch.arange(T) + T - 1) % T


# ---- builders: (q [B, H, Tq, hd], k, v [B, H, T, hd]) fp32, before the 16-bit rounding -----------------------------------------------------------
def _unit8(x):
    return x * (8.0 / x.norm(dim=-1, keepdim=True).clamp_min(1e-30))


def build(name: str, B: int, T: int, H: int, seed: int, Tq: int | None = None, hd: int = 64, a: int | None = None):
    Tq = T if Tq is None else Tq
    g = torch.Generator().manual_seed(seed * 7919 + 31 * T + H)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    v = rn(B, H, T, hd)
    if name == "gaussian":
        return rn(B, H, Tq, hd), rn(B, H, T, hd), v
    if name == "planted":                                  # 1.5 * |k|^2 / 8 = 12 nats on key pi(i)
        k = _unit8(rn(B, H, T, hd))
        return 0.5 * rn(B, H, Tq, hd) + 1.5 * k[:, :, plant_map(T, a)[:Tq]], k, v
    if name == "saturated":                                # sign keys (|k| = 8 exactly), q = 5 k_pi(i): 40 nats, |q| <= 6 per element
        k = torch.where(torch.rand(B, H, T, hd, generator=g) < 0.5, -1.0, 1.0)
        q = (5.0 * k[:, :, plant_map(T, a)[:Tq]] + 0.25 * rn(B, H, Tq, hd)).clamp(-6.0, 6.0)
        return q, k, v
    if name == "uniform":                                  # one key row per (bag, head): P = 1 / T exactly
        return 0.5 * rn(B, H, Tq, hd), (0.25 * rn(B, H, 1, hd)).expand(B, H, T, hd).contiguous(), v
    if name in ("ascending", "descending"):
        # tile t's boosted key is 8 e_t (one-hot: the boosted keys are exactly orthogonal), the others have no component on the first ntile axes;
        # q carries c_t on axis t: logit c_t + N(0, 0.5) on the boosted key, N(0, 0.5) elsewhere.  c_t = 8 + 4 t nats (ascending), reversed (descending).
        nt = (T + TILE - 1) // TILE
        assert nt <= hd
        k = rn(B, H, T, hd)
        k[..., :nt] = 0.0
        k = _unit8(k) if hd > nt else k
        for t in range(nt):
            j = min(t * TILE + (7 * t + 3) % TILE, T - 1)
            k[:, :, j] = 0.0
            k[:, :, j, t] = 8.0
        c = 8.0 + 4.0 * torch.arange(nt, dtype=torch.float32)
        q = 0.5 * rn(B, H, Tq, hd)
        q[..., :nt] = q[..., :nt] + (c if name == "ascending" else c.flip(0))
        return q, k, v
    raise KeyError(name)


def pack_qkv(q, k, v, dt):
    """[B, H, T, 64] x 3 -> the packed [B*T][3*H*hd] tensor (q | k | v thirds, each [H][hd]) in `dt`."""
    B, H, T, hd = k.shape
    return torch.stack((q, k, v), 0).permute(1, 3, 0, 2, 4).reshape(B * T, 3 * H * hd).to(dt)


def unpack_qkv(qkv, B, T, H, hd=64):
    q, k, v = qkv.double().reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    return q, k, v


def tokens(x):
    """[B, H, T, hd] -> [B*T][H*hd]."""
    B, H, T, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * hd)


def heads(x, B, T, H, hd=64):
    return x.double().reshape(B, T, H, hd).permute(0, 2, 1, 3)


def make_qkv(name, B, T, H, dt, seed=0, hd=64):
    return pack_qkv(*build(name, B, T, H, seed, hd=hd), dt)


def make_dout(B, T, H, dt, seed=0, hd=64, scale=1.0):
    g = torch.Generator().manual_seed(seed * 104729 + T + 3 * H + 1)
    return (torch.randn(B * T, H * hd, generator=g) * scale).to(dt)


def make_coords(B, T, seed=0):
    """Tile coordinates in [0, 4000) with the class token at (0, 0) (vision_tranformer.py:349-351), head scales as the existing ALiBi tests draw them."""
    g = torch.Generator().manual_seed(seed * 15485863 + T)
    c = torch.rand(B, T, 2, generator=g) * 4000.0
    c[:, 0] = 0.0
    return c


def make_alibi_scales(H, seed=0):
    g = torch.Generator().manual_seed(seed + 97 * H)
    return torch.rand(H, generator=g) * 0.5 + 0.1, torch.rand(H, generator=g) * 500.0 + 1800.0          # bias_scale, running_mean


def make_pad(B, T, seed=0):
    g = torch.Generator().manual_seed(seed + 5 * T + B)
    pad = (torch.rand(B, T, generator=g) > 0.5).to(torch.uint8)
    pad[:, 0] = 0
    return pad


def literal_mask(pad, B, T, H, mask_heads=None):
    """blocked [B, H, T, T] of attention_flash.hip's header (:28-34): (pad[q] & pad[k]) | (q > 0 & k == 0); mask_heads given: the pad row of bag
    (b * mask_heads + h) % B (the nn.MultiheadAttention branch), else that of bag b (the ALiBi branch)."""
    pb = pad.bool()
    if mask_heads is not None:
        idx = (torch.arange(B, device=pad.device)[:, None] * mask_heads + torch.arange(H, device=pad.device)[None, :]) % B
        pr = pb[idx]
    else:
        pr = pb[:, None].expand(B, H, T)
    blocked = (pr[..., :, None] & pr[..., None, :]).clone()
    blocked[..., 1:, 0] = True
    return blocked


# ---- fp64 references: the plain statement of each form, differentiated by autograd ----------------------------------------------------------------------
def reference(q, k, v, dout=None, *, scale=None, mult=None, pre_bias=None, blocked=None, post=None, zero=None, bias_scale=None):
    """q [B, H, Q, hd], k, v [B, H, K, hd] (any float type, taken to fp64).  out = W v with
         P = softmax(q k^T scale + pre_bias, blocked -> -inf)                 pre_bias: TICON's -slope_h |c_q - c_k| (ticon.py:183-215)
         W = (P o mult - bias_scale_h post) with `zero` products set to 0      mult: dropout keep mask x keep scale; post [B, H, Q, K]: cdist / running_mean
                                                                              (vision_tranformer.py:42-74), bias_scale [H]
    -> dict(out [B, H, Q, hd], lse [B, H, Q] log2 domain (of the undropped softmax), and with dout [B, H, Q, hd]: dq, dk, dv, dbs [H])."""
    q, k, v = (t.double().detach().clone().requires_grad_(dout is not None) for t in (q, k, v))
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    s = q @ k.transpose(-1, -2) * scale
    if pre_bias is not None:
        s = s + pre_bias.double()
    if blocked is not None:
        s = s.masked_fill(blocked, float("-inf"))
    w = torch.softmax(s, -1)
    if mult is not None:
        w = w * mult.double()
    bs = None
    if post is not None:
        bs = bias_scale.double().detach().clone().requires_grad_(dout is not None)
        w = w - post.double() * bs.view(1, -1, 1, 1)
    if zero is not None:
        w = w.masked_fill(zero, 0.0)
    out = w @ v
    r = {"out": out.detach(), "lse": torch.logsumexp(s.detach(), -1) * LOG2E}
    if post is not None:
        wz = post.double() if zero is None else post.double().masked_fill(zero, 0.0)
        r["u"] = wz @ v.detach()
        r["osm"] = r["out"] + r["u"] * bs.detach().view(1, -1, 1, 1)
    if dout is not None:
        out.backward(dout.double())
        r.update(dq=q.grad, dk=k.grad, dv=v.grad)
        if bs is not None:
            r["dbs"] = bs.grad
    return r


# ---- the kernels' way of computing the same thing: rounding model and mutants ---------------------------------------------------------------------------
def flash(q, k, v, dout=None, *, scale=None, mult=None, pre_bias=None, blocked=None, post=None, zero=None, bias_scale=None, post_scale=None,
          dt=None, round_p=True, out_dt="dt", grad_dt="dt", dq_dt="grad", fault=None):
    """The computation of `reference`, written as the kernels do it.  dt None: exact (fp64), must equal `reference`.  dt a 16-bit type: the ROUNDING MODEL,
    every site a line of the kernels:
      R1  the un-normalised weights exp2(s - m) (dropped and scaled: M o P) are rounded to dt before the P V product, the normaliser l sums the unrounded
          ones                                                                                         attention_flash.hip:242-246, :254-264, :277
      R2  ALiBi: the distance operand dist * post_scale_h is rounded to dt before its own V product     attention_flash.hip:286-290
      R3  out (and U, Osm) are rounded once, at the store                                               attention_flash.hip:320-331
      R4  the backward takes D = rowsum(dO o Osm) from the ROUNDED Osm, in fp32                         attention_train.hip:40-43
      R5  the backward rounds its V-side weight (M o P - dist_scale_h dist) and dS = P o (dP - D) to dt before their MFMA products
                                                                                                       attention_train.hip:247-253, :419-422
      R6  dq, dk, dv are rounded once, at the store                                                    attention_train.hip:294, :452
    round_p False: the one-query and cross-attention kernels, fp32 throughout (attention_flash.hip:405-431, :484-516; barspoon_train.hip:58, :158): R3 / R4 / R6
    only.  out_dt / grad_dt (dk, dv) / dq_dt: "dt", a torch dtype, or None for an fp32 tensor (cross-attention's out and dq; the ALiBi forms' bf16 out).
    post: the raw distances [B, 1 | H, Q, K]; post_scale [H]: the factor inside the rounded operand (1 / running_mean in training, bias_scale / running_mean
    at inference, where bias_scale is then None = 1).
    fault: a mutant of MUTANTS, (name, *args), applied to the exact computation.
    -> the tensors of `reference`, plus "floor": per tensor the first-order fp32 accumulation error (see the module docstring)."""
    dev = q.device
    q, k, v = q.double(), k.double(), v.double()
    B, H, Q, hd = q.shape
    K = k.shape[2]
    scale = hd ** -0.5 if scale is None else scale
    fname, fargs = (fault[0], fault[1:]) if fault else (None, ())
    r16 = (lambda x: x.to(dt).double()) if dt is not None else (lambda x: x)                    # noqa: E731
    r32 = (lambda x: x.float().double()) if dt is not None else (lambda x: x)                   # noqa: E731
    rp = r16 if round_p else (lambda x: x)                                                      # noqa: E731
    odt = dt if out_dt == "dt" else out_dt
    gdt = dt if grad_dt == "dt" else grad_dt
    ro = (lambda x: x.to(odt).double()) if (dt is not None and odt is not None) else r32          # noqa: E731
    rg = (lambda x: x.to(gdt).double()) if (dt is not None and gdt is not None) else r32          # noqa: E731
    qdt = gdt if dq_dt == "grad" else dq_dt
    rq = (lambda x: x.to(qdt).double()) if (dt is not None and qdt is not None) else r32          # noqa: E731
    mult = None if mult is None else mult.double()
    if mult is not None and fname == "swap_pair_bits":           # the two keep bits of each key pair of tile t change places
        t, = fargs
        lo, hi = t * TILE, min((t + 1) * TILE, K) // 2 * 2
        mult = mult.clone()
        if hi > lo:
            mult[..., lo:hi] = mult[..., lo:hi].reshape(*mult.shape[:-1], -1, 2).flip(-1).reshape(*mult.shape[:-1], hi - lo)
    if fname == "mask_next_head":
        mult = None if mult is None else mult.roll(-1, 1)
        blocked = None if blocked is None else blocked.roll(-1, 1)
        zero = None if zero is None else zero.roll(-1, 1)
    if fname == "mask_next_row":
        mult = None if mult is None else mult.roll(-1, 2)
        blocked = None if blocked is None else blocked.roll(-1, 2)
        zero = None if zero is None else zero.roll(-1, 2)
    if mult is not None and fname == "drop_keep_scale":
        mult = (mult > 0).double()

    s2 = q @ k.transpose(-1, -2) * (scale * LOG2E)               # log2 domain, as the kernels hold it
    if pre_bias is not None:
        s2 = s2 + pre_bias.double() * LOG2E
    s2 = r32(s2)
    dead = torch.zeros(B, H, Q, K, dtype=torch.bool, device=dev) if blocked is None else blocked.clone()
    if fname == "drop_last_key" and K > 1:
        dead[..., K - 1] = True
    if fname == "skip_tile":
        t, b = fargs
        dead[:, :, b * QBLOCK:(b + 1) * QBLOCK, t * TILE:(t + 1) * TILE] = True
    s2 = s2.masked_fill(dead, float("-inf"))
    m = s2.max(-1, keepdim=True).values
    e = torch.exp2(s2 - m)
    l = e.sum(-1, keepdim=True)
    o_w = torch.ones_like(e)                                      # extra factor on a key's weight in O (a missed rescale)
    if fname == "pad_in_l":                                       # the zero rows behind the last key of a partial tile counted with score 0
        l = l + ((-K) % TILE) * torch.exp2(-m)
    if fname in ("no_rescale_o", "no_rescale_l"):                 # the rescale by exp2(m_old - m_new) left out when tile t arrives
        t, = fargs
        if 0 < t < (K + TILE - 1) // TILE:
            m_before = s2[..., :t * TILE].max(-1, keepdim=True).values
            m_with = s2[..., :(t + 1) * TILE].max(-1, keepdim=True).values
            miss = torch.exp2(m_with - m_before)                  # >= 1: what the earlier tiles' sums keep too much of
            early = (torch.arange(K, device=dev) < t * TILE).view(1, 1, 1, K)
            if fname == "no_rescale_o":
                o_w = torch.where(early, miss, o_w)
            else:
                l = l + (e * early).sum(-1, keepdim=True) * (miss - 1.0)
    lse = r32(m + torch.log2(l)).squeeze(-1)
    w = e if mult is None else e * mult                          # un-normalised V-side weights
    if zero is not None:
        w = w.masked_fill(zero, 0.0)
    osm_acc = (rp(w) * o_w) @ v / l                               # R1
    res = {"lse": lse}
    bsv = None
    if post is not None:
        ps = torch.ones(H, device=dev, dtype=torch.float64) if post_scale is None else post_scale.double()
        dist_op = post.double() * ps.view(1, H, 1, 1)
        if zero is not None:
            dist_op = dist_op.masked_fill(zero, 0.0)
        u_acc = rp(dist_op) @ v                                   # R2 (fp32 distances in the one-query kernels, attention_flash.hip:560)
        bsv = torch.ones(H, device=dev, dtype=torch.float64) if bias_scale is None else bias_scale.double()
        out = ro(osm_acc - bsv.view(1, H, 1, 1) * u_acc)          # R3
        res.update(out=out, u=ro(u_acc), osm=ro(osm_acc))
    else:
        out = ro(osm_acc)                                         # R3
        res["out"] = out

    # fp32 accumulation floors (first order; module docstring)
    absq_k = (q.abs() @ k.abs().transpose(-1, -2)) * (scale * LOG2E)
    ds2 = math.sqrt(hd) * U32 * absq_k                            # the score's own fp32 error, log2 units
    rel_p = ds2 * math.log(2.0) + 2 * U32                         # ... as a relative error of a weight, + exp2 and the normaliser
    rel_p = rel_p.masked_fill(dead, 0.0)
    p_n = e / l
    w_abs = p_n if mult is None else p_n * mult
    if zero is not None:
        w_abs = w_abs.masked_fill(zero, 0.0)
    floor = {"lse": (p_n * ds2.masked_fill(dead, 0.0)).sum(-1) + 2 * U32 * (lse.abs() + 1.0),
             "out": (w_abs * rel_p) @ v.abs() + math.sqrt(K) * U32 * (w_abs @ v.abs())}
    if post is not None:
        floor["u"] = math.sqrt(K) * U32 * (dist_op.abs() @ v.abs())
        floor["osm"] = floor["out"]
        floor["out"] = floor["out"] + bsv.view(1, H, 1, 1) * floor["u"]
    res["floor"] = floor
    if dout is None:
        return res

    g = dout.double()
    osm_saved = res["osm"] if post is not None else out
    d_row = r32((g * osm_saved).sum(-1, keepdim=True))            # R4
    p = torch.exp2(s2 - lse.unsqueeze(-1))                        # the backward's P, from the saved log2-sum-exp (attention_train.hip:239)
    dp = r32(g @ v.transpose(-1, -2))
    dpr = dp if mult is None else dp * mult
    pw = p if mult is None else p * mult
    if fname == "omit_pd":
        ds = p * dpr
    else:
        ds = p * (dpr - d_row)
    if post is not None:
        chd = (bsv * ps).view(1, H, 1, 1) * post.double()
        pw = pw - (chd if zero is None else chd.masked_fill(zero, 0.0))
    if zero is not None:
        pw = pw.masked_fill(zero, 0.0)
        ds = ds.masked_fill(zero, 0.0)
    pw_r, ds_r = rp(pw), rp(ds)                                   # R5
    dv = pw_r.transpose(-1, -2) @ g
    dk = ds_r.transpose(-1, -2) @ q * scale
    dq = ds_r @ k * scale
    if fname == "scale_grad":
        which, f = fargs
        dq, dk, dv = (t * f if n == which else t for n, t in (("dq", dq), ("dk", dk), ("dv", dv)))
    if fname == "zero_last_key_grad":
        which, = fargs
        dk, dv = dk.clone(), dv.clone()
        (dk if which == "dk" else dv)[:, :, K - 1] = 0.0
    res.update(dq=rq(dq), dk=rg(dk), dv=rg(dv))                  # R6
    if post is not None:
        res["dbs"] = -(g * res["u"]).sum((0, 2, 3))               # attention_train.hip:44-47, from the rounded U
    a = ds.abs()                                                  # d(dS) = dP_weight (dP - D) + P (d(dP) + d(D)): the first term scales with dS itself
    ds_floor = a * rel_p + p * math.sqrt(hd) * U32 * ((g.abs() @ v.abs().transpose(-1, -2)) * (1.0 if mult is None else mult)
                                                         + (g * osm_saved).abs().sum(-1, keepdim=True))
    pw_abs = pw.abs()
    floor["dq"] = (ds_floor @ k.abs() + math.sqrt(K) * U32 * (a @ k.abs())) * scale
    floor["dk"] = (ds_floor.transpose(-1, -2) @ q.abs() + math.sqrt(Q) * U32 * (a.transpose(-1, -2) @ q.abs())) * scale
    floor["dv"] = (pw_abs * rel_p).transpose(-1, -2) @ g.abs() + math.sqrt(Q) * U32 * (pw_abs.transpose(-1, -2) @ g.abs())
    if post is not None:
        floor["dbs"] = math.sqrt(B * Q * hd) * U32 * (g.abs() * res["u"].abs()).sum((0, 2, 3)) + (g.abs() * floor["u"]).sum((0, 2, 3))
    return res


def rounding_model(dt, **form):
    """`flash` with the kernels' documented rounding sites in `dt`; `form`: the keyword arguments that make the form (round_p, out_dt, grad_dt included)."""
    return lambda q, k, v, dout=None, **kw: flash(q, k, v, dout, dt=dt, **form, **kw)


# ---- forms: the extra operands of each member of the family, from its raw inputs ------------------------------------------------------------------
def alibi_train_form(coords, bias_scale, running_mean):
    """Post-softmax ALiBi in TRAIN mode (mask = None): out = softmax(.) v - bias_scale_h (cdist / running_mean_h) v."""
    dist = torch.cdist(coords.double(), coords.double())[:, None]
    ref = dict(post=dist / running_mean.double().view(1, -1, 1, 1), bias_scale=bias_scale)
    mod = dict(post=dist, post_scale=1.0 / running_mean.double(), bias_scale=bias_scale, out_dt=torch.bfloat16)
    return ref, mod


def alibi_infer_form(coords, head_scale, blocked=None):
    """amds_attention_alibi / _alibi_masked: head_scale_h = bias_scale_h / running_mean_h in one operand; masked: blocked products zeroed after the softmax,
    no distance term on the class token's row and column (:62-70, :370-372)."""
    H = head_scale.numel()
    dist = torch.cdist(coords.double(), coords.double())[:, None].expand(-1, H, -1, -1).clone()
    if blocked is not None:
        dist[..., 0, :] = 0
        dist[..., :, 0] = 0
    one = torch.ones(H, dtype=torch.float64, device=coords.device)
    ref = dict(post=dist * head_scale.double().view(1, H, 1, 1), bias_scale=one, zero=blocked)
    mod = dict(post=dist, post_scale=head_scale.double(), bias_scale=None, zero=blocked, out_dt=torch.bfloat16)
    return ref, mod


def distbias_form(coords, slopes):
    """TICON's pre-softmax distance bias: softmax(q k^T / 8 - slope_h |c_q - c_k|) v."""
    c = coords.double()
    dist = torch.sqrt(((c[:, :, None, :] - c[:, None, :, :]) ** 2).sum(-1))
    return dict(pre_bias=-slopes.double().view(1, -1, 1, 1) * dist[:, None])


# ---- errors and bars -------------------------------------------------------------------------------------------------------------------------------
def errors(got: dict, ref: dict) -> dict:
    """Per tensor, never jointly: name -> (relative L2 |got - ref| / |ref|, max-abs / the tensor's own |ref|max); lse: absolute, log2 units, in both slots.
    A zero reference gives 0 for a zero error and inf otherwise: there is no floor here."""
    out = {}
    for n, r in ref.items():
        if n == "floor" or n not in got:
            continue
        d = (got[n].double() - r.double())
        if n == "lse":
            a = d.abs().max().item()
            out[n] = (a, a)
            continue
        dn, dm, rn_, rm = d.norm().item(), d.abs().max().item(), r.double().norm().item(), r.double().abs().max().item()
        out[n] = (dn / rn_ if rn_ > 0 else (0.0 if dn == 0 else math.inf), dm / rm if rm > 0 else (0.0 if dm == 0 else math.inf))
    return out


def abs_errors(got: dict, ref: dict) -> dict:
    """name -> (|got - ref|_2, |got - ref|_max), the numerators of `errors`."""
    return {n: ((got[n].double() - r.double()).norm().item(), (got[n].double() - r.double()).abs().max().item())
            for n, r in ref.items() if n != "floor" and n in got}


def bars(model: dict, ref: dict) -> dict:
    """name -> (L2 bar, max-abs bar), absolute: factor x (the rounding model's error + the fp32 floor of that tensor).  Computed from references alone."""
    me = abs_errors(model, ref)
    out = {}
    for n, (l2, mx) in me.items():
        f = model["floor"].get(n)
        fl2, fmx = (f.norm().item(), f.abs().max().item()) if f is not None else (0.0, 0.0)
        k = FWD_FACTOR if n in FWD_TENSORS else BWD_FACTOR
        out[n] = (k * (l2 + fl2), k * (mx + fmx))
    return out


def judge(got: dict, model: dict, ref: dict, names=None) -> dict:
    """name -> (error / bar in L2, in max-abs, relative L2 error, model's relative L2 error); a value > 1 in the first two misses the bar."""
    b, e, rel, mrel = bars(model, ref), abs_errors(got, ref), errors(got, ref), errors(model, ref)
    out = {}
    for n in (names or e.keys()):
        (el2, emx), (bl2, bmx) = e[n], b[n]
        out[n] = (el2 / bl2 if bl2 > 0 else (0.0 if el2 == 0 else math.inf), emx / bmx if bmx > 0 else (0.0 if emx == 0 else math.inf), rel[n][0], mrel[n][0])
    return out


def old_joint_bar_accepts(got: dict, ref: dict, dt) -> bool:
    """The family's existing bar (test_attention_train_forward_backward): out 4 eps max(1, |ref|max), lse 1e-2, dq | dk | dv JOINTLY 8 eps max(1, |grad|max)."""
    e = eps(dt)
    ok = (got["out"] - ref["out"]).abs().max().item() < 4 * e * max(1.0, ref["out"].abs().max().item())
    ok &= (got["lse"] - ref["lse"]).abs().max().item() < 1e-2
    gmax = max(ref[n].abs().max().item() for n in ("dq", "dk", "dv"))
    err = max((got[n] - ref[n]).abs().max().item() for n in ("dq", "dk", "dv"))
    return bool(ok and err < 8 * e * max(1.0, gmax))


# ---- mutants: faults of the reference computation, never of a kernel ----------------------------------------------------------------------------------
MUTANTS = {
    "drop key T-1": ("drop_last_key",),
    "skip key tile 1 for query block 0": ("skip_tile", 1, 0),
    "skip the last key tile for the last query block": ("skip_tile", "last", "last"),
    "pad keys of the last tile counted in l": ("pad_in_l",),
    "no rescale of O at tile 1": ("no_rescale_o", 1),
    "no rescale of l at tile 1": ("no_rescale_l", 1),
    "no rescale of O at the last tile": ("no_rescale_o", "last"),
    "dropout pair bits swapped in tile 0": ("swap_pair_bits", 0),
    "dropout pair bits swapped in the last full tile": ("swap_pair_bits", "last_full"),
    "mask of head (h + 1) mod H": ("mask_next_head",),
    "mask of query row q + 1": ("mask_next_row",),
    "-P D omitted": ("omit_pd",),
    "dq x 0.9": ("scale_grad", "dq", 0.9),
    "dk x 0.9": ("scale_grad", "dk", 0.9),
    "dv x 0.9": ("scale_grad", "dv", 0.9),
    "dk of the last key = 0": ("zero_last_key_grad", "dk"),
    "dv of the last key = 0": ("zero_last_key_grad", "dv"),
    "keep scale dropped": ("drop_keep_scale",),
}


def resolve_fault(fault, Q, K):
    """'last' -> the last key tile / query block of this shape."""
    nt, nb = (K + TILE - 1) // TILE, (Q + QBLOCK - 1) // QBLOCK
    if fault[0] == "skip_tile":
        return (fault[0], nt - 1 if fault[1] == "last" else fault[1], nb - 1 if fault[2] == "last" else fault[2])
    if fault[0] in ("no_rescale_o", "no_rescale_l", "swap_pair_bits"):
        return (fault[0], nt - 1 if fault[1] == "last" else max(K // TILE - 1, 0) if fault[1] == "last_full" else fault[1])
    return fault
