"""Every launch of the training row kernels (stamp_amd/csrc/train.hip) and the element-wise dropout sites (stamp_amd/csrc/dropout.hip) against fp64, through the
C ABI, element by element.

References, inputs, bars and the dropout-mask rule: tests/train_rows_oracle.py (pinned on the CPU by test_cpu_train_rows_oracle.py).  EVERY mask here is the
oracle's numpy restatement of the rule; the library's own mask entries (amds_dropout_mask, amds_attention_dropout_mask(_rows), amds_dropout_keep_scale) are held to
it bit for bit.  Two families:

* grid -- integer operands whose every partial sum is exact in fp32 (asserted on the CPU): column sums, d(beta), dropout_add / cast_bwd / ReLU at power-of-two keep
  scales must equal fp64 BIT FOR BIT on every route.
* real -- Gaussian operands and the planted edges, |got - ref| <= the oracle's bar PER ELEMENT.

Every operand sits in a tests/guarded.py allocation (1 MiB bands of 0xFF around it, pitch padding and the elements in front of an offset pointer 0xFF as well);
outputs and workspaces are 0xFF (NaN) everywhere before the call; bands, padding and offsets must survive it.  Every call runs twice on fresh buffers and must
repeat its bits.  Each check prints `trainrows| kernel | variant | family | case | error / bar` under -s and the module ends with the worst figure per kernel and
variant: profiles/train_rows_kernel_errors.txt is that table from one run.

fp16 copies of the LayerNorm backward are reached only through csrc-internal layernorm_bwd_partials_dt (no C entry): left to the whole-step chain tests; every bf16
form is here.  Rows crossing 65 536 x cols boundaries mean nothing to amds_attention_dropout_rows and the attention masks: the ROW is the key there, not the flat index.
amds_grad_unscale_check's two caps (2048 blocks, VEC and scalar) are passed by test_gpu_loss_scale.py::test_unscale_check_counts_and_bits (n = 2^20 + 3 on an odd
pointer, n = 3 700 001 aligned) and not repeated.

Which case reaches which launch (t: = train.hip line, d: = dropout.hip line of the hipLaunchKernelGGL; every launch of the entry points below is named once):

  amds_transpose16
    R, Cc multiples of 64, pitches multiples of 8, both pointers 16-byte aligned      transpose16_vec_kernel           t:440
    R or Cc of 1, 63, 65; each of the six conditions failed alone                     transpose16_kernel               t:443
  amds_cast_transpose_multi        64 x 64, 128 x 64, 64 x 192, both dtypes, with and without dst_t      cast_transpose_multi_kernel      t:519
  amds_sum_partials_multi          rows 1 .. 2048, two entries                        sum_partials_multi_kernel        t:577
  amds_colsum / _partials
    every M x N x dtype; N >= 4 on aligned rows: vector branch (:81), N 130's last two columns, N < 4, odd pitch, odd pointer: scalar branch (:98)
                                                                                     colsum_partial_kernel<f32|bf16|f16>      t:593
    M 2049 (3 chunks, the last of one row), 4097 (5 chunks); accumulate = 1 at any M  colsum_final_kernel              t:613
  amds_colsum_multi                kind 0 (fp32, M <= 2048), kind 1 (chunk partials); 33 entries = two launches       colsum_multi_kernel      t:643
  amds_layernorm_train / _train_copy      cols 4, 508, 512 / 516, 1024 / 1028, 2048 -> ln_train_kernel<f32|bf16|f16, 2 / 4 / 8>      t:667
    rows 1, 3, 4, 5 (four rows per workgroup); copy_cols = cols + 4: the loop at :176; rows = 0 launches nothing
  amds_layernorm_bwd / _bwd_cast / _bwd_partials      the same cols -> ln_bwd_kernel<2 / 4 / 8, bf16>      t:707
    rows 1, 63, 64, 65, 130; cols 2048: 8 * 2048 * 4 = 65 536 bytes of dynamic LDS (rows 65: two blocks of it); the finish is amds_colsum (t:593, t:613 under accumulate_params)
  amds_gelu_fwd      fp32 z, 16-bit z with n % 8 != 0 or an odd pointer     gelu_fwd_kernel<TZ, TO>      t:758      (else -> amds_gelu_dropout_fwd at p = 0)
  amds_gelu_bwd      the same                                               gelu_bwd_kernel<TZ, TG, TZ>  t:779      (else -> amds_gelu_dropout_bwd at p = 0)
  amds_adamw         three hyper-parameter cases; n = 2^20 + 257: second trip     adamw_kernel              t:792
  amds_adamw_guarded clean state: amds_adamw's bits; after two skipped steps: t = step - 2; n = 2^20 + 257      adamw_guarded_kernel      t:824
  amds_gelu_dropout_fwd_rows / _bwd_rows / amds_dropout_add_rows / amds_dropout_cast_bwd_rows      3 x 520, row_mul 1, 9, 2^23, 2^40; 2017 x 520: second trip
                                                                                     gelu_dropout_fwd_rows_kernel d:312, gelu_dropout_bwd_rows_kernel d:330,
                                                                                     dropout_add_rows_kernel d:346, dropout_cast_bwd_rows_kernel<bf16> d:359
  amds_gelu_dropout_fwd      16-bit z, n % 8 == 0, aligned (n 8, 65 544, 8 * (2^21 + 3))      gelu_dropout_fwd8_kernel      d:386
                             fp32 z; n 12; a pointer 2 bytes off; n = 2^21 + 257               gelu_dropout_fwd_kernel       d:389
  amds_gelu_dropout_bwd      the same                                                          gelu_dropout_bwd8_kernel d:413 / gelu_dropout_bwd_kernel d:417
  amds_relu_dropout_fwd      the same                                                          relu_dropout_fwd8_kernel d:440 / relu_dropout_fwd_kernel d:443
  amds_relu_dropout_bwd      the same                                                          relu_dropout_bwd8_kernel d:466 / relu_dropout_bwd_kernel d:470
  amds_attention_dropout_rows        cols 1, 2, 3, 257, in place and out of place; 8161 x 257: second trip      attn_dropout_rows_kernel      d:483
  amds_attention_dropout_mask_rows   the same shapes                                                            attn_dropout_mask_rows_kernel d:491
  amds_dropout_add           cols 264 on pitch 272, aligned (37 rows; 63 551 rows: second trip)      dropout_add8_kernel      d:502
                             cols 260; pitch 262; a pointer 4 bytes off; 8068 x 260: second trip       dropout_add_kernel       d:505
  amds_dropout_cast_bwd      bf16 / fp16, cols 264, aligned                                          dropout_cast_bwd8_kernel<bf16|f16>      d:522
                             fp32 output; cols 260; pitch 262; odd pointer; 7946 x 264 to fp32        dropout_cast_bwd_kernel<f32|bf16|f16>    d:525
  amds_dropout_mask          n = 65 544 at every rate; n = 2^21 + 257: second trip                   dropout_mask_kernel           d:535
  amds_attention_dropout_mask      (B, H, T) = (2, 3, 1 | 2 | 3 | 257)                                attn_dropout_mask_kernel      d:544
"""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as G
import train_rows_oracle as O
from stamp_amd import _lib
from stamp_amd import train_ops as T

pytestmark = pytest.mark.gpu
F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
DT = {F32: _lib.F32, BF16: _lib.BF16, F16: _lib.F16}
NAME = {F32: "f32", BF16: "bf16", F16: "f16", torch.uint8: "u8"}
FAMILIES = ("grid", "real")
ERR_INVALID = -1
SEED, SID = 0x5EED0123456789AB, 13          # a seed with a high word
_WORST: dict = {}


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---- operands ----------------------------------------------------------------------------------------------------------------------------------------------
class Buf:
    """rows x cols elements at pitch ld, `offset` elements behind the 256-byte aligned start of a guarded allocation; 0xFF wherever no data was loaded."""

    def __init__(self, gpu, shape, dtype, ld=None, offset=0, data=None, name="buf"):
        self.flat1d = isinstance(shape, int)
        rows, cols = (1, shape) if self.flat1d else shape
        self.rows, self.cols, self.ld, self.off = rows, cols, cols if ld is None else ld, offset
        self.item = torch.empty((), dtype=dtype).element_size()
        self.total = offset + max(rows, 1) * self.ld
        self.flat, self.h = G.guarded((self.total,), dtype, gpu, name=name)
        self.view = self.flat[offset:offset + rows * self.ld].view(rows, self.ld)[:, :cols]
        if data is not None:
            self.view.copy_(data.reshape(rows, cols))

    def ptr(self):
        return self.flat.data_ptr() + self.off * self.item

    def check(self):
        torch.cuda.synchronize()
        self.h.assert_bands_intact()
        if self.off or self.ld > self.cols or self.rows == 0:
            inside = torch.zeros(self.total, dtype=torch.bool, device=self.flat.device)
            inside[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = True
            raw = self.flat.view(torch.uint8).view(self.total, self.item)
            assert bool((raw[~inside] == 0xFF).all()), f"{self.h.name}: pitch padding or the elements in front of the pointer were written"

    def cpu(self):
        self.check()
        out = self.view.cpu().clone()
        return out.reshape(-1) if self.flat1d else out


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _twice(run):
    """run() -> dict of CPU tensors from fresh buffers; twice, bit for bit."""
    a, b = run(), run()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{k}: the second call did not repeat the first one's bits"
    return a


def _judge(kernel, variant, family, case, got, ref, bar=None):
    """bar None: equal to the fp64 value (bit for bit: every grid value is representable).  Non-finite wanted values must come back as the same non-finite
    values.  Prints the figure, keeps the worst per (kernel, variant, family), then asserts."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, f"{kernel} {variant} {case}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    nf = ~torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[torch.isinf(ref)], ref[torch.isinf(ref)]) and bool(torch.isfinite(got[~nf]).all()), \
        f"{kernel} [{variant}] {family} {case}: non-finite values differ from the reference's (an element never written reads as NaN)"
    err = torch.where(nf, torch.zeros_like(ref), (got - ref).abs())
    if bar is None:
        ratio = 0.0 if bool((err == 0).all()) else float("inf")
        where = "" if ratio == 0.0 else f"{int((err != 0).sum())} element(s) differ, first at flat index {int((err != 0).reshape(-1).nonzero()[0])}, largest difference {float(err.max()):.6g}"
    else:
        r = torch.where(err == 0, torch.zeros_like(err), err / bar)
        ratio = float(r.max()) if r.numel() else 0.0
        i = int(r.reshape(-1).argmax()) if r.numel() else 0
        where = f"flat index {i}: got {float(got.reshape(-1)[i])!r} want {float(ref.reshape(-1)[i])!r}, error {float(err.reshape(-1)[i]):.6g}" if r.numel() else ""
    print(f"trainrows| {kernel} | {variant} | {family} | {case} | {ratio:.3f}")
    key = (kernel, variant, family)
    if key not in _WORST or ratio > _WORST[key][0]:
        _WORST[key] = (ratio, case)
    assert ratio <= 1.0, f"{kernel} [{variant}] {family} {case}: error / bar = {ratio:.4g}; {where}"


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\ntrainrows-worst| kernel | variant | family | worst error / bar | at case")
    for (kernel, variant, family), (ratio, case) in sorted(_WORST.items()):
        print(f"trainrows-worst| {kernel} | {variant} | {family} | {ratio:.3f} | {case}")


def _up4(n):
    return (n + 3) // 4 * 4


# ==== the mask entries are the rule ================================================================================================================================
def test_keep_scale_is_the_rule(gpu):
    lib = _lib.lib()
    for p in O.DROP_RATES + (0.3, 0.75, 1e-6, 0.999999):
        assert lib.amds_dropout_keep_scale(p) == O.drop_scale(O.drop_thr16(p)), p


@pytest.mark.parametrize("p", O.DROP_RATES)
def test_dropout_mask_is_the_rule(gpu, p):
    lib, thr = _lib.lib(), O.drop_thr16(p)
    sizes = (65536 + 8, (1 << 21) + 257) if p == 0.25 else (65536 + 8,)          # the second: dropout_mask_kernel's 8192-block cap
    for n in sizes:
        def run():
            m = Buf(gpu, n, torch.uint8, name="mask")
            _lib.check(lib.amds_dropout_mask(m.ptr(), n, p, SEED, SID, _st()), "dropout_mask")
            return dict(mask=m.cpu())
        want = torch.from_numpy(O.keep_flat(SEED, SID, np.arange(n, dtype=np.int64), thr).astype(np.uint8))
        _judge("amds_dropout_mask", "dropout_mask_kernel", "rule", f"n={n} p={p:g}", _twice(run)["mask"], want)


@pytest.mark.parametrize("cols", [1, 2, 3, 257])
def test_attention_masks_are_the_rule(gpu, cols):
    lib = _lib.lib()
    for p in O.DROP_RATES:
        thr = O.drop_thr16(p)
        B, H = 2, 3
        rows = B * H * cols

        def run():
            m = Buf(gpu, (rows, cols), torch.uint8, name="attention mask")
            _lib.check(lib.amds_attention_dropout_mask(m.ptr(), B, H, cols, p, SEED, SID, _st()), "attention_dropout_mask")
            m2 = Buf(gpu, (5, cols), torch.uint8, name="mask rows")
            _lib.check(lib.amds_attention_dropout_mask_rows(m2.ptr(), 5, cols, p, SEED, SID, _st()), "attention_dropout_mask_rows")
            return dict(full=m.cpu(), rows=m2.cpu())
        o = _twice(run)
        ar = lambda n: np.arange(n, dtype=np.int64)          # noqa: E731
        _judge("amds_attention_dropout_mask", "attn_dropout_mask_kernel", "rule", f"B=2 H=3 T={cols} p={p:g}", o["full"],
               torch.from_numpy(O.keep_rows(SEED, SID, ar(rows)[:, None], ar(cols)[None, :], thr).astype(np.uint8)))
        _judge("amds_attention_dropout_mask_rows", "attn_dropout_mask_rows_kernel", "rule", f"5 x {cols} p={p:g}", o["rows"],
               torch.from_numpy(O.keep_rows(SEED, SID, ar(5)[:, None], ar(cols)[None, :], thr).astype(np.uint8)))


# ==== column sums ================================================================================================================================================
def _colsum_case(gpu, M, N, dt, family, ld=None, offset=0, accumulate=0):
    lib = _lib.lib()
    ld = _up4(N) + 4 if ld is None else ld
    x0 = O.colsum_inputs(M, N, family, dt)
    old0 = O.ints(O._gen(5, M, N), (N,)) if family == "grid" else torch.randn(N, generator=O._gen(5, M, N))
    nb = lib.amds_colsum_workspace_bytes(M, N)
    nchunk_want = 1 if M <= 2048 else (M + 1023) // 1024

    def run():
        x = Buf(gpu, (M, N), dt, ld, offset, x0, "x")
        out, ws = Buf(gpu, N, F32, data=old0 if accumulate else None, name="out"), Buf(gpu, max(nb, 4), torch.uint8, name="ws")
        _lib.check(lib.amds_colsum(x.ptr(), ld, out.ptr(), M, N, DT[dt], accumulate, ws.ptr(), nb, _st()), "colsum")
        res = dict(out=out.cpu())
        ws.check()
        if not accumulate:
            part, out1 = Buf(gpu, (nchunk_want, N), F32, name="partials"), Buf(gpu, N, F32, name="out kind 1")
            nchunk = C.c_int(0)
            _lib.check(lib.amds_colsum_partials(x.ptr(), ld, part.ptr(), M, N, DT[dt], C.byref(nchunk), _st()), "colsum_partials")
            assert nchunk.value == nchunk_want
            entries = [_lib.ColsumEntry(part.ptr(), out1.ptr(), N, nchunk.value, N, 1)]
            out0 = None
            if dt == F32 and M <= 2048:
                out0 = Buf(gpu, N, F32, name="out kind 0")
                entries.append(_lib.ColsumEntry(x.ptr(), out0.ptr(), ld, M, N, 0))
            _lib.check(lib.amds_colsum_multi((_lib.ColsumEntry * len(entries))(*entries), len(entries), _st()), "colsum_multi")
            res["kind1"] = out1.cpu()
            part.check()
            if out0 is not None:
                res["kind0"] = out0.cpu()
        assert torch.equal(_bits(x.cpu()), _bits(x0))
        return res

    o = _twice(run)
    ref, ab = O.colsum(x0, old0 if accumulate else None)
    vec = ld % 4 == 0 and (offset * x0.element_size()) % (4 * x0.element_size()) == 0 and N >= 4
    variant = f"{NAME[dt]} {'vector' if vec else 'scalar'} branch, {'1 chunk' if nchunk_want == 1 else 'chunks + final'}" + (" accumulate" if accumulate else "")
    case = f"M={M} N={N}" + (f" ld={ld}" if ld % 4 else "") + (f" +{offset} element" if offset else "")
    _judge("amds_colsum", variant, family, case, o["out"], ref, None if family == "grid" else O.colsum_bar(M + accumulate, ab))
    for k in ("kind1", "kind0"):
        if k in o:
            assert torch.equal(_bits(o[k]), _bits(o["out"])), f"amds_colsum_multi {k} differs from amds_colsum at {case}"


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("M", O.COLSUM_M)
def test_colsum(gpu, dt, M):
    for N in O.COLSUM_N:
        for family in FAMILIES:
            _colsum_case(gpu, M, N, dt, family)


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_colsum_without_the_vector_path_and_with_accumulate(gpu, dt):
    for family in FAMILIES:
        for M, N in ((65, 130), (17, 64), (2049, 64)):
            _colsum_case(gpu, M, N, dt, family, ld=N + 1)                   # a pitch that is no multiple of 4
            _colsum_case(gpu, M, N, dt, family, offset=1)                   # a pointer one element off
        for M in (1, 65, 2048, 2049, 4097):
            _colsum_case(gpu, M, 130, dt, family, accumulate=1)


def test_colsum_multi_33_entries(gpu):
    """Mixed kinds through the wrapper (fp32 with M <= 2048 -> kind 0, the rest -> amds_colsum_partials + kind 1): 33 entries are two launches."""
    shapes = [(O.COLSUM_M[i % len(O.COLSUM_M)], O.COLSUM_N[(i * 3) % len(O.COLSUM_N)], (F32, F32, BF16)[i % 3]) for i in range(33)]
    assert sum(1 for M, _, dt in shapes if dt == F32 and M <= 2048) >= 8 and sum(1 for M, _, dt in shapes if dt != F32 or M > 2048) >= 8
    for family in FAMILIES:
        xs0 = [O.colsum_inputs(M, N, family, dt) for M, N, dt in shapes]
        run = lambda: {str(i): t.cpu() for i, t in enumerate(T.colsum_multi([x.to(gpu) for x in xs0]))}          # noqa: E731
        o = _twice(run)
        for i, ((M, N, dt), x0) in enumerate(zip(shapes, xs0)):
            ref, ab = O.colsum(x0)
            _judge("amds_colsum_multi", "kind 0" if dt == F32 and M <= 2048 else "kind 1", family, f"entry {i}: M={M} N={N} {NAME[dt]}", o[str(i)], ref,
                   None if family == "grid" else O.colsum_bar(M, ab))


@pytest.mark.parametrize("rows", O.SUM_PARTIALS_ROWS)
def test_sum_partials_multi_is_colsum_bit_for_bit(gpu, rows):
    """include/amdstamp.h: "the association of amds_colsum ... (same bits, for every row count 1 .. 2048 the call accepts)" -- 49 rows is where a plain in-order sum
    per row lane stops agreeing (test_cpu_train_rows_oracle.py)."""
    lib, counts = _lib.lib(), (260, 8)
    for family in FAMILIES:
        parts0 = [O.colsum_inputs(rows, c, family) for c in counts]

        def run():
            pin = [Buf(gpu, (rows, c), F32, data=p0, name="partials") for c, p0 in zip(counts, parts0)]
            pout = [Buf(gpu, c, F32, name="sum of partials") for c in counts]
            arr = lambda bs: (C.c_void_p * 2)(*[b.ptr() for b in bs])          # noqa: E731
            _lib.check(lib.amds_sum_partials_multi(arr(pin), arr(pout), (C.c_long * 2)(*counts), 2, rows, _st()), "sum_partials_multi")
            res = {f"multi{i}": b.cpu() for i, b in enumerate(pout)}
            for i, (c, b) in enumerate(zip(counts, pin)):
                nb = lib.amds_colsum_workspace_bytes(rows, c)
                out, ws = Buf(gpu, c, F32, name="colsum"), Buf(gpu, max(nb, 4), torch.uint8, name="ws")
                _lib.check(lib.amds_colsum(b.ptr(), c, out.ptr(), rows, c, _lib.F32, 0, ws.ptr(), nb, _st()), "colsum")
                res[f"colsum{i}"] = out.cpu()
            return res

        o = _twice(run)
        for i, (c, p0) in enumerate(zip(counts, parts0)):
            ref, ab = O.colsum(p0)
            _judge("amds_sum_partials_multi", "sum_partials_multi_kernel", family, f"rows={rows} count={c}", o[f"multi{i}"], ref,
                   None if family == "grid" else O.colsum_bar(rows, ab))
            assert torch.equal(_bits(o[f"multi{i}"]), _bits(o[f"colsum{i}"])), f"rows={rows} count={c} {family}: not amds_colsum's bits"


# ==== LayerNorm forward ===========================================================================================================================================
def _maxv(cols):
    return 2 if cols <= 512 else 4 if cols <= 1024 else 8


@pytest.mark.parametrize("cols", O.LN_COLS)
def test_layernorm_train(gpu, cols):
    lib = _lib.lib()
    ldx, ldy, ldc, ccols = cols + 8, cols + 12, cols + 8, cols + 4
    for rows in O.LN_FWD_ROWS:
        x0, gamma0, beta0, _, _ = O.ln_inputs(rows, cols)
        xw = torch.cat([x0, torch.randn(rows, 4, generator=O._gen(6, rows, cols))], 1)          # the columns behind the row: only the copy reads them
        f = O.layernorm_fwd(x0, gamma0, beta0)
        for odt in (F32, BF16, F16):
            def run():
                x, gam, bet = Buf(gpu, (rows, ccols), F32, ldx, 0, xw, "x"), Buf(gpu, cols, F32, data=gamma0, name="gamma"), Buf(gpu, cols, F32, data=beta0, name="beta")
                y, mean, rstd = Buf(gpu, (rows, cols), odt, ldy, name="y"), Buf(gpu, rows, F32, name="mean"), Buf(gpu, rows, F32, name="rstd")
                _lib.check(lib.amds_layernorm_train(x.ptr(), ldx, gam.ptr(), bet.ptr(), y.ptr(), ldy, mean.ptr(), rstd.ptr(), rows, cols, O.LN_EPS, DT[odt], _st()), "ln_train")
                y2, mean2, rstd2 = Buf(gpu, (rows, cols), odt, ldy, name="y2"), Buf(gpu, rows, F32, name="mean2"), Buf(gpu, rows, F32, name="rstd2")
                xc = Buf(gpu, (rows, ccols), F32, ldc, name="x_copy")
                _lib.check(lib.amds_layernorm_train_copy(x.ptr(), ldx, gam.ptr(), bet.ptr(), y2.ptr(), ldy, mean2.ptr(), rstd2.ptr(), rows, cols, O.LN_EPS, DT[odt], xc.ptr(),
                                                         ldc, ccols, _st()), "ln_train_copy")
                return dict(y=y.cpu(), mean=mean.cpu(), rstd=rstd.cpu(), y2=y2.cpu(), mean2=mean2.cpu(), rstd2=rstd2.cpu(), xc=xc.cpu())

            o = _twice(run)
            variant, case = f"ln_train_kernel<{NAME[odt]}, {_maxv(cols)}>", f"rows={rows} cols={cols}"
            _judge("amds_layernorm_train", variant, "real", case + " y", o["y"], f["y"], f["d_y"] + O.half_ulp(f["y"], odt))
            _judge("amds_layernorm_train", variant, "real", case + " mean", o["mean"], f["mean"], f["d_mean"])
            _judge("amds_layernorm_train", variant, "real", case + " rstd", o["rstd"], f["rstd"], f["d_rstd"])
            for k in ("y", "mean", "rstd"):
                assert torch.equal(_bits(o[k]), _bits(o[k + "2"])), f"amds_layernorm_train_copy's {k} differs from amds_layernorm_train's at {case}"
            assert torch.equal(_bits(o["xc"]), _bits(xw)), f"x_copy is not a copy at {case} (copy_cols = cols + 4)"


def test_layernorm_train_zero_rows(gpu):
    lib, cols = _lib.lib(), 512
    y, mean, gam = Buf(gpu, (0, cols), BF16, name="y"), Buf(gpu, 4, F32, name="mean"), Buf(gpu, cols, F32, data=torch.ones(cols), name="gamma")
    assert lib.amds_layernorm_train(gam.ptr(), cols, gam.ptr(), gam.ptr(), y.ptr(), cols, mean.ptr(), mean.ptr(), 0, cols, O.LN_EPS, _lib.BF16, _st()) == 0
    y.check()
    assert bool((_bits(mean.cpu()) == -1).all())


# ==== LayerNorm backward ==========================================================================================================================================
def _ln_bwd_case(gpu, rows, cols, family, form, add_skip, acc, p):
    lib = _lib.lib()
    ldy, ldx, lddx, ld16 = cols + 4, cols + 8, cols + 12, cols + 16
    x0, gamma0, _, dy0, skip0 = O.ln_inputs(rows, cols, family)
    mean0, rstd0 = O.ln_stats32(x0)
    g = O._gen(7, rows, cols)
    oldg0, oldb0 = (O.ints(g, (cols,)), O.ints(g, (cols,))) if family == "grid" else (torch.randn(cols, generator=g), torch.randn(cols, generator=g))
    nb, nblk = lib.amds_layernorm_bwd_workspace_bytes(rows, cols), (rows + 63) // 64
    want16 = form != "bwd"

    def run():
        dy, x = Buf(gpu, (rows, cols), F32, ldy, data=dy0, name="dy"), Buf(gpu, (rows, cols), F32, ldx, data=x0, name="x")
        mean, rstd, gam = Buf(gpu, rows, F32, data=mean0, name="mean"), Buf(gpu, rows, F32, data=rstd0, name="rstd"), Buf(gpu, cols, F32, data=gamma0, name="gamma")
        dx = Buf(gpu, (rows, cols), F32, lddx, data=skip0 if add_skip else None, name="dx")
        d16 = Buf(gpu, (rows, cols), BF16, ld16, name="dx16") if want16 else None
        p16 = d16.ptr() if want16 else None
        if form == "partials":
            dg, db = Buf(gpu, (nblk, cols), F32, name="dgamma partials"), Buf(gpu, (nblk, cols), F32, name="dbeta partials")
            rc = lib.amds_layernorm_bwd_partials(dy.ptr(), ldy, x.ptr(), ldx, mean.ptr(), rstd.ptr(), gam.ptr(), dx.ptr(), lddx, add_skip, dg.ptr(), db.ptr(), rows, cols,
                                                 p16, ld16, p, SEED, SID, _st())
        else:
            dg, db = Buf(gpu, cols, F32, data=oldg0 if acc else None, name="dgamma"), Buf(gpu, cols, F32, data=oldb0 if acc else None, name="dbeta")
            ws = Buf(gpu, max(nb, 4), torch.uint8, name="ws")
            if form == "bwd":
                rc = lib.amds_layernorm_bwd(dy.ptr(), ldy, x.ptr(), ldx, mean.ptr(), rstd.ptr(), gam.ptr(), dx.ptr(), lddx, add_skip, dg.ptr(), db.ptr(), acc, rows, cols,
                                            ws.ptr(), nb, _st())
            else:
                rc = lib.amds_layernorm_bwd_cast(dy.ptr(), ldy, x.ptr(), ldx, mean.ptr(), rstd.ptr(), gam.ptr(), dx.ptr(), lddx, add_skip, dg.ptr(), db.ptr(), acc, rows, cols,
                                                 ws.ptr(), nb, p16, ld16, p, SEED, SID, _st())
        _lib.check(rc, form)
        res = dict(dx=dx.cpu(), dg=dg.cpu(), db=db.cpu())
        if want16:
            res["d16"] = d16.cpu()
        if form != "partials":
            ws.check()
        return res

    o = _twice(run)
    b = O.layernorm_bwd(dy0, x0, mean0, rstd0, gamma0, skip0 if add_skip else None)
    kernel = {"bwd": "amds_layernorm_bwd", "cast": "amds_layernorm_bwd_cast", "partials": "amds_layernorm_bwd_partials"}[form]
    variant = f"ln_bwd_kernel<{_maxv(cols)}, bf16>"
    case = f"rows={rows} cols={cols} add_skip={add_skip}" + (f" accumulate={acc}" if form != "partials" else "") + (f" p={p:g}" if want16 else "")
    _judge(kernel, variant, family, case + " dx", o["dx"], b["dx"], b["d_dx"])
    for key, got in (("t_gamma", o["dg"]), ("t_beta", o["db"])):
        part, pbar = O.ln_param_partials(b[key])
        exact = family == "grid" and key == "t_beta"
        if form == "partials":
            _judge(kernel, variant, family, f"{case} {key[2:]} partials", got, part, None if exact else pbar)
        else:
            val, bar = O.ln_param_finish(part, pbar, (oldg0 if key == "t_gamma" else oldb0) if acc else None)
            _judge(kernel, variant, family, f"{case} d{key[2:]}", got, val, None if exact else bar)
    if want16:
        mult = O.mult_flat(SEED, SID, np.arange(rows * cols, dtype=np.int64), p).view(rows, cols) if p > 0 else torch.ones(rows, cols, dtype=F64)
        want = b["dx"] * mult
        _judge(kernel, variant + " 16-bit copy", family, case + " dx16", o["d16"], want, b["d_dx"] * mult + O.EPS * want.abs() + O.half_ulp(want, BF16))


@pytest.mark.parametrize("cols", O.LN_COLS)
@pytest.mark.parametrize("rows", O.LN_BWD_ROWS)
def test_layernorm_bwd(gpu, rows, cols):
    """cols 2048: 65 536 bytes of dynamic LDS, exactly the default limit (rows 65 and 130 launch two and three such blocks)."""
    for add_skip in (0, 1):
        for acc in (0, 1):
            _ln_bwd_case(gpu, rows, cols, "real", "bwd", add_skip, acc, 0.0)
    _ln_bwd_case(gpu, rows, cols, "grid", "bwd", 1, 1, 0.0)
    for p in (0.0, 0.25):
        _ln_bwd_case(gpu, rows, cols, "real", "cast", 1, 0, p)
        _ln_bwd_case(gpu, rows, cols, "real", "partials", 0, 0, p)
    _ln_bwd_case(gpu, rows, cols, "grid", "partials", 1, 0, 0.25)


# ==== transposes: copies, bit for bit ===================================================================================================================================
def _transpose_case(gpu, R, Cc, ld_src, ld_dst, off_src=0, off_dst=0):
    lib = _lib.lib()
    x0 = torch.randn(R, Cc, generator=O._gen(8, R, Cc)).bfloat16()

    def run():
        x, t = Buf(gpu, (R, Cc), BF16, ld_src, off_src, x0, "src"), Buf(gpu, (Cc, R), BF16, ld_dst, off_dst, name="dst")
        _lib.check(lib.amds_transpose16(x.ptr(), ld_src, t.ptr(), ld_dst, R, Cc, _st()), "transpose16")
        return dict(t=t.cpu())

    vec = R % 64 == 0 and Cc % 64 == 0 and ld_src % 8 == 0 and ld_dst % 8 == 0 and off_src % 8 == 0 and off_dst % 8 == 0
    _judge("amds_transpose16", "transpose16_vec_kernel" if vec else "transpose16_kernel", "copy", f"R={R} Cc={Cc} ld={ld_src}/{ld_dst} +{off_src}/{off_dst}",
           _twice(run)["t"].float(), x0.t().float())


def test_transpose16(gpu):
    for R in (1, 63, 64, 65):
        for Cc in (1, 63, 64, 65):
            _transpose_case(gpu, R, Cc, Cc + 8, R + 8)
    _transpose_case(gpu, 128, 64, 72, 136)                                   # the vector path, then each of its six conditions failed alone
    for kw in (dict(R=127), dict(Cc=63), dict(ld_src=68), dict(ld_dst=132), dict(off_src=1), dict(off_dst=1)):
        _transpose_case(gpu, **{**dict(R=128, Cc=64, ld_src=72, ld_dst=136), **kw})


def test_cast_transpose_multi(gpu):
    lib = _lib.lib()
    shapes = [(64, 64, BF16, True), (128, 64, F16, True), (64, 192, BF16, False), (64, 192, F16, True)]
    srcs = [torch.randn(r, c, generator=O._gen(9, r, c)) for r, c, _, _ in shapes]

    def run():
        arr, keep, res = (_lib.CastEntry * len(shapes))(), [], {}
        for j, ((r, c, dt, tr), s0) in enumerate(zip(shapes, srcs)):
            s, d = Buf(gpu, (r, c), F32, c + 4, data=s0, name=f"src{j}"), Buf(gpu, (r, c), dt, c + 8, name=f"dst{j}")
            dtp = Buf(gpu, (c, r), dt, r + 8, name=f"dst_t{j}") if tr else None
            arr[j] = _lib.CastEntry(s.ptr(), c + 4, d.ptr(), c + 8, dtp.ptr() if tr else None, r + 8 if tr else 0, r, c, DT[dt])
            keep.append((s, d, dtp))
        _lib.check(lib.amds_cast_transpose_multi(arr, len(shapes), _st()), "cast_transpose_multi")
        for j, (s, d, dtp) in enumerate(keep):
            res[f"d{j}"] = d.cpu()
            if dtp is not None:
                res[f"t{j}"] = dtp.cpu()
        return res

    o = _twice(run)
    for j, ((r, c, dt, tr), s0) in enumerate(zip(shapes, srcs)):
        _judge("amds_cast_transpose_multi", f"cast to {NAME[dt]}", "copy", f"{r} x {c}", o[f"d{j}"].float(), s0.to(dt).float())
        if tr:
            _judge("amds_cast_transpose_multi", f"transposed {NAME[dt]}", "copy", f"{r} x {c}", o[f"t{j}"].float(), s0.to(dt).t().float())
    # shapes the one kernel cannot take are refused before anything is launched
    for r, c in ((1, 64), (63, 64), (65, 64), (64, 1), (64, 63), (64, 65)):
        s, d = Buf(gpu, (r, c), F32, _up4(c) + 4, data=torch.ones(r, c), name="src"), Buf(gpu, (r, c), BF16, c + 8 - c % 8, name="dst")
        arr = (_lib.CastEntry * 1)(_lib.CastEntry(s.ptr(), s.ld, d.ptr(), d.ld, None, 0, r, c, _lib.BF16))
        assert lib.amds_cast_transpose_multi(arr, 1, _st()) == ERR_INVALID, (r, c)
        assert bool((d.cpu().view(torch.int16) == -1).all())


# ==== GELU / ReLU with dropout, flat ===============================================================================================================================
FWD_PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32))                                   # (z, u)
FWD_REFUSED = ((F32, BF16), (F32, F16), (BF16, F16), (F16, BF16))
BWD_TRIPLES = ((F32, F32, F32), (BF16, BF16, BF16), (BF16, F32, BF16), (F16, F16, F16), (F16, F32, F16))      # (z, du, dz)
BWD_REFUSED = ((BF16, BF16, F32), (F32, F32, BF16), (F16, F16, BF16), (F32, BF16, F32), (F32, F16, F32), (BF16, F16, BF16), (F16, BF16, F16))
ACT_SIZES = ((8, 0), (12, 0), (16, 1), (65536 + 8, 0))          # (n, elements the pointers are off): 8-wide | scalar (n % 8) | scalar (alignment) | a mask-row boundary


def _act_want(act, z0, du0, mult, scale, odt, fwd):
    """-> (want, bar or None) for one flat call; z0, du0 in their storage types, mult the per-element multiplier (0 | scale)."""
    z = z0.double()
    if act == "gelu":
        val, bar = O.gelu(z) if fwd else O.gelu_grad(z)
        if not fwd:
            val, bar = val * du0.double(), bar * du0.double().abs()
        want = torch.where(mult > 0, val * mult, torch.zeros_like(val))
        mag = torch.where(torch.isfinite(want), want.abs(), torch.zeros_like(want))
        wbar = torch.where(torch.isfinite(bar), bar, torch.zeros_like(bar)) * scale + 2 * O.EPS * mag + torch.clamp(O.half_ulp(want, odt), min=0.0 if odt == F32 else 2.0 ** -25)
        return O.saturate(want, odt), wbar
    val = (O.relu(z) if fwd else (z > 0).double() * du0.double()) * mult
    val = torch.where(mult > 0, val, torch.zeros_like(val))
    src = z0.dtype if fwd else du0.dtype          # the factor's type: the product with a power of two is exact in it, and in fp32
    pow2 = O.scale_is_pow2_value(scale)
    if pow2 and odt in (F32, src):
        return O.saturate(val, odt), None
    mag = torch.where(torch.isfinite(val), val.abs(), torch.zeros_like(val))
    return O.saturate(val, odt), (0.0 if pow2 else O.U) * mag + O.half_ulp(val, odt)


def _act_call(lib, act, fwd, z, du, out, n, zt, gt, ot, p, plain):
    if fwd:
        if plain:
            return lib.amds_gelu_fwd(z.ptr(), out.ptr(), n, DT[zt], DT[ot], _st())
        fn = lib.amds_gelu_dropout_fwd if act == "gelu" else lib.amds_relu_dropout_fwd
        return fn(z.ptr(), out.ptr(), n, DT[zt], DT[ot], p, SEED, SID, _st())
    if plain:
        return lib.amds_gelu_bwd(z.ptr(), du.ptr(), out.ptr(), n, DT[zt], DT[gt], DT[ot], _st())
    fn = lib.amds_gelu_dropout_bwd if act == "gelu" else lib.amds_relu_dropout_bwd
    return fn(z.ptr(), du.ptr(), out.ptr(), n, DT[zt], DT[gt], DT[ot], p, SEED, SID, _st())


def _act_case(gpu, act, fwd, types, n, off, p, family, plain=False, sel=None, z0=None, du0=None):
    """One flat call.  plain: amds_gelu_fwd / _bwd (no rate).  sel: compare these flat indices only (the second-trip cases)."""
    lib = _lib.lib()
    zt, gt, ot = (types[0], None, types[1]) if fwd else types
    if z0 is None:
        z0, du0 = O.gelu_inputs(n, zt, family)
        du0 = du0.float().to(gt) if gt is not None else None

    def run():
        z = Buf(gpu, n, zt, offset=off, data=z0, name="z")
        du = Buf(gpu, n, gt, offset=off, data=du0, name="du") if not fwd else None
        out = Buf(gpu, n, ot, offset=off, name="out")
        _lib.check(_act_call(lib, act, fwd, z, du, out, n, zt, gt, ot, p, plain), act)
        return dict(out=out.cpu())

    got = _twice(run)["out"]
    idx = np.arange(n, dtype=np.int64) if sel is None else sel.numpy()
    thr = O.drop_thr16(p)
    scale = O.drop_scale(thr)
    mult = torch.from_numpy(O.keep_flat(SEED, SID, idx, thr).astype(np.float64)) * scale
    pick = (lambda t: t) if sel is None else (lambda t: t[sel])
    want, bar = _act_want(act, pick(z0), pick(du0) if du0 is not None else None, mult, scale, ot, fwd)
    wide = zt != F32 and n % 8 == 0 and off % 8 == 0
    routed = plain and not wide
    kernel = ("amds_gelu_" + ("fwd" if fwd else "bwd")) if plain else f"amds_{act}_dropout_" + ("fwd" if fwd else "bwd")
    body = f"{act}_{'fwd' if fwd else 'bwd'}_kernel" if routed else f"{act}_dropout_{'fwd' if fwd else 'bwd'}{'8' if wide else ''}_kernel"
    variant = f"{body}<{', '.join(NAME[t] for t in ((zt, ot) if fwd else (zt, gt, ot)))}>"
    _judge(kernel, variant, family, f"n={n}" + (f" +{off} element" if off else "") + ("" if plain else f" p={p:g}") + ("" if sel is None else " (ends and past the cap)"),
           pick(got), want, bar)


@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("fwd", [True, False], ids=["fwd", "bwd"])
def test_act_dropout(gpu, act, fwd):
    for types in (FWD_PAIRS if fwd else BWD_TRIPLES):
        for n, off in ACT_SIZES:
            for p in O.DROP_RATES:
                for family in (FAMILIES if act == "relu" else ("real",)):
                    _act_case(gpu, act, fwd, types, n, off, p, family)


@pytest.mark.parametrize("fwd", [True, False], ids=["fwd", "bwd"])
def test_gelu_without_dropout(gpu, fwd):
    """amds_gelu_fwd / _bwd: the 16-bit routes go to dropout.hip at p = 0 (n 8, 65 544), the rest to train.hip's scalar kernels -- every value compared."""
    for types in (FWD_PAIRS if fwd else BWD_TRIPLES):
        for n, off in ACT_SIZES:
            _act_case(gpu, "gelu", fwd, types, n, off, 0.0, "real", plain=True)


def test_refused_dtype_pairs_touch_nothing(gpu):
    lib, n = _lib.lib(), 64
    for fwd, combos in ((True, FWD_REFUSED), (False, BWD_REFUSED)):
        for types in combos:
            zt, gt, ot = (types[0], None, types[1]) if fwd else types
            for act, plain in (("gelu", False), ("relu", False), ("gelu", True)):
                z, out = Buf(gpu, n, zt, data=torch.ones(n), name="z"), Buf(gpu, n, ot, name="out")
                du = Buf(gpu, n, gt, data=torch.ones(n), name="du") if not fwd else None
                assert _act_call(lib, act, fwd, z, du, out, n, zt, gt, ot, 0.25, plain) == ERR_INVALID, (act, plain, types)
                assert bool((_bits(out.cpu()) == -1).all()), (act, plain, types)


# ==== dropout_add / dropout_cast_bwd ==================================================================================================================================
def _site_inputs(rows, cols, family):
    g = O._gen(10, rows, cols)
    if family == "grid":
        return O.ints(g, (rows, cols)), O.ints(g, (rows, cols))
    return torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)


def _site_want(kind, y0, x0, mult, scale, odt, family):
    """dropout_add: x + mult y (two roundings: EPS of each term's share); cast_bwd: mult y rounded to odt (one rounding unless the scale is a power of two)."""
    prod = y0.double() * mult
    if kind == "add":
        want = x0.double() + prod
        return want, None if family == "grid" and O.scale_is_pow2_value(scale) else O.EPS * (prod.abs() + want.abs())
    if family == "grid" and O.scale_is_pow2_value(scale):
        return O.saturate(prod, odt), None          # |y| <= 8 times 1, 2 or 65536: a 16-bit value, or past fp16's range altogether
    return O.saturate(prod, odt), (0.0 if O.scale_is_pow2_value(scale) else O.U) * prod.abs() + O.half_ulp(prod, odt)


def _site_case(gpu, kind, rows, cols, ld, off, odt, p, family, row_mul=None, sel=None):
    lib = _lib.lib()
    y0, x0 = _site_inputs(rows, cols, family)
    ldo = ld          # (the output shares the pitch: 272 is a multiple of 8, 262 defeats the 8-wide forms)

    def run():
        y, x = Buf(gpu, (rows, cols), F32, ld, off, y0, "y"), Buf(gpu, (rows, cols), F32, ld, off, x0, "x_in")
        out = Buf(gpu, (rows, cols), F32 if kind == "add" else odt, ldo, off, name="out")
        if kind == "add" and row_mul is None:
            rc = lib.amds_dropout_add(y.ptr(), ld, x.ptr(), ld, out.ptr(), ldo, rows, cols, p, SEED, SID, _st())
        elif kind == "add":
            rc = lib.amds_dropout_add_rows(y.ptr(), ld, x.ptr(), ld, out.ptr(), ldo, rows, cols, row_mul, p, SEED, SID, _st())
        elif row_mul is None:
            rc = lib.amds_dropout_cast_bwd(y.ptr(), ld, out.ptr(), ldo, rows, cols, DT[odt], p, SEED, SID, _st())
        else:
            rc = lib.amds_dropout_cast_bwd_rows(y.ptr(), ld, out.ptr(), ldo, rows, cols, row_mul, p, SEED, SID, _st())
        _lib.check(rc, kind)
        return dict(out=out.cpu())

    got = _twice(run)["out"].reshape(-1)
    flat = np.arange(rows * cols, dtype=np.int64) if sel is None else sel.numpy()
    r, c = flat // cols, flat % cols
    idx = flat if row_mul is None else r * row_mul * cols + c
    thr = O.drop_thr16(p)
    scale = O.drop_scale(thr)
    mult = torch.from_numpy(O.keep_flat(SEED, SID, idx, thr).astype(np.float64)) * scale
    pick = (lambda t: t.reshape(-1)) if sel is None else (lambda t: t.reshape(-1)[sel])
    want, bar = _site_want(kind, pick(y0), pick(x0), mult, scale, odt, family)
    wide = cols % 8 == 0 and ld % 4 == 0 and off % 4 == 0 and (kind == "add" or (odt != F32 and ldo % 8 == 0 and off % 8 == 0))
    if row_mul is not None:
        kernel, variant = f"amds_dropout_{'add' if kind == 'add' else 'cast_bwd'}_rows", "dropout_add_rows_kernel" if kind == "add" else "dropout_cast_bwd_rows_kernel<bf16>"
    elif kind == "add":
        kernel, variant = "amds_dropout_add", "dropout_add8_kernel" if wide else "dropout_add_kernel"
    else:
        kernel, variant = "amds_dropout_cast_bwd", f"dropout_cast_bwd{'8' if wide else ''}_kernel<{NAME[odt]}>"
    case = f"{rows} x {cols} ld={ld}" + (f" +{off} element" if off else "") + f" p={p:g}" + (f" row_mul={row_mul}" if row_mul else "") + ("" if sel is None else " (ends and past the cap)")
    _judge(kernel, variant, family, case, pick(got), want, bar)


SITE_LAYOUTS = ((264, 272, 0), (260, 272, 0), (256, 262, 0), (264, 272, 1))          # (cols, pitch, elements off): 8-wide | cols % 8 | a pitch of 262 floats | a pointer 4 bytes off


@pytest.mark.parametrize("kind,odt", [("add", F32), ("cast", BF16), ("cast", F16), ("cast", F32)])
def test_dropout_sites(gpu, kind, odt):
    for cols, ld, off in SITE_LAYOUTS:
        for p in O.DROP_RATES:
            for family in FAMILIES:
                _site_case(gpu, kind, 37, cols, ld, off, odt, p, family)


# ==== the four *_rows forms: logical row r * row_mul, so the flat index passes 2^32 and 2^48 and the high word of the row key is no longer zero ================================
@pytest.mark.parametrize("row_mul", [1, 9, 1 << 23, 1 << 40])
def test_rows_forms(gpu, row_mul):
    rows, cols, ld = 3, 520, 528
    assert row_mul < (1 << 40) or ((rows - 1) * row_mul * cols) >> 16 >= (1 << 32)          # the mask row (flat index >> 16) of the last rows needs more than 32 bits
    for p in (0.0, 0.25, 0.5):
        for family in FAMILIES:
            _site_case(gpu, "add", rows, cols, ld, 0, F32, p, family, row_mul=row_mul)
            _site_case(gpu, "cast", rows, cols, ld, 0, BF16, p, family, row_mul=row_mul)
        _gelu_rows_case(gpu, rows, cols, ld, row_mul, p)


def _gelu_rows_case(gpu, rows, cols, ld, row_mul, p, sel=None):
    lib = _lib.lib()
    z0, du0 = O.gelu_inputs(rows * cols, BF16)
    z0, du0 = z0.view(rows, cols), du0.view(rows, cols)

    def run():
        z, du = Buf(gpu, (rows, cols), BF16, ld, data=z0, name="z"), Buf(gpu, (rows, cols), BF16, ld + 8, data=du0, name="du")
        u, dz = Buf(gpu, (rows, cols), BF16, ld + 16, name="u"), Buf(gpu, (rows, cols), BF16, ld + 24, name="dz")
        _lib.check(lib.amds_gelu_dropout_fwd_rows(z.ptr(), ld, u.ptr(), ld + 16, rows, cols, row_mul, p, SEED, SID, _st()), "gelu_dropout_fwd_rows")
        _lib.check(lib.amds_gelu_dropout_bwd_rows(z.ptr(), ld, du.ptr(), ld + 8, dz.ptr(), ld + 24, rows, cols, row_mul, p, SEED, SID, _st()), "gelu_dropout_bwd_rows")
        return dict(u=u.cpu(), dz=dz.cpu())

    o = _twice(run)
    flat = np.arange(rows * cols, dtype=np.int64) if sel is None else sel.numpy()
    idx = (flat // cols) * row_mul * cols + flat % cols
    thr = O.drop_thr16(p)
    scale = O.drop_scale(thr)
    mult = torch.from_numpy(O.keep_flat(SEED, SID, idx, thr).astype(np.float64)) * scale
    pick = (lambda t: t.reshape(-1)) if sel is None else (lambda t: t.reshape(-1)[sel])
    case = f"{rows} x {cols} row_mul={row_mul} p={p:g}" + ("" if sel is None else " (ends and past the cap)")
    want, bar = _act_want("gelu", pick(z0), None, mult, scale, BF16, True)
    _judge("amds_gelu_dropout_fwd_rows", "gelu_dropout_fwd_rows_kernel<bf16>", "real", case, pick(o["u"]), want, bar)
    want, bar = _act_want("gelu", pick(z0), pick(du0), mult, scale, BF16, False)
    _judge("amds_gelu_dropout_bwd_rows", "gelu_dropout_bwd_rows_kernel<bf16>", "real", case, pick(o["dz"]), want, bar)


# ==== dropout on fp32 attention probabilities ========================================================================================================================
def _attn_rows_case(gpu, rows, cols, p, family, in_place, sel=None):
    lib = _lib.lib()
    g = O._gen(11, rows, cols)
    x0 = O.ints(g, (rows, cols), 0, 8) if family == "grid" else torch.rand(rows, cols, generator=g)

    def run():
        x = Buf(gpu, (rows, cols), F32, data=x0, name="x")
        y = x if in_place else Buf(gpu, (rows, cols), F32, name="y")
        _lib.check(lib.amds_attention_dropout_rows(x.ptr(), y.ptr(), rows, cols, p, SEED, SID, _st()), "attention_dropout_rows")
        return dict(y=y.cpu())

    got = _twice(run)["y"].reshape(-1)
    flat = np.arange(rows * cols, dtype=np.int64) if sel is None else sel.numpy()
    thr = O.drop_thr16(p)
    scale = O.drop_scale(thr)
    mult = torch.from_numpy(O.keep_rows(SEED, SID, flat // cols, flat % cols, thr).astype(np.float64)) * scale
    pick = (lambda t: t.reshape(-1)) if sel is None else (lambda t: t.reshape(-1)[sel])
    want = pick(x0).double() * mult
    _judge("amds_attention_dropout_rows", "attn_dropout_rows_kernel" + (" in place" if in_place else ""), family,
           f"{rows} x {cols} p={p:g}" + ("" if sel is None else " (ends and past the cap)"), pick(got), want, None if O.scale_is_pow2_value(scale) else O.U * want.abs())


@pytest.mark.parametrize("cols", [1, 2, 3, 257])
def test_attention_dropout_rows(gpu, cols):
    for p in O.DROP_RATES:
        for family in FAMILIES:
            for in_place in (False, True):
                _attn_rows_case(gpu, 5, cols, p, family, in_place)


# ==== AdamW ========================================================================================================================================================
def _adam_run(gpu, n, hyper, step, p0, g0, m0, v0, state=None):
    lib = _lib.lib()

    def run():
        p, g, m, v = (Buf(gpu, n, F32, data=t, name=k) for k, t in (("p", p0), ("g", g0), ("m", m0), ("v", v0)))
        args = (p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"], hyper["wd"], step)
        if state is None:
            _lib.check(lib.amds_adamw(*args, _st()), "adamw")
        else:
            _lib.check(lib.amds_adamw_guarded(*args, state.data_ptr(), _st()), "adamw_guarded")
        assert torch.equal(_bits(g.cpu()), _bits(g0))
        return dict(p=p.cpu(), m=m.cpu(), v=v.cpu())

    return _twice(run)


def _adam_judge(kernel, case, o, r, sel=None):
    pick = (lambda t: t) if sel is None else (lambda t: t[sel])
    for k in ("p", "m", "v"):
        _judge(kernel, kernel[5:] + "_kernel", "real", f"{case} {k}", pick(o[k]), pick(r[k]), pick(r["d_" + k]))


@pytest.mark.parametrize("name,hyper,step,fresh", O.ADAM_CASES)
def test_adamw(gpu, name, hyper, step, fresh):
    n = 1000
    p0, g0, m0, v0 = O.adam_inputs(n, fresh)
    o = _adam_run(gpu, n, hyper, step, p0, g0, m0, v0)
    _adam_judge("amds_adamw", name, o, O.adamw(p0, g0, m0, v0, t=step, **hyper))
    st = T.loss_scale_state(gpu, 1024.0)
    og = _adam_run(gpu, n, hyper, step, p0, g0, m0, v0, state=st)
    for k in o:
        assert torch.equal(_bits(o[k]), _bits(og[k])), f"amds_adamw_guarded on a clean state is not amds_adamw's bits ({name}, {k})"


def test_adamw_guarded_after_skips(gpu):
    """Two skipped steps, then step 5: the bias corrections are those of t = 3 applied steps."""
    n, step = 1000, 5
    st = T.loss_scale_state(gpu, 1024.0, growth_interval=1000)
    for _ in range(2):
        T.grad_unscale_check(torch.tensor([1.0, float("inf"), 2.0], device=gpu), st)
        T.loss_scale_update(st, apply=True)
    assert st.cpu().tolist()[T.LS_SKIPPED] == 2 and st.cpu().tolist()[T.LS_NONFINITE] == 0
    p0, g0, m0, v0 = O.adam_inputs(n, False)
    o = _adam_run(gpu, n, O.ADAM_HYPER, step, p0, g0, m0, v0, state=st)
    _adam_judge("amds_adamw_guarded", "step 5, 2 skipped", o, O.adamw(p0, g0, m0, v0, t=step - 2, **O.ADAM_HYPER))
    wrong = O.adamw(p0, g0, m0, v0, t=step, **O.ADAM_HYPER)
    assert bool(((o["p"].double() - wrong["p"]).abs() > wrong["d_p"]).any())          # the bar tells t = 3 from t = 5


# ==== second trips of the grid-stride loops ===========================================================================================================================
def _sel(n, cap):
    """The first 4096 elements, the last 4096, and every element from the cap (the grid's thread count times the elements per thread) onwards."""
    return torch.unique(torch.cat([torch.arange(min(4096, n)), torch.arange(cap, n), torch.arange(max(n - 4096, 0), n)]))


CAP_TRAIN, CAP_DROP = 4096 * 256, 8192 * 256


@pytest.mark.parametrize("which", ["gelu_fwd f32", "gelu_bwd bf16", "adamw", "adamw_guarded", "rows forms"])
def test_second_trip_train_hip_and_rows(gpu, which):
    """grid1d caps at 4096 blocks of 256 threads, the *_rows forms likewise: n = 2^20 + 257 sends 257 threads round again."""
    n = CAP_TRAIN + 257
    sel = _sel(n, CAP_TRAIN)
    if which == "gelu_fwd f32":
        z0, _ = O.gelu_inputs(n, F32)
        _act_case(gpu, "gelu", True, (F32, F32), n, 0, 0.0, "real", plain=True, sel=sel, z0=z0)
    elif which == "gelu_bwd bf16":          # n is odd: the 16-bit route stays on train.hip's scalar kernel
        z0, du0 = O.gelu_inputs(n, BF16)
        _act_case(gpu, "gelu", False, (BF16, BF16, BF16), n, 0, 0.0, "real", plain=True, sel=sel, z0=z0, du0=du0)
    elif which in ("adamw", "adamw_guarded"):
        p0, g0, m0, v0 = O.adam_inputs(n, False)
        st = T.loss_scale_state(gpu, 1024.0) if which == "adamw_guarded" else None
        o = _adam_run(gpu, n, O.ADAM_HYPER, 7, p0, g0, m0, v0, state=st)
        r = O.adamw(p0[sel], g0[sel], m0[sel], v0[sel], t=7, **O.ADAM_HYPER)
        _adam_judge("amds_" + which, f"n={n} (ends and past the cap)", {k: t[sel] for k, t in o.items()}, r)
    else:
        rows, cols = 2017, 520
        assert rows * cols >= n
        sel = _sel(rows * cols, CAP_TRAIN)
        _site_case(gpu, "add", rows, cols, 528, 0, F32, 0.25, "real", row_mul=1, sel=sel)
        _site_case(gpu, "cast", rows, cols, 528, 0, BF16, 0.25, "real", row_mul=1, sel=sel)
        _gelu_rows_case(gpu, rows, cols, 528, 1, 0.25, sel=sel)


@pytest.mark.parametrize("which", ["gelu fwd", "gelu bwd", "relu fwd", "relu bwd", "dropout_add", "dropout_cast_bwd", "attention_dropout_rows"])
def test_second_trip_dropout_hip_scalar(gpu, which):
    """grid1d_ caps at 8192 blocks: the one-element-per-thread kernels take a second trip from n = 2^21 on."""
    n = CAP_DROP + 257
    if which in ("gelu fwd", "gelu bwd", "relu fwd", "relu bwd"):
        act, fwd = which.split()[0], which.endswith("fwd")
        z0, du0 = O.gelu_inputs(n, F32)
        _act_case(gpu, act, fwd, (F32, F32) if fwd else (F32, F32, F32), n, 0, 0.25, "real", sel=_sel(n, CAP_DROP), z0=z0, du0=None if fwd else du0)
    elif which == "dropout_add":
        _site_case(gpu, "add", 8068, 260, 260, 0, F32, 0.25, "real", sel=_sel(8068 * 260, CAP_DROP))
    elif which == "dropout_cast_bwd":
        _site_case(gpu, "cast", 7946, 264, 264, 0, F32, 0.25, "real", sel=_sel(7946 * 264, CAP_DROP))
    else:
        _attn_rows_case(gpu, 8161, 257, 0.25, "real", False, sel=_sel(8161 * 257, CAP_DROP))
        thr, rows, cols = O.drop_thr16(0.25), 8161, 257

        def run():
            m = Buf(gpu, (rows, cols), torch.uint8, name="mask rows")
            _lib.check(_lib.lib().amds_attention_dropout_mask_rows(m.ptr(), rows, cols, 0.25, SEED, SID, _st()), "attention_dropout_mask_rows")
            return dict(m=m.cpu())
        want = O.keep_rows(SEED, SID, np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :], thr).astype(np.uint8)
        _judge("amds_attention_dropout_mask_rows", "attn_dropout_mask_rows_kernel", "rule", f"{rows} x {cols} p=0.25 (second trip)", _twice(run)["m"], torch.from_numpy(want))


@pytest.mark.parametrize("which", ["gelu fwd", "gelu bwd", "relu fwd", "relu bwd", "dropout_add", "dropout_cast_bwd"])
def test_second_trip_dropout_hip_8_wide(gpu, which):
    """The 8-wide kernels take theirs from 8 * 2^21 elements on."""
    n, cap = 8 * (CAP_DROP + 3), 8 * CAP_DROP
    if which in ("gelu fwd", "gelu bwd", "relu fwd", "relu bwd"):
        act, fwd = which.split()[0], which.endswith("fwd")
        zt = BF16 if which in ("gelu fwd", "relu bwd") else F16
        z0, du0 = O.gelu_inputs(n, zt)
        types = (zt, F32 if act == "relu" else zt) if fwd else (zt, F32 if act == "gelu" else zt, zt)
        _act_case(gpu, act, fwd, types, n, 0, 0.25, "real", sel=_sel(n, cap), z0=z0, du0=None if fwd else du0.float().to(types[1]))
    else:
        rows, cols = 63551, 264
        assert rows * cols >= n
        _site_case(gpu, "add" if which == "dropout_add" else "cast", rows, cols, cols, 0, F32 if which == "dropout_add" else BF16, 0.25, "real", sel=_sel(rows * cols, cap))
