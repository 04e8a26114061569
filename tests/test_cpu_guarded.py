"""tests/guarded.py bites: five faulty "kernels" written in plain torch on CPU tensors are each flagged, a correct one passes.
The fakes compute a row-scaled copy, out[r, c] = 2 * x[r, c] + bias[c], the way a strided row kernel of the library would: they get
raw 2-D storage (rows at a pitch) and the logical sizes, so they CAN step outside -- which is what the helper has to notice."""
import pytest
import torch

import guarded as G

ROWS, COLS, LD = 37, 24, 32
DT = torch.float32


def _raw(h: G.Guarded) -> torch.Tensor:
    """The whole allocation as bytes, indexed from its first byte (the interior starts at `h.start`): everything a stray pointer of a kernel can reach."""
    return h.buf.view(torch.uint8)


def _elem(h: G.Guarded, r: int, c: int) -> slice:
    """Byte range of element (r, c) addressed by pitch alone, with no bounds test."""
    at = h.start + (r * h.ld + c) * h.item
    return slice(at, at + h.item)


def _store(h: G.Guarded, r: int, c: int, value: float) -> None:
    _raw(h)[_elem(h, r, c)] = torch.tensor([value], dtype=h.dtype).view(torch.uint8)


def _load_row(h: G.Guarded, r: int, ncols: int) -> torch.Tensor:
    at = h.start + r * h.ld * h.item
    return _raw(h)[at:at + ncols * h.item].view(h.dtype)


def _case(kernel, with_ws=False):
    """-> call(pattern) for run_contract: x pitched with poisoned padding, out pitched and poisoned everywhere, optionally a poisoned workspace."""
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(ROWS, COLS, generator=g)
    bias = torch.randn(COLS, generator=g)

    def call(pattern):
        x, hx = G.guarded_like(x0, ld=LD, pattern=pattern, name="x")
        out, ho = G.guarded((ROWS, COLS), DT, "cpu", ld=LD, pattern=pattern, name="out")
        hs = [hx, ho]
        ws = None
        if with_ws:
            ws, hw = G.guarded((COLS,), DT, "cpu", pattern=pattern, name="ws")
            hs.append(hw)
        kernel(hx, ho, bias, ws)
        return G.Result({"out": out}, hs)

    return call, 2 * x0 + bias


def _correct(hx, ho, bias, ws):
    for r in range(ROWS):
        ho.view[r] = 2 * _load_row(hx, r, COLS) + bias


def _writes_one_element_past_the_last_row(hx, ho, bias, ws):
    _correct(hx, ho, bias, ws)
    _store(ho, ROWS, 0, 1.0)                              # row index == rows: the first element behind the buffer


def _writes_a_padding_column(hx, ho, bias, ws):
    _correct(hx, ho, bias, ws)
    _store(ho, 5, COLS, 1.0)                              # column index == cols < pitch


def _writes_one_byte_before_the_buffer(hx, ho, bias, ws):
    _correct(hx, ho, bias, ws)
    _raw(ho)[ho.start - 1] = 0x5A


def _reads_a_padding_column(hx, ho, bias, ws):
    for r in range(ROWS):                                   # a vector load one element too wide, folded into the last column
        row = _load_row(hx, r, COLS + 1)
        ho.view[r] = 2 * row[:COLS] + bias
        ho.view[r, COLS - 1] += 0.0 * row[COLS]           # times a "masked" weight of 0: fine with finite leftovers, NaN with 0xFF


def _accumulates_into_unzeroed_workspace(hx, ho, bias, ws):
    for r in range(ROWS):
        ws += _load_row(hx, r, COLS)                        # column sums, on top of whatever the workspace held
    for r in range(ROWS):
        ho.view[r] = 2 * _load_row(hx, r, COLS) + bias + 0.0 * ws


def test_correct_fake_passes():
    call, ref = _case(_correct)
    out = G.run_contract(call)
    assert torch.equal(out["out"], ref)
    call, ref = _case(lambda hx, ho, bias, ws: (ws.zero_(), _accumulates_into_unzeroed_workspace(hx, ho, bias, ws)), with_ws=True)
    assert torch.equal(G.run_contract(call)["out"], ref)       # the same accumulation is fine once the call zeroes what it needs zeroed


@pytest.mark.parametrize("kernel,what,with_ws", [
    (_writes_one_element_past_the_last_row, r"out: bytes written PAST the buffer's end .*first at \+\d B = row 37,", False),
    (_writes_a_padding_column, r"out: pitch padding written, first at row 5, column 24", False),
    (_writes_one_byte_before_the_buffer, r"out: bytes written BEFORE the buffer .*from 1 B to 1 B", False),
    (_reads_a_padding_column, r"output out \(poison 0xFF\): 37 non-finite", False),
    (_accumulates_into_unzeroed_workspace, r"output out \(poison 0xFF\): \d+ non-finite", True),
], ids=["past_last_row", "padding_column", "byte_before", "reads_padding", "stale_workspace"])
def test_faulty_fake_is_flagged(kernel, what, with_ws):
    call, _ = _case(kernel, with_ws)
    with pytest.raises(G.GuardViolation, match=what):
        G.run_contract(call)


def test_stale_integer_workspace_shows_as_a_bit_difference():
    """An arrival counter that is never reset: nothing turns non-finite (0xFF bytes are -1 in an int32), the two runs just disagree."""
    def call(pattern):
        cnt, hc = G.guarded((4,), torch.int32, "cpu", pattern=pattern, name="counters")
        out, ho = G.guarded((4,), DT, "cpu", pattern=pattern, name="out")
        cnt += 3                                            # three arrivals, no reset
        out.copy_(cnt.float())
        return G.Result({"out": out}, [hc, ho])

    with pytest.raises(G.GuardViolation, match="differ between poison 0x00 and 0xFF"):
        G.run_contract(call)


def test_layout_alignment_and_band_sizes():
    v, h = G.guarded((3, 5, 7), torch.float16, "cpu", ld=12, pattern=0xFF)
    assert v.shape == (3, 5, 7) and v.stride() == (60, 12, 1) and v.data_ptr() % 256 == 0
    assert h.band >= 1 << 20 and h.start >= h.band and h.buf.numel() - (h.start + h.body) >= h.band
    assert torch.isnan(v).all()                             # 0xFF bytes are NaN in fp16 ...
    for dt in (torch.float32, torch.bfloat16):
        assert torch.isnan(G.guarded((2, 3), dt, "cpu")[0]).all()
    assert (G.guarded((2, 3), torch.int32, "cpu")[0] == -1).all() and (G.guarded((2, 3), torch.uint8, "cpu")[0] == 255).all()
    _, wide = G.guarded((2, 4), torch.float32, "cpu", ld=3000)
    assert wide.band >= 256 * 3000 * 4                      # ... and a band holds 256 rows of a wide pitch
    assert G.guarded((50 << 20,), torch.uint8, "cpu", band_bytes=G.FLAT_BAND_BYTES)[1].band == G.FLAT_BAND_BYTES      # a flat workspace has no pitch to scale with
    v.zero_()
    h.assert_bands_intact()                                 # writing every interior element touches no guard byte
    h2 = G.guarded_like(torch.ones(4, 6), ld=8, pattern=0xFF)[1]
    h2.assert_bands_intact()
    h2.buf[h2.start + 6 * 4] = 1
    with pytest.raises(G.GuardViolation, match="pitch padding written, first at row 0, column 6"):
        h2.assert_bands_intact()


def test_scratch_hook_returns_exact_poisoned_bytes_and_restores(monkeypatch):
    from stamp_amd import ops
    real = ops.scratch
    dev = torch.device("cpu")
    with G.scratch_hook(monkeypatch, 0xFF) as log:
        a = ops.scratch("tag_a", dev, 1000)
        assert a.numel() == 1000 and a.dtype == torch.uint8 and a.data_ptr() % 256 == 0 and (a == 0xFF).all()
        b = ops.scratch("tag_a", dev, 10)
        assert b.data_ptr() != a.data_ptr() and log.requests == [("tag_a", 1000), ("tag_a", 10)]
        a.zero_()
        log.assert_bands_intact()
        log.handles[0].buf[log.handles[0].start + 1000] = 0          # the byte behind the requested size
        with pytest.raises(G.GuardViolation, match=r"scratch\[tag_a\]: bytes written PAST"):
            log.assert_bands_intact()
    assert ops.scratch is real
    with G.scratch_hook(monkeypatch, 0x00, persistent=True) as log:
        big = ops.scratch("t", dev, 4096)
        big.fill_(7)
        small = ops.scratch("t", dev, 100)                  # the big call's leftovers, not poisoned again
        assert small.numel() == 100 and small.data_ptr() == big.data_ptr() and (small == 7).all() and len(log.handles) == 1
    assert ops.scratch is real
