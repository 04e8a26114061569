"""Guard bands, poison patterns and a scratch hook for the C-ABI contract tests (test_cpu_guarded.py, test_gpu_abi_*.py).

The parity tests check the values INSIDE the tensors a caller asked for.  This helper checks the rest of the contract:

* `guarded(...)` -- one uint8 allocation laid out as  front band | rows at pitch ld >= cols | back band.  The bands and the pitch
  padding carry a poison byte; `handle.assert_bands_intact()` compares them byte for byte after a call.  Each band holds at least
  1 MiB and at least 256 rows of the buffer's pitch, so a kernel that overruns by a whole 256-row tile still lands inside the
  allocation and is reported.  The interior starts on a 256-byte boundary (what include/amdstamp.h asks of `ws`).
* two poison bytes: 0x00, and 0xFF -- a NaN in fp32 / fp16 / bf16 / e4m3, -1 in a signed counter, 255 in u8.  Inputs carry the
  poison in their bands and padding; workspaces, saved arenas, gradient buffers and pure outputs carry it everywhere.
* `run_contract(call)` -- runs `call(pattern)` under both bytes and asserts: every declared output bit-identical between the two
  runs, every floating output finite, every band and padding byte unchanged.  A kernel that reads a byte it was not given, or one
  of its workspace that it never wrote, cannot satisfy the first two; one that writes outside what it owns cannot satisfy the third.
* `scratch_hook(monkeypatch, pattern)` -- replaces `stamp_amd.ops.scratch` so the whole-model wrappers run on a guarded, poisoned
  workspace of exactly the requested size, and `stamp_amd.ops.alloc` (saved arenas, gradient buffers) likewise; `persistent=True` keeps one grow-only buffer per tag WITHOUT poisoning it again (the
  "big shape, then small shape" order of a long-lived process).
"""
from __future__ import annotations

import contextlib
import math
from dataclasses import dataclass, field

import torch

PATTERNS = (0x00, 0xFF)
MIN_BAND_BYTES = 1 << 20
MIN_BAND_ROWS = 256
FLAT_BAND_BYTES = 8 << 20          # bands of the flat workspaces / arenas: 256 rows of 8192 fp32 columns
ALIGN = 256


class GuardViolation(AssertionError):
    """A byte outside the tensor a call owns changed, or a declared output depends on a poisoned byte."""


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


class Guarded:
    """Handle of one guarded allocation (see `guarded`)."""

    def __init__(self, shape, dtype, device, ld, band_bytes, pattern, name):
        shape = tuple(int(s) for s in shape)
        assert len(shape) >= 1 and all(s >= 0 for s in shape)
        self.shape, self.dtype, self.pattern, self.name = shape, dtype, int(pattern), name
        self.item = torch.empty((), dtype=dtype).element_size()
        self.cols = shape[-1]
        self.rows = math.prod(shape[:-1])
        self.ld = self.cols if ld is None else int(ld)
        assert self.ld >= self.cols, f"pitch {self.ld} < {self.cols} columns"
        pitch = self.ld * self.item
        # (a flat buffer -- a workspace, an arena -- has no row pitch of its own: its bands are `band_bytes`, which the caller sizes to 256 rows of the widest
        # tensor the call keeps there)
        self.band = _round_up(max(int(band_bytes), MIN_BAND_BYTES, MIN_BAND_ROWS * pitch if len(shape) > 1 else 0), ALIGN)
        assert self.band < 1 << 31
        self.body = self.rows * pitch
        self.buf = torch.empty(self.band + ALIGN + self.body + self.band, dtype=torch.uint8, device=device)
        self.start = self.band + (-(self.buf.data_ptr() + self.band)) % ALIGN          # the interior starts 256-byte aligned
        self.buf.fill_(self.pattern)
        flat = self.buf[self.start:self.start + self.body].view(dtype)
        rows2d = flat.view(self.rows, self.ld) if self.rows else flat.view(0, self.ld)
        self.view2d = rows2d[:, :self.cols]
        strides, step = [1] * len(shape), self.ld          # leading dimensions walk whole rows of the pitch
        for i in range(len(shape) - 2, -1, -1):
            strides[i] = step
            step *= shape[i]
        self.view = torch.as_strided(flat, shape, tuple(strides))
        assert self.view.data_ptr() % ALIGN == 0

    # ---- filling ------------------------------------------------------------------------------------------------------------------
    def load(self, t: torch.Tensor) -> torch.Tensor:
        """Copy `t` into the interior (bands and pitch padding keep the poison) -> the strided view."""
        self.view.copy_(t.to(self.view.device, self.dtype).reshape(self.shape))
        return self.view

    # ---- checking -----------------------------------------------------------------------------------------------------------------
    def _padding(self) -> torch.Tensor:
        pitch = self.ld * self.item
        return self.buf[self.start:self.start + self.body].view(self.rows, pitch)[:, self.cols * self.item:]

    @staticmethod
    def _bad_span(region: torch.Tensor, want):
        """(first, last) flat index of the bytes of `region` that differ from `want`, or None."""
        idx = (region != want).reshape(-1).nonzero()
        return None if idx.numel() == 0 else (int(idx[0]), int(idx[-1]))

    def assert_bands_intact(self) -> None:
        end = self.start + self.body
        pitch = max(self.ld * self.item, 1)
        span = self._bad_span(self.buf[:self.start], self.pattern)
        if span is not None:
            raise GuardViolation(f"{self.name}: bytes written BEFORE the buffer (front band): from {self.start - span[0]} B to {self.start - span[1]} B in front of it")
        span = self._bad_span(self.buf[end:], self.pattern)
        if span is not None:
            at = span[0]
            raise GuardViolation(f"{self.name}: bytes written PAST the buffer's end (back band): first at +{at} B = row {self.rows + at // pitch}, "
                                 f"byte {at % pitch} of its pitch; last at +{span[1]} B")
        if self.ld > self.cols and self.rows:
            pad = self._padding()
            span = self._bad_span(pad, self.pattern)
            if span is not None:
                w = pad.shape[1]
                raise GuardViolation(f"{self.name}: pitch padding written, first at row {span[0] // w}, column {self.cols + (span[0] % w) // self.item} "
                                     f"(cols {self.cols}, pitch {self.ld})")


def guarded(shape, dtype, device, ld=None, band_bytes=MIN_BAND_BYTES, *, pattern=0xFF, name="buffer"):
    """-> (view, handle).  `view` has `shape`, rows (the last dimension) at pitch `ld` elements; every byte of the allocation, the
    interior included, holds `pattern` until the caller loads data (`handle.load`)."""
    h = Guarded(shape if not isinstance(shape, int) else (shape,), dtype, device, ld, band_bytes, pattern, name)
    return h.view, h


def guarded_like(t: torch.Tensor, *, ld=None, pattern=0xFF, name="input", device=None):
    """A guarded copy of `t`: data inside, poison in bands and pitch padding -> (view, handle)."""
    v, h = guarded(tuple(t.shape), t.dtype, device if device is not None else t.device, ld=ld, pattern=pattern, name=name)
    h.load(t)
    return v, h


# ---- the two-pattern contract ------------------------------------------------------------------------------------------------------
@dataclass
class Result:
    outputs: dict                                   # name -> tensor the call declares as an output (cloned by run_contract)
    handles: list = field(default_factory=list)     # every Guarded the call touched, inputs included


def _finite(name: str, t: torch.Tensor) -> None:
    if t.is_floating_point() and not bool(torch.isfinite(t).all()):
        n = int((~torch.isfinite(t)).sum())
        raise GuardViolation(f"output {name}: {n} non-finite value(s): the call read a poisoned byte (padding, band, or workspace it never wrote)")


def run_contract(call, patterns=PATTERNS) -> dict:
    """`call(pattern) -> Result` once per poison byte.  Asserts bands / padding intact, floating outputs finite, and every output
    bit-identical between the runs; -> the outputs of the FIRST pattern's run (0x00), for the caller's reference bar."""
    runs = []
    for p in patterns:
        r = call(p)
        if r.handles and r.handles[0].buf.is_cuda:
            torch.cuda.synchronize()
        for h in r.handles:
            h.assert_bands_intact()
        outs = {k: v.detach().clone() for k, v in r.outputs.items()}
        for k, v in outs.items():
            _finite(f"{k} (poison 0x{p:02X})", v)
        runs.append(outs)
    first = runs[0]
    for p, other in zip(patterns[1:], runs[1:]):
        assert other.keys() == first.keys()
        for k in first:
            if not torch.equal(first[k], other[k]):
                d = (first[k] != other[k])
                raise GuardViolation(f"output {k}: {int(d.sum())} element(s) differ between poison 0x{patterns[0]:02X} and 0x{p:02X}: "
                                     f"the result depends on bytes the call was not given")
    return first


# ---- the operands of one leaf-kernel call ----------------------------------------------------------------------------------------------------------
def act_eps(dt):
    """One unit in the last place at 1.0 of a 16-bit activation dtype."""
    return 2 ** -10 if dt == torch.float16 else 2 ** -7


class Bufs:
    """The guarded operands of one call under one poison byte."""

    def __init__(self, gpu, pattern):
        self.gpu, self.pattern, self.handles = gpu, pattern, []

    def inp(self, t, ld=None, name="in"):
        v, h = guarded_like(t, ld=ld, pattern=self.pattern, name=name, device=self.gpu)
        self.handles.append(h)
        return v

    def out(self, shape, dtype, ld=None, name="out"):
        v, h = guarded(shape, dtype, self.gpu, ld=ld, pattern=self.pattern, name=name)
        self.handles.append(h)
        return v

    def result(self, **outs):
        return Result(outs, self.handles)


def cur_stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- the scratch hook --------------------------------------------------------------------------------------------------------------
class ScratchLog:
    def __init__(self):
        self.requests: list[tuple[str, int]] = []
        self.handles: list[Guarded] = []
        self._by_tag: dict = {}

    def assert_bands_intact(self) -> None:
        for h in self.handles:
            h.assert_bands_intact()

    def bytes_for(self, tag: str) -> list[int]:
        return [n for t, n in self.requests if t == tag]


@contextlib.contextmanager
def scratch_hook(monkeypatch, pattern: int, *, persistent: bool = False, short_by: int = 0):
    """Within the block `stamp_amd.ops.scratch(tag, dev, nbytes)` returns EXACTLY `nbytes` bytes of a guarded buffer poisoned with
    `pattern`, a fresh one per request; with `persistent` one grow-only buffer per tag that is poisoned when it is allocated and
    never again, its first `nbytes` bytes returned -- the state a long-lived process hands a small call after a big one.  `short_by`: the
    tensor handed out is that many bytes SHORTER than asked for while the guarded buffer behind it keeps the full size -- the wrappers pass
    `ws.numel()` as ws_bytes, so the library sees a workspace one byte too small, and a missing size check shows in the bands instead of overrunning."""
    from stamp_amd import ops

    log = ScratchLog()

    def fake(tag, dev, nbytes):
        nbytes = int(nbytes)
        log.requests.append((tag, nbytes))
        h = log._by_tag.get(tag) if persistent else None
        if h is None or h.cols < nbytes:
            _, h = guarded((max(nbytes, 1),), torch.uint8, dev, band_bytes=FLAT_BAND_BYTES, pattern=pattern, name=f"scratch[{tag}]")
            log.handles.append(h)
            log._by_tag[tag] = h
        return h.view[:max(nbytes - short_by, 0)]

    def fake_alloc(shape, dtype, dev):          # saved arenas, flat gradient buffers, d(bags): poisoned everywhere, a fresh one each time
        v, h = guarded(shape, dtype, dev, band_bytes=FLAT_BAND_BYTES, pattern=pattern, name=f"alloc[{len(log.handles)}]")
        log.requests.append(("alloc", h.body))
        log.handles.append(h)
        return v

    with monkeypatch.context() as m:
        m.setattr(ops, "scratch", fake)
        m.setattr(ops, "alloc", fake_alloc)
        m.setattr(ops, "_gap_workspace", lambda device, nbytes: fake("gap", device, nbytes))        # the pooling entries keep a workspace of their own
        yield log
