"""Every form of gated-attention pooling (stamp_amd/csrc/gap_fused.hip, gap.hip) against fp64 on planted scores, through the C ABI, element by element.

Reference, cases, bars and the reference-side mutants that prove the cases can fail: tests/gap_oracle.py (pinned on the CPU by test_cpu_gap_oracle.py).
Family I (integer grids: uniform, winner, two_winners, winner_per_unit): A_raw bit-equal to fp64, out bit-equal where the winner count is a power of two, else
within 2 u |out| (the six-launch form: its own counted roundings).  Family II (diffuse, gaussian, ascending, descending, plateau): per-element propagated bars.
Outputs and the workspace are guarded allocations (tests/guarded.py: poison 0xFF, bands checked after the calls).  Each check prints
`gap| form | geometry | family | A_raw err/bar | out err/bar` under -s and the module ends with the worst figure per form: profiles/gap_kernel_errors.txt is that
output from one run.

Forms ("route" of an item):
  pool      amds_gated_attn_pool, one call per bag, no offset table (gap.hip:180; L = 320 goes on to the six-launch form, :189)
  slab / split / auto      amds_gated_attn_pool_batched with that mode (gap_fused.hip:576; kernels chosen at :518, launched at :545-550)
  unfused   amds_gated_attn_pool_unfused, one call per bag (gap.hip:192)
  nopack    amds_gated_attn_pool_batched, auto, w->packed == NULL: gap_pack_kernel into the workspace (gap_fused.hip:536-541)
With "slab" / "split" every checked bag is pooled once more alone (one bag, no table) and must give the same bits -- all bags up to 32, else the first four,
every bag from 250 on (up to 300 bags) or a spread of them (65 537 bags); every form is called twice and must repeat its bits.

What reaches what (gap_fused.hip lines):
  gap_fused_kernel<16> / <32>, gap_split_kernel<16> / <32> (:545-550)      L = 256: l256, f32d64, f16d16, f1040, bags*, ragged300; L = 512: chief512, f48d48, f4096
  gf_locate, one round (:71-82)             every batched geometry up to 256 bags (bags255, bags256)
  gf_locate, second round                   bags257, ragged300 (300 bags, lengths 1 .. 90, 8192 < rows <= 12 288: auto = slab, split forced)
  gf_locate, third round                    bags65537 (65 537 one-row bags, F 32, L 256, D 16, slab): every bag checked
  F = 16: KG = 1, no next tile (:246-251)   f16d16, chunk2
  F/4 no multiple of 64, partial pass (:185-191)      f32d64 (8), f16d16 (4), f48d48 (12), f1040 (260)
  F > 1024: second trip of :140             f1040 (slab, units merged), f4096 (slab and split; the 70-row bag merges 2 / 5 units)
  D = 16 (NDB = 1, :279), D = 48            f16d16, chunk2, bags65537; f48d48 (L = 512: PP = 2, six pieces)
  rows per bag 1, 15, 16, 17, 63, 64, 65    chief512
  units per bag 1, 2, 3, 4, 5, 17, 69       chief512, of 64 rows (slab) and of 16 rows (split), each ROWS x units - 5 rows; 2 and 3 units leave waves an empty
                                            quarter (:184); 69 units = 18 per quarter: the DEPTH-16 body and the tail of gf_weighted_rows (:102-116)
  second merge chunk (:176)                 chunk2: one bag of 4097 x 64 - 5 rows, F 16, L 256, D 16, with and without the offset table
  both sides of every unit edge             sweep: single winners at row 0, N - 1 and 16 k - 1, 16 k of a 75- and a 139-row bag
  six-launch form (gap.hip:218-229)         chief512, f32d64, f16d16, f1040, and l320 (L = 320, F = 208, D = 72: only it takes that shape)
"""
import ctypes as C
import functools
import time

import pytest
import torch

import gap_oracle as O
import guarded as G
from stamp_amd import _lib, ops

pytestmark = pytest.mark.gpu
ITEMS = [(g, r) for g, v in O.GEOMS.items() for r in v[4]]
_WORST: dict = {}
_T0 = time.time()
SPLIT_AUTO_ROWS = 8192                             # gap_fused.hip:500


@functools.lru_cache(maxsize=None)
def _case(geom, family):
    x, lengths, w = O.build_case(geom, family, device=torch.device("cuda:0"))
    return x, lengths, w, O.reference(x, lengths, w)


def _split_ok(F, D):
    return F % 32 == 0 and D % 64 == 0


class _Call:
    """The guarded outputs and workspace of one route over one case; run() fills them through the C ABI."""

    def __init__(self, gpu, route, x, lengths, w, mode=None):
        self.gpu, self.route, self.x, self.lengths, self.w = gpu, route, x, lengths, w
        self.F, self.L, self.D = x.shape[1], w["fc_w"].shape[0], w["a_w"].shape[0]
        self.mode = mode or route

    def run(self):
        lib, x, F, L, D = _lib.lib(), self.x, self.F, self.L, self.D
        B, rows = len(self.lengths), x.shape[0]
        out, ho = G.guarded((B, F), torch.float32, self.gpu, pattern=0xFF, name="out")
        araw, ha = G.guarded((rows,), torch.float32, self.gpu, pattern=0xFF, name="attn_raw")
        st = ops._stream()
        if self.route in ("slab", "split", "auto", "nopack"):
            gw = ops._gap_weights(self.w, pack=self.route != "nopack")
            assert (gw.packed is None) == (self.route == "nopack")
            need = lib.amds_gated_attn_pool_batched_workspace_bytes(rows, B, F, L, D)
            assert need > 0
            ws, hw = G.guarded((need,), torch.uint8, self.gpu, band_bytes=G.FLAT_BAND_BYTES, pattern=0xFF, name="ws")
            off = torch.tensor([0] + list(self.lengths), dtype=torch.int64).cumsum(0).to(self.gpu)
            mode = ops.GAP_MODES["auto" if self.route == "nopack" else self.mode]
            _lib.check(lib.amds_gated_attn_pool_batched(x.data_ptr(), off.data_ptr(), B, rows, C.byref(gw), out.data_ptr(), araw.data_ptr(), F, L, D, mode,
                                                        ws.data_ptr(), need, st), "gated_attn_pool_batched")
            handles = [hw]
        else:
            unfused = self.route == "unfused"
            gw = ops._gap_weights(self.w, pack=not unfused)
            sz, fn = ((lib.amds_gated_attn_pool_unfused_workspace_bytes, lib.amds_gated_attn_pool_unfused) if unfused else
                      (lib.amds_gated_attn_pool_workspace_bytes, lib.amds_gated_attn_pool))
            need = max(sz(n, F, L, D) for n in set(self.lengths))
            ws, hw = G.guarded((need,), torch.uint8, self.gpu, band_bytes=G.FLAT_BAND_BYTES, pattern=0xFF, name="ws")
            o = 0
            for i, n in enumerate(self.lengths):
                _lib.check(fn(x.data_ptr() + 4 * o * F, C.byref(gw), out.data_ptr() + 4 * i * F, araw.data_ptr() + 4 * o, n, F, L, D, ws.data_ptr(), sz(n, F, L, D), st),
                           "gated_attn_pool")
                o += n
            handles = [hw]
        torch.cuda.synchronize()
        for h in (ho, ha, *handles):
            h.assert_bands_intact()
        return araw.clone(), out.clone()


def _alone(gpu, mode, xb, w):
    """One bag through the batched entry without an offset table, mode forced -> (A_raw, out[0])."""
    lib = _lib.lib()
    n, F = xb.shape
    L, D = w["fc_w"].shape[0], w["a_w"].shape[0]
    need = lib.amds_gated_attn_pool_batched_workspace_bytes(n, 1, F, L, D)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu)
    out, araw = torch.empty(1, F, device=gpu), torch.empty(n, device=gpu)
    gw = ops._gap_weights(w)
    _lib.check(lib.amds_gated_attn_pool_batched(xb.data_ptr(), None, 1, n, C.byref(gw), out.data_ptr(), araw.data_ptr(), F, L, D, ops.GAP_MODES[mode],
                                                ws.data_ptr(), need, ops._stream()), "gated_attn_pool_batched")
    return araw, out[0]


def _alone_bags(B):
    if B <= 32:
        return list(range(B))
    if B <= 300:
        return [0, 1, 2, 3] + list(range(250, B))
    return sorted({0, 1, 255, 256, 257, 65535, 65536, B - 1} | set(range(7, B, 4099)))


def _form_of(route, total, F, L, D):
    """Which association a call of `total` rows takes: 16 / 64 (rows per unit of the fused forms) or 128 (the six-launch form)."""
    if route == "unfused" or L not in (256, 512):
        return 128
    if route == "slab":
        return 64
    if route == "split":
        return 16
    return 16 if total <= SPLIT_AUTO_ROWS and _split_ok(F, D) else 64


def _ratio(err, bar):
    """max err / bar; where the bar is 0 the error must be 0 (-> inf otherwise).  Zero: below half the smallest fp32 subnormal -- the fp64 reference keeps
    exp(-128) ~ 1e-56 of every losing row, which shows where the winners' sum cancels to 0."""
    zero = bar == 0
    err = torch.where(err < 2.0 ** -150, torch.zeros_like(err), err)
    r = torch.where(zero, torch.where(err == 0, 0.0, float("inf")), err / torch.where(zero, torch.ones_like(bar), bar))
    return float(r.max())


@pytest.mark.parametrize("geom,route", ITEMS)
def test_gap_form(gpu, geom, route):
    F, L, D, lengths, _, families = O.GEOMS[geom]
    if route == "split":
        assert _split_ok(F, D) and sum(lengths) <= 12288
    for family in families:
        x, _, w, ref = _case(geom, family)
        call = _Call(gpu, route, x, lengths, w)
        A, out = call.run()
        assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(out).all()), f"{geom}/{family}: non-finite output"
        per_bag = route in ("pool", "unfused")
        totals = ref.lengths if per_bag else torch.full_like(ref.lengths, int(ref.lengths.sum()))
        forms = [_form_of(route, int(t), F, L, D) for t in sorted(set(totals.tolist()))]
        rows_of = {int(t): f for t, f in zip(sorted(set(totals.tolist())), forms)}
        rpu = torch.tensor([rows_of[int(t)] for t in totals.tolist()], device=gpu)
        six = rpu == 128
        if family in O.GRID_FAMILIES:
            barA = torch.zeros_like(ref.A)
            barO = torch.where(six[:, None], O.grid_out_bar(ref, six_launch=True), O.grid_out_bar(ref))
            errA = (A.double() - ref.A.float().double()).abs()         # "bit-equal to fp64": to fp64 rounded to fp32 (fp64 keeps sigmoid(32) = 1 - 1.3e-14)
            pow2 = (ref.nwin & (ref.nwin - 1)) == 0
            assert torch.equal(out[pow2], ref.out.float()[pow2]), f"{geom}/{family}: out not bit-equal where the winner count is a power of two"
        else:
            depth = torch.where(six, O.depth_unfused(ref.lengths), O.depth_fused(ref.lengths, rpu))
            barA, barO = O.real_bars(ref, depth)
            errA = (A.double() - ref.A).abs()
        rA, rO = _ratio(errA, barA), _ratio((out.double() - ref.out).abs(), barO)
        print(f"gap| {route} | {geom} | {family} | A_raw {rA:.4f} | out {rO:.4f}")
        key = (route, "I" if family in O.GRID_FAMILIES else "II")
        _WORST[key] = max(_WORST.get(key, 0.0), rA, rO)
        assert rA <= 1.0, f"{geom}/{family}/{route}: A_raw error / bar = {rA}"
        assert rO <= 1.0, f"{geom}/{family}/{route}: out error / bar = {rO}"
        A2, out2 = call.run()
        assert torch.equal(A, A2) and torch.equal(out, out2), f"{geom}/{family}/{route}: two calls differ"
        if route in ("slab", "split"):
            offs = [0]
            for n in lengths:
                offs.append(offs[-1] + n)
            same = []
            for b in _alone_bags(len(lengths)):
                a1, o1 = _alone(gpu, route, x[offs[b]:offs[b + 1]], w)
                same.append((a1 == A[offs[b]:offs[b + 1]]).all() & (o1 == out[b]).all())
            bad = [b for b, ok in zip(_alone_bags(len(lengths)), torch.stack(same).tolist()) if not ok]
            assert not bad, f"{geom}/{family}/{route}: bags {bad[:8]} differ from the bag pooled alone"


def test_zz_worst_figures(gpu):
    """Not a check of its own: the table of profiles/gap_kernel_errors.txt (worst error / bar per form and family; family I: 0 = every bit equal)."""
    for (route, fam), v in sorted(_WORST.items()):
        print(f"gap| worst | {route} | family {fam} | {v:.4f}")
    print(f"gap| {len(ITEMS)} items in {time.time() - _T0:.1f} s")
