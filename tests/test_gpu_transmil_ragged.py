"""Ragged bags through the TransMIL head: N bags of different lengths packed without padding, one library call (amds_transmil_forward_ragged,
csrc/transmil_ragged.hip), each bag computed as the reference computes it at batch 1 -- its own grid, front padding and pseudo-inverse scale."""
import ctypes as C
import contextlib
import functools

import pytest
import torch

from oracle.transmil import transmil_forward
from stamp_amd import _lib, ops
from stamp_amd.mil import TransMIL

pytestmark = pytest.mark.gpu

COHORT = [1, 2, 3, 50, 255, 256, 257, 300, 511, 1024, 1025, 2300]
# Per-bag pinv start (test 2).  E0: the largest |logit error| of the existing one-bag call `model(b[None])` against the fp64 one-bag oracle over PARITY_COHORT at
# "highest", measured on the MI355X at the parent commit (profiles/transmil_ragged_parity.txt).  The ragged call's bar is 4 x E0: its packed token-row products may
# land on a differently tiled kernel than the one-bag call's (another summation order); nothing else differs.
PARITY_COHORT = [300, 50, 300, 1024, 257]
E0 = 7.463e-7
BAR = 4 * E0


@contextlib.contextmanager
def _precision(level):
    old = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision(level)
    try:
        yield
    finally:
        torch.set_float32_matmul_precision(old)


def _model(dim_input, dim_hidden, C_=3, seed=0):
    torch.manual_seed(seed)
    m = TransMIL(dim_output=C_, dim_input=dim_input, dim_hidden=dim_hidden).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return m


def _oracle_rows(m, bags):
    """The fp64 oracle on every bag ALONE (the reference's batch-1 semantics) -> [N, C] fp64."""
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    return torch.cat([transmil_forward(b[None].double().cpu(), sd, dtype=torch.float64) for b in bags], dim=0)


@functools.lru_cache(maxsize=None)
def _cohort_case(dim_input, dim_hidden):
    """(model on the CPU, bags, fp64 one-bag references).  Feature values are multiples of 1/16 in [-63/16, 63/16]: exact in fp32, fp16 and bf16, so ONE reference serves
    every feats dtype."""
    m = _model(dim_input, dim_hidden)
    g = torch.Generator().manual_seed(1)
    bags = [(torch.randn(t, dim_input, generator=g) * 16).round().clamp(-63, 63) / 16 for t in COHORT]
    assert all(torch.equal(b.half().float(), b) and torch.equal(b.bfloat16().float(), b) for b in bags)
    return m, bags, _oracle_rows(m, bags)


@functools.lru_cache(maxsize=None)
def _parity_case():
    """dim_hidden 512, dim_input 256, randn(...).half().float() feats, seed 5; PARITY_COHORT holds two 300-tile bags (positions 0 and 2)."""
    m = _model(256, 512, C_=2, seed=5)
    g = torch.Generator().manual_seed(5)
    bags = [torch.randn(t, 256, generator=g).half().float() for t in PARITY_COHORT]
    return m, bags, _oracle_rows(m, bags)


def _coupling_gap(m, bags):
    """fp64, CPU: the two 300-tile bags run as ONE dense batch of 2 (one pinv scale for both, trans_mil.py:28) against each alone."""
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    pair = torch.stack([bags[0], bags[2]]).double()
    both = transmil_forward(pair, sd, dtype=torch.float64)
    alone = torch.cat([transmil_forward(pair[i:i + 1], sd, dtype=torch.float64) for i in range(2)])
    return (both - alone).abs().max().item()


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("dims", [(1024, 512), (24, 64)])
def test_ragged_rows_match_the_one_bag_oracle(gpu, dims, dt, precision):
    m, bags, ref = _cohort_case(*dims)
    m = m.to(gpu)
    with torch.no_grad(), _precision(precision):
        out = m.forward_ragged([b.to(dt).to(gpu) for b in bags])
    assert out.shape == (len(bags), 3) and out.dtype == torch.float32 and torch.isfinite(out).all()
    err = (out.double().cpu() - ref).abs()
    print("dims", dims, dt, precision, "max err", err.max().item(), "per bag", [f"{e:.2e}" for e in err.max(1).values.tolist()])
    for i, t in enumerate(COHORT):                              # the dense forward's own bar (tests/test_gpu_mil.py, bag of 1 024 against the oracle)
        bar = 2e-3 * max(1.0, ref[i].abs().max().item())
        assert err[i].max().item() < bar, (i, t, err[i], ref[i], out[i])


def test_pinv_start_is_per_bag(gpu):
    """The test a dense-style batch (one pinv scale for the whole call) fails: at "highest" every row stays within 4 x E0 of its fp64 one-bag oracle, and that bar
    is at least 5 x below the coupling gap between the two 300-tile bags run as a batch of 2 and run alone."""
    m, bags, ref = _parity_case()
    g = _coupling_gap(m, bags)
    print("coupling gap g", g, "E0", E0, "bar", BAR)
    assert BAR > 0 and g >= 5 * BAR, (g, BAR)
    m = m.to(gpu)
    with torch.no_grad(), _precision("highest"):
        out = m.forward_ragged([b.to(gpu) for b in bags])
        one = torch.cat([m(b[None].to(gpu)) for b in bags])
    err = (out.double().cpu() - ref).abs().max().item()
    e_one = (one.double().cpu() - ref).abs().max().item()
    print("ragged err", err, "one-bag err", e_one)
    assert err <= BAR, (err, BAR)


def test_grouped_pinv_init_with_one_group_gives_the_bits_of_pinv_init(gpu):
    lib = _lib.lib()
    torch.manual_seed(2)
    for n in (256, 32, 30):
        x = torch.softmax(torch.randn(16, n, n, device=gpu) * 3, dim=-1)
        za, zb, zc = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        sa, sb = torch.zeros(2, dtype=torch.int32, device=gpu), torch.zeros(4, dtype=torch.int32, device=gpu)
        _lib.check(lib.amds_pinv_init(x.data_ptr(), za.data_ptr(), 8, n, sa.data_ptr(), ops._stream()), "pinv_init")
        _lib.check(lib.amds_pinv_init_grouped(x.data_ptr(), zb.data_ptr(), 8, n, 8, sa.data_ptr(), ops._stream()), "pinv_init_grouped")
        assert torch.equal(za[:8], zb[:8])
        # two groups: each the bits of its own amds_pinv_init
        _lib.check(lib.amds_pinv_init_grouped(x.data_ptr(), zc.data_ptr(), 16, n, 8, sb.data_ptr(), ops._stream()), "pinv_init_grouped")
        _lib.check(lib.amds_pinv_init(x[8:].data_ptr(), za[8:].data_ptr(), 8, n, sa.data_ptr(), ops._stream()), "pinv_init")
        assert torch.equal(zc, za)
        col, row = x.abs().sum(-1), x.abs().sum(-2)
        want = x.transpose(-1, -2) / (col.view(2, -1).max(1).values * row.view(2, -1).max(1).values).repeat_interleave(8)[:, None, None]
        assert torch.allclose(zc, want, rtol=1e-5, atol=0)
    assert lib.amds_pinv_init_grouped(x.data_ptr(), zb.data_ptr(), 12, n, 8, sb.data_ptr(), ops._stream()) == -1 and b"groups" in lib.amds_last_error()


def test_order_grouping_and_repeat_invariance(gpu):
    m, bags, ref = _parity_case()
    m = m.to(gpu)
    dev = [b.to(gpu) for b in bags]
    n = len(dev)
    with torch.no_grad(), _precision("highest"):
        base = m.forward_ragged(dev)
        assert torch.equal(m.forward_ragged(dev), base)                                  # the same call twice
        rev = m.forward_ragged(dev[::-1]).flip(0)
        assert (rev - base).abs().max().item() <= BAR
        for k in (1, 3, n):
            got = m.forward_ragged(dev, bags_per_call=k)
            assert got.shape == base.shape and (got - base).abs().max().item() <= BAR, k
        narrow = m.forward_ragged(dev, max_rows_per_call=600)                            # every 300-tile bag (np = 512) with at most one neighbour
        assert (narrow - base).abs().max().item() <= BAR
        for i, b in enumerate(dev):
            one = m(b[None])
            solo = m.forward_ragged([b])
            assert (solo - one).abs().max().item() <= BAR and (solo - base[i:i + 1]).abs().max().item() <= BAR, i


def test_predict_groups_one_bag_batches_and_keeps_the_patient_order(gpu):
    from stamp_amd.deploy import predict_

    m, bags, _ = _parity_case()
    m = m.to(gpu)
    batches = [(b[None], None, None, None) for b in bags]
    batches.insert(2, (torch.stack([bags[1], bags[1]]), None, None, None))               # a two-bag batch keeps its own forward, between the grouped ones
    pids = [f"p{i}" for i in range(len(bags) + 2)]
    with _precision("highest"):
        base = predict_(m, batches, pids, task="classification", device=gpu)
        for k in (2, 3, 64):
            got = predict_(m, batches, pids, task="classification", device=gpu, bags_per_call=k)
            assert list(got) == pids
            for p in pids:                                                                # probabilities: softmax is 1-Lipschitz in the max norm
                assert (got[p] - base[p]).abs().max().item() <= BAR, (k, p)
        small = predict_(m, batches, pids, task="classification", device=gpu, bags_per_call=64, max_rows_per_call=600)
        assert list(small) == pids and all((small[p] - base[p]).abs().max().item() <= BAR for p in pids)


def test_class_row_tail_on_and_off_agree(gpu):
    m, bags, ref = _parity_case()
    m = m.to(gpu)
    dev = [b.to(gpu) for b in bags]
    with torch.no_grad(), _precision("highest"):
        on = m.forward_ragged(dev)
        was = ops.set_mil_cls_tail(False)
        try:
            off = m.forward_ragged(dev)
        finally:
            ops.set_mil_cls_tail(was)
    print("tail on/off", (on - off).abs().max().item())
    assert torch.isfinite(off).all() and (on - off).abs().max().item() <= BAR
    assert (off.double().cpu() - ref).abs().max().item() <= BAR
    # at "high" the one-row products of the tail take another kernel than the full layer's (bf16 x 3 tiles): both stay within the dense forward's bar of the oracle
    with torch.no_grad(), _precision("high"):
        on_h = m.forward_ragged(dev)
        was = ops.set_mil_cls_tail(False)
        try:
            off_h = m.forward_ragged(dev)
        finally:
            ops.set_mil_cls_tail(was)
    print("tail on/off at high", (on_h - off_h).abs().max().item())
    for got in (on_h, off_h):
        assert (got.double().cpu() - ref).abs().max().item() < 2e-3 * max(1.0, ref.abs().max().item())


def test_c_entry_checks(gpu):
    from stamp_amd import transmil_core

    lib = _lib.lib()
    m = _model(24, 64).to(gpu)
    w = m._c_weights(torch.device(gpu))
    cfg = _lib.TransMilCfg(24, 64, 3)
    lengths = [5, 70, 1]
    tiles = (C.c_int * 3)(*lengths)
    table, _, _ = transmil_core.ragged_plan(lengths, 64)
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(gpu)
    feats = torch.randn(sum(lengths), 24, device=gpu)
    logits = torch.zeros(3, 3, device=gpu)
    need = lib.amds_transmil_ragged_workspace_bytes(C.byref(cfg), 3, tiles)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)

    def call(n=3, feats_p=feats.data_ptr(), tiles_p=tiles, table_p=table_dev.data_ptr(), logits_p=logits.data_ptr(), ws_p=ws.data_ptr(), ws_n=need):
        return lib.amds_transmil_forward_ragged(C.byref(cfg), C.byref(w), feats_p, _lib.F32, tiles_p, table_p, logits_p, n, ws_p, ws_n, ops._stream())

    assert call(n=0) == 0 and call(n=0, feats_p=None, tiles_p=None, table_p=None, logits_p=None, ws_p=None, ws_n=0) == 0      # zero bags: OK, nothing launched
    torch.cuda.synchronize()
    assert logits.abs().max().item() == 0
    for kw in (dict(feats_p=None), dict(table_p=None), dict(logits_p=None), dict(ws_p=None), dict(tiles_p=None)):
        assert call(**kw) == -1 and b"null" in lib.amds_last_error(), kw
    assert call(ws_n=need - 256) == -2 and b"workspace" in lib.amds_last_error()         # AMDS_ERR_WORKSPACE
    assert call(ws_p=ws.data_ptr() + 16, ws_n=need - 16) != 0
    assert call(tiles_p=(C.c_int * 3)(5, 0, 1)) == -1 and b"empty bag" in lib.amds_last_error()
    with torch.no_grad(), _precision("highest"):
        ops.sync_float32_matmul_precision()                                               # the C entry follows the context's level, not torch's flag
        assert call() == 0
        want = m.forward_ragged(list(feats.split(lengths)))
    assert torch.equal(logits, want)
