"""Host side of the ragged barspoon forward: grouping without a class-token row, validation of `EncDecTransformer.forward_ragged`, the host-only
exports (workspace size, the shared-call limit) and `predict_`'s handling of `bags_per_call` for multi-target heads -- no kernels."""
import ctypes as C
import os

import pytest
import torch

from stamp_amd import _lib
from stamp_amd.barspoon import EncDecTransformer
from stamp_amd.deploy import predict_
from stamp_amd.mil_core import MAX_SOLO_TILES, group_bags


def test_group_bags_without_the_class_token_row():
    # rows = tiles alone: 3 bags of 10 tiles fill 30 rows exactly (with a class token each they would need 33)
    assert group_bags([10, 10, 10, 10], 64, 30, extra_rows=0) == [(0, 3), (3, 4)]
    assert group_bags([10, 10, 10, 10], 64, 30, extra_rows=1) == [(0, 2), (2, 4)]
    assert group_bags([9, 9, 9, 9], 64, 27, extra_rows=0) == [(0, 3), (3, 4)]
    # a bag whose rows alone exceed the limit runs alone; exactly at the limit it may still be joined by nothing
    assert group_bags([5, 50, 5], 64, 50, extra_rows=0) == [(0, 1), (1, 2), (2, 3)]
    assert group_bags([5, 100, 5], 64, 50, extra_rows=0) == [(0, 1), (1, 2), (2, 3)]
    # too long to share: alone, neighbours keep their order; bags_per_call still counts bags
    assert group_bags([3, 5889, 4, 5], 64, 10 ** 9, max_shared=5888, extra_rows=0) == [(0, 1), (1, 2), (2, 4)]
    assert group_bags([3, 5888, 4, 5], 64, 10 ** 9, max_shared=5888, extra_rows=0) == [(0, 4)]
    assert group_bags([1] * 5, 2, 10 ** 9, extra_rows=0) == [(0, 2), (2, 4), (4, 5)]
    assert group_bags([], 4, 1000, extra_rows=0) == []
    with pytest.raises(ValueError):
        group_bags([1], 1, 10, extra_rows=2)
    # every bag once, in order, within the limits
    g = torch.Generator().manual_seed(0)
    lengths = [int(x) for x in torch.randint(1, 20000, (300,), generator=g)]
    for k, rows, shared in ((1, 10 ** 9, 32767), (7, 262144, 5888), (64, 65536, 16128)):
        groups = group_bags(lengths, k, rows, shared, extra_rows=0)
        assert [a for a, _ in groups] == [0] + [e for _, e in groups[:-1]] and groups[-1][1] == len(lengths)
        for a, e in groups:
            assert 1 <= e - a <= k
            if e - a > 1:
                assert sum(lengths[a:e]) <= rows and max(lengths[a:e]) <= shared


def test_group_bags_default_keeps_todays_groups():
    """extra_rows = 1 and the default on the cases of tests/test_cpu_mil_ragged.py."""
    cases = [(([], 4, 1000), {}, []),
             (([10] * 10, 4, 10 ** 9), {}, [(0, 4), (4, 8), (8, 10)]),
             (([9, 9, 9, 9], 64, 30), {}, [(0, 3), (3, 4)]),
             (([5, 100, 5], 64, 50), {}, [(0, 1), (1, 2), (2, 3)]),
             (([3, 40000, 4, 5], 64, 10 ** 9), {}, [(0, 1), (1, 2), (2, 4)]),
             (([3, 33000, 4], 64, 10 ** 9), dict(max_shared=10 ** 6), [(0, 1), (1, 2), (2, 3)]),
             (([3, 8000, 4, 7936], 64, 10 ** 9), dict(max_shared=7935), [(0, 1), (1, 2), (2, 3), (3, 4)]),
             (([MAX_SOLO_TILES, 1], 64, 10 ** 9), {}, [(0, 2)])]
    for args, kw, want in cases:
        assert group_bags(*args, **kw) == want, args
        assert group_bags(*args, extra_rows=1, **kw) == want, args
    g = torch.Generator().manual_seed(0)
    lengths = [int(x) for x in torch.randint(1, 20000, (300,), generator=g)]
    for k, rows, shared in ((1, 10 ** 9, 32767), (7, 262144, 7935), (64, 65536, 32767)):
        assert group_bags(lengths, k, rows, shared) == group_bags(lengths, k, rows, shared, extra_rows=1)


def _tiny(positional_encoding=True):
    return EncDecTransformer(16, {"A": 2, "B": 3}, d_model=32, num_encoder_heads=2, num_decoder_heads=2, num_encoder_layers=1, num_decoder_layers=1,
                             dim_feedforward=32, positional_encoding=positional_encoding)


def test_forward_ragged_refusals():
    m = _tiny().eval()
    b, p = [torch.randn(5, 16), torch.randn(3, 16)], [torch.rand(5, 2), torch.rand(3, 2)]
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_ragged(b, p)                                          # grad mode
    m.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval"):
        m.forward_ragged(b, p)                                          # train mode
    m.eval()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU"):
            m.forward_ragged(b, p)                                      # CPU tensors
        with pytest.raises(ValueError, match="empty"):
            m.forward_ragged([b[0], b[1][:0]], [p[0], p[1][:0]])
        with pytest.raises(ValueError, match="features"):
            m.forward_ragged([b[0], torch.randn(3, 12)], p)             # ragged feature widths
        with pytest.raises(ValueError, match="features"):
            m.forward_ragged([torch.randn(5, 12), torch.randn(3, 12)], p)       # one width, not the model's
        with pytest.raises(ValueError, match="positions"):
            m.forward_ragged(b)                                         # positional_encoding=True needs them
        with pytest.raises(ValueError, match="positions"):
            m.forward_ragged(b, [p[0], None])
        with pytest.raises(ValueError, match="positions"):
            m.forward_ragged(b, [p[0], torch.rand(4, 2)])               # shaped unlike its bag
        with pytest.raises(ValueError, match="positions"):
            m.forward_ragged(b, [p[0]])                                 # one list shorter than the other
        with pytest.raises(ValueError):
            m.forward_ragged([b[0], torch.randn(2, 3, 16)], p)          # not [tiles, features]
        out = _tiny().eval().forward_ragged([], [])
        assert list(out) == ["A", "B"] and out["A"].shape == (0, 2) and out["B"].shape == (0, 3) and out["A"].dtype == torch.float32
        # without positional encoding the positions are optional
        with pytest.raises(RuntimeError, match="GPU"):
            _tiny(False).eval().forward_ragged(b)


def _cfg(n_feats=768, dim=512, enc_heads=8, dec_heads=8, ff=2048, enc_layers=2, dec_layers=2, n_targets=2, pe=1, dtype=_lib.F16):
    return _lib.BarspoonCfg(n_feats, dim, enc_heads, dec_heads, ff, enc_layers, dec_layers, n_targets, pe, dtype)


def test_ragged_workspace_bytes_and_refusals():
    lib = _lib.lib()

    def refused(n, msg):
        assert n == 0 and msg in lib.amds_last_error(), (n, lib.amds_last_error())

    ok = _cfg()
    ws = lib.amds_barspoon_ragged_workspace_bytes
    need = ws(C.byref(ok), 3, 100, 50)
    assert need > 0 and need % 256 == 0
    # the dense plan's buffers over the same rows, plus the per-call table
    assert need >= lib.amds_barspoon_workspace_bytes(C.byref(ok), 1, 100) + lib.amds_attention_varlen_workspace_bytes(3, 100)
    assert ws(C.byref(ok), 0, 0, 0) > 0                                             # an empty call is a valid call
    refused(ws(None, 3, 100, 50), b"null config")
    refused(ws(C.byref(_cfg(dim=520, enc_heads=8, dec_heads=8)), 3, 100, 50), b"head_dim <= 64")           # head_dim 65
    refused(ws(C.byref(_cfg(dim=512, enc_heads=4)), 3, 100, 50), b"head_dim <= 64")                        # encoder head_dim 128
    refused(ws(C.byref(_cfg(dtype=_lib.F32)), 3, 100, 50), b"operand dtype must be f16 or bf16")
    refused(ws(C.byref(_cfg(n_targets=0)), 3, 100, 50), b"bad config")
    refused(ws(C.byref(ok), 65536, 70000, 50), b"bad shape n_bags=65536")
    refused(ws(C.byref(ok), 9000, 9000, 1), b"decoder heads")                       # 9000 x 8 batches of one fp32 product
    refused(ws(C.byref(ok), -1, 100, 50), b"bad shape n_bags=-1")
    refused(ws(C.byref(ok), 3, -1, 50), b"bad shape")
    refused(ws(C.byref(ok), 3, 100, -1), b"bad shape")
    refused(ws(C.byref(ok), 3, 2, 1), b"at least one tile")                         # fewer tiles than bags


def test_ragged_max_shared_tiles():
    lib = _lib.lib()
    f = lib.amds_barspoon_ragged_max_shared_tiles
    assert f(None) == -1 and b"null config" in lib.amds_last_error()
    assert f(C.byref(_cfg(dtype=_lib.F32))) == -1
    assert f(C.byref(_cfg(dim=520))) == -1
    n = f(C.byref(_cfg()))
    assert n >= 1
    # the limit of the `vit` head's rule on barspoon's widest GEMM (T, FFp = 2048, Dp): the 256-row kernel takes over at ceil(T / 256) * 8 >= 192
    if not os.environ.get("AMDS_GEMM_CFG"):
        assert n == 23 * 256
        small = _cfg(n_feats=96, dim=128, enc_heads=4, dec_heads=2, ff=256, n_targets=3)
        assert f(C.byref(small)) == 63 * 256                                        # (T, 3 Da = 768, Dp): ceil(T / 256) * 3 >= 192


class _Multi(torch.nn.Module):                       # the barspoon head's surface without being one: forward(tokens, positions) -> {target: logits}
    target_labels = ["A", "B"]
    class_tokens = None
    calls = 0

    def forward(self, x, pos):
        type(self).calls += 1
        m = x.float().mean(1)
        return {"A": m[:, :2], "B": m[:, 2:5]}


def test_predict_duck_typed_multi_target_head_ignores_bags_per_call():
    bags = [torch.randn(1, n, 8) for n in (4, 7, 2, 9)]
    batches = [(b, torch.zeros(1, b.shape[1], 2), None, None) for b in bags]
    pids = ["w", "x", "y", "z"]
    base = predict_(_Multi(), batches, pids, task="classification", device="cpu")
    _Multi.calls = 0
    got = predict_(_Multi(), batches, pids, task="classification", device="cpu", bags_per_call=4)
    assert _Multi.calls == 4                                # one forward per batch: no ragged entry is looked for
    assert list(got) == list(base) == pids
    for pid in pids:
        for t in ("A", "B"):
            assert torch.equal(got[pid][t], base[pid][t])
    with pytest.raises(ValueError, match="bags_per_call"):
        predict_(_Multi(), batches, pids, task="classification", device="cpu", bags_per_call=0)
    with pytest.raises(ValueError, match="bags_per_call"):
        predict_(_tiny().eval(), batches, pids, task="classification", device="cpu", bags_per_call=0)
