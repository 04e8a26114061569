"""Host side of `HipTransMilTrainer` (stamp_amd/transmil_train.py), no GPU: the PPEG window layout the unpack kernel is compared against, the flat
parameter / gradient layout and its views, the C structs over them, the `group_valid_bags` hook of `mil_train._validate_ragged`, the new export."""
import ctypes

import pytest
import torch

from stamp_amd import _lib, mil_core, mil_train, ops, transmil_core
from stamp_amd.mil import TransMIL
from stamp_amd.transmil_train import HipTransMilTrainer, flat_layout
from transmil_trainer_cases import PPEG_NAMES, ppeg_windows


class _BackwardStub:
    """Stands in for the library under `transmil_core.backward`: the backward call writes a given table where `amds_transmil_grads.ppeg_corr` points."""

    def __init__(self, table):
        self.table = table.contiguous()

    def amds_transmil_train_workspace_bytes(self, cfg, n_bags, n_tiles):
        return 256

    def amds_transmil_train_backward(self, cfg, w, dlogits, p_drop, seed, n_bags, n_tiles, saved, saved_bytes, grads, dbags, ws, ws_bytes, stream):
        ctypes.memmove(grads._obj.ppeg_corr, self.table.data_ptr(), self.table.numel() * 4)
        return 0


@pytest.mark.parametrize("Cd", [64, 512])
def test_ppeg_windows_equal_the_slicing_of_the_module_path(monkeypatch, Cd):
    """`ppeg_windows` -- the torch restatement the kernel test compares `amds_ppeg_grads_unpack` against -- equals what `transmil_core.backward` itself cuts out
    of the table its library call returned (here: a stub that writes a random table), tensor for tensor, shape and bits."""
    table = torch.randn(50, Cd, generator=torch.Generator().manual_seed(Cd))
    monkeypatch.setattr(_lib, "lib", lambda: _BackwardStub(table))
    monkeypatch.setattr(ops, "sync_float32_matmul_precision", lambda: "highest")
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    saved = dict(dims=(8, Cd, 2), shape=(1, 4, 8), cfg=_lib.TransMilCfg(8, Cd, 2, 0), w=_lib.TransMilWeights(), arena=torch.zeros(256, dtype=torch.uint8), p_out=0.0, seed=0)
    G, dbags = transmil_core.backward(saved, torch.zeros(1, 2))
    want = ppeg_windows(table)
    assert dbags is None and set(PPEG_NAMES) <= set(G)
    for k, s in zip(PPEG_NAMES, [(Cd, 1, 7, 7), (Cd, 1, 5, 5), (Cd, 1, 3, 3), (Cd,), (Cd,), (Cd,)]):
        assert want[k].shape == s == G[k].shape and want[k].is_contiguous() and torch.equal(want[k], G[k]), k
    # the layout in words: tap r * 7 + q of channel c is w7[c, 0, r, q]; the 5 x 5 and 3 x 3 kernels are its centre windows; every bias is tap 49
    c, r, q = Cd - 3, 4, 2
    assert want[PPEG_NAMES[0]][c, 0, r, q] == table[r * 7 + q, c] and want[PPEG_NAMES[1]][c, 0, r - 1, q - 1] == table[r * 7 + q, c]
    assert want[PPEG_NAMES[2]][c, 0, r - 2, q - 2] == table[r * 7 + q, c] and all(torch.equal(want[k], table[49]) for k in PPEG_NAMES[3:])


def _trainer(dim_hidden=64, dim_input=24, C_=3, **kw):
    torch.manual_seed(0)
    return HipTransMilTrainer(TransMIL(dim_output=C_, dim_input=dim_input, dim_hidden=dim_hidden), device="cpu", **kw)


@pytest.mark.parametrize("dim_hidden", [64, 512])
def test_flat_layout_covers_the_state_dict_once_in_its_order(dim_hidden):
    tr = _trainer(dim_hidden)
    sd = tr.model.state_dict()
    assert tr.names == list(sd) and list(tr.offs) == tr.names
    at = 0
    for k in tr.names:                                     # back to back, in the state_dict's order: no gap, no overlap
        assert tr.offs[k] == (at, sd[k].numel()), k
        at += sd[k].numel()
    assert at == tr.P.numel() == tr.G.numel() == tr.m.numel() == tr.v.numel() == sum(v.numel() for v in sd.values())
    assert flat_layout({k: tuple(v.shape) for k, v in sd.items()}) == (tr.offs, at)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (tr.P, tr.G, tr.m, tr.v))
    for k in tr.names:                                     # views: same storage, the offset's address, 16-byte aligned, the module's shape and values
        o = tr.offs[k][0]
        for view, flat in ((tr.p(k), tr.P), (tr.g(k), tr.G)):
            assert view.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and view.data_ptr() == flat.data_ptr() + 4 * o
            assert view.shape == sd[k].shape and view.is_contiguous() and (4 * o) % 16 == 0
        assert torch.equal(tr.p(k), sd[k])
    tr.p("norm.bias")[3] = 7.0
    tr.g("_fc2.weight")[1, 2] = -2.0
    assert tr.P[tr.offs["norm.bias"][0] + 3] == 7.0 and tr.G[tr.offs["_fc2.weight"][0] + dim_hidden + 2] == -2.0


def test_c_structs_point_into_the_flat_buffers():
    tr = _trainer()
    at = lambda flat, k: flat.data_ptr() + 4 * tr.offs[k][0]  # noqa: E731
    w, g = tr._w, tr._gc
    pairs = [("fc1_w", "_fc1.0.weight"), ("fc1_b", "_fc1.0.bias"), ("cls_token", "cls_token"), ("norm_w", "norm.weight"), ("norm_b", "norm.bias"),
             ("fc2_w", "_fc2.weight"), ("fc2_b", "_fc2.bias")]
    for f, k in pairs:
        assert getattr(w, f) == at(tr.P, k) and getattr(g, f) == at(tr.G, k), f
    for f, k in (("ppeg_w7", "pos_layer.proj.weight"), ("ppeg_b7", "pos_layer.proj.bias"), ("ppeg_w5", "pos_layer.proj1.weight"), ("ppeg_b5", "pos_layer.proj1.bias"),
                 ("ppeg_w3", "pos_layer.proj2.weight"), ("ppeg_b3", "pos_layer.proj2.bias")):
        assert getattr(w, f) == at(tr.P, k), f
    for i, nm in enumerate(("layer1", "layer2")):
        for f, k in (("norm_w", "norm.weight"), ("norm_b", "norm.bias"), ("qkv_w", "attn.to_qkv.weight"), ("out_w", "attn.to_out.0.weight"),
                     ("out_b", "attn.to_out.0.bias"), ("conv_w", "attn.res_conv.weight")):
            assert getattr(w.layer[i], f) == at(tr.P, f"{nm}.{k}") and getattr(g.layer[i], f) == at(tr.G, f"{nm}.{k}"), (nm, f)
    assert g.ppeg_corr == tr._corr.data_ptr() and tr._corr.shape == (50, 64)          # the table is a buffer of its own; the unpack kernel fills G's six views


def test_sync_and_load_round_trip_bit_for_bit():
    tr = _trainer()
    tr.P.copy_(torch.randn(tr.P.numel(), generator=torch.Generator().manual_seed(1)))
    want = tr.P.clone()
    tr.sync_to_model()
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v, tr.p(k)) and v.data_ptr() != tr.p(k).data_ptr(), k
    tr.P.zero_()
    tr.load_from_model()
    assert torch.equal(tr.P, want)
    tr._refresh()                                          # `fit` calls it after restoring P: nothing derived to rebuild
    assert torch.equal(tr.P, want)


def test_surface_and_cpu_tensors_raise():
    tr = _trainer(dropout=False, sched_interval="step", total_steps=5, max_lr=1e-3)
    assert tr.skipped_steps == 0 and tr.current_loss_scale == 1.0 and tr.step_count == 0 and tr.train_pred_median is None and tr.use_dropout is False
    assert tr.clock.interval == "step" and len(tr.clock.lrs) == 5 and tr.dims == (24, 64, 3)
    assert _trainer().use_dropout is True
    with pytest.raises(RuntimeError, match="GPU"):
        tr.step(torch.zeros(2, 5, 24), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        tr.predict(torch.zeros(2, 5, 24))
    with pytest.raises(RuntimeError, match="GPU"):
        tr.predict_ragged([torch.zeros(5, 24)])
    with pytest.raises(ValueError):
        HipTransMilTrainer(tr.model, device="cpu", sched_interval="batch")
    assert tr.predict_ragged([]).shape == (0, 3)
    lens = [50, 300, 20, 1000, 7]
    assert tr.group_valid_bags(lens, 2) == transmil_core.group_bags_padded(lens, 64, 2, tr.valid_max_rows_per_call) == [(0, 2), (2, 4), (4, 5)]
    tr.valid_max_rows_per_call = 400                       # padded token rows at 32 landmarks: 96, 352, 32, 1056, 32
    assert tr.group_valid_bags(lens, 4) == [(0, 1), (1, 3), (3, 4), (4, 5)]


class _Stub:
    """The least `_validate_ragged` asks of a trainer."""

    def __init__(self):
        self.calls = []

    def predict_ragged(self, bags, coords=None):
        self.calls.append([int(b.shape[0]) for b in bags])
        return torch.zeros(len(bags), 2)

    def predict(self, bags, coords=None):
        raise AssertionError("one-bag batches go through predict_ragged")


class _StubWithLimit(_Stub):
    def max_shared_tiles(self):
        return 1234


class _StubWithHook(_StubWithLimit):
    def __init__(self):
        super().__init__()
        self.hook_calls = []

    def group_valid_bags(self, lengths, per_call):
        self.hook_calls.append((list(lengths), per_call))
        return [(0, 1), (1, len(lengths))]


def test_validate_ragged_uses_the_hook_and_defaults_to_group_bags(monkeypatch):
    lens = [5, 9, 3, 11, 2]
    batches = lambda: [(torch.zeros(1, t, 4), None, None, torch.tensor([[1.0, 0.0]])) for t in lens]  # noqa: E731
    seen = []
    real = mil_core.group_bags

    def recorder(*a, **kw):
        seen.append((a, kw))
        return real(*a, **kw)

    monkeypatch.setattr(mil_core, "group_bags", recorder)
    cpu = torch.device("cpu")
    # no hook: exactly today's call -- the lengths, per_call, no row limit, the trainer's shared-tile limit (or MAX_SOLO_TILES without one)
    for stub, limit in ((_Stub(), mil_core.MAX_SOLO_TILES), (_StubWithLimit(), 1234)):
        seen.clear()
        vtot, vcnt = mil_train._validate_ragged(stub, batches, cpu, None, None, 3)
        assert seen == [(([5, 9, 3], 3, 1 << 62, limit), {}), (([11, 2], 3, 1 << 62, limit), {})]
        assert stub.calls == [[5, 9, 3], [11, 2]] and vcnt == 5 and abs(vtot - 5 * 0.6931471805599453) < 1e-5
    # with the hook: the hook's groups, and group_bags is not asked
    seen.clear()
    stub = _StubWithHook()
    vtot, vcnt = mil_train._validate_ragged(stub, batches, cpu, None, None, 3)
    assert seen == [] and stub.hook_calls == [([5, 9, 3], 3), ([11, 2], 3)]
    assert stub.calls == [[5], [9, 3], [11], [2]] and vcnt == 5


def test_unpack_entry_is_declared_bound_and_exported():
    from pathlib import Path
    header = (Path(__file__).resolve().parent.parent / "include" / "amdstamp.h").read_text()
    assert "int amds_ppeg_grads_unpack(const float* corr, int C, float* w7, float* w5, float* w3, float* b7, float* b5, float* b3, void* stream);" in header
    res, args = _lib.PROTOTYPES["amds_ppeg_grads_unpack"]
    assert res is ctypes.c_int and len(args) == 9 and args[1] is ctypes.c_int
    assert hasattr(_lib.lib(), "amds_ppeg_grads_unpack")
