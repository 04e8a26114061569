"""tests/abmil_oracle.py against the reference's own CHIEFModel (tests/golden/abmil_xs.npz, made by tools/make_golden.py::golden_abmil), the module's
parameter tree, and the host-only parts of the library's gated-attention MIL entries (sizes, refusals, grouping).  No GPU."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import abmil_oracle as O

GOLD = Path(__file__).resolve().parent / "golden"
RTOL, ATOL = 1e-5, 1e-6          # test_chief_gated_attention's


def _fixture():
    fx = np.load(GOLD / "abmil_xs.npz")
    base = np.load(GOLD / "chief_gated_attention_xs.npz")
    w = {k: torch.from_numpy(base["w:" + k]) for k in O.KEYS if k.startswith("attention_net.")}
    w.update({k: torch.from_numpy(fx["w:" + k]) for k in O.KEYS if k.startswith("classifiers.")})
    return fx, w


def test_oracle_fp32_equals_the_reference_values_and_gradients():
    fx, w = _fixture()
    x = torch.from_numpy(fx["x"]).float()
    lengths = [int(n) for n in fx["lengths"]]
    assert lengths == [77, 40]
    res = O.gradients(x, lengths, w, loss_fn=lambda lg: torch.nn.functional.cross_entropy(lg, torch.tensor([0, 1])))
    for name, key in (("attn_raw", "attention_raw"), ("pooled", "WSI_feature_transformed"), ("logits", "logits")):
        np.testing.assert_allclose(res[name].numpy(), fx[key], rtol=RTOL, atol=ATOL, err_msg=name)
    for k in O.KEYS:
        np.testing.assert_allclose(res["g:" + k].numpy(), fx["g:" + k], rtol=RTOL, atol=ATOL, err_msg=k)


def test_oracle_masks_of_ones_change_nothing_and_fp64_agrees():
    fx, w = _fixture()
    x = torch.from_numpy(fx["x"]).float()[:30]
    ones = (torch.ones(30, 256), torch.ones(30, 256), torch.ones(30, 256))
    a, b = O.forward(x, [13, 17], w), O.forward(x, [13, 17], w, masks=ones)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = O.forward(x, [13, 17], w, dtype=torch.float64)
    assert O.rel_err(a["logits"], c["logits"]) < 1e-5 and c["logits"].dtype == torch.float64
    assert torch.allclose(c["probs"][:13].sum(), torch.tensor(1.0, dtype=torch.float64))


def test_state_dict_keys_equal_the_fixtures():
    from stamp_amd.abmil import CHIEF_SIZES, KEYS, GatedAttentionMIL

    fx, _ = _fixture()
    want = {k[2:] for k in fx.files if k.startswith("g:")}
    assert want == set(O.KEYS) == set(KEYS.values())
    m = GatedAttentionMIL(*CHIEF_SIZES["xs"], 2)
    assert list(m.state_dict().keys()) == list(O.KEYS)
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == fx["g:" + k].shape, k


def test_from_chief_loads_attention_net_and_keeps_fitting_classifiers():
    from stamp_amd.abmil import GatedAttentionMIL

    fx, w = _fixture()
    sd = dict(w)
    sd["instance_classifiers.0.weight"] = torch.zeros(2, 256)          # ignored
    m = GatedAttentionMIL.from_chief("xs", sd, dim_output=2)
    assert all(torch.equal(m.state_dict()[k], w[k]) for k in O.KEYS)
    m3 = GatedAttentionMIL.from_chief("xs", sd, dim_output=3)            # classifiers [2, 256] does not fit [3, 256]: stays fresh
    assert m3.state_dict()["classifiers.weight"].shape == (3, 256)
    assert all(torch.equal(m3.state_dict()[k], w[k]) for k in O.KEYS if k.startswith("attention_net."))
    with pytest.raises(ValueError):
        GatedAttentionMIL.from_chief("small", sd)
    with pytest.raises(KeyError):
        GatedAttentionMIL.from_chief("xs", {k: v for k, v in sd.items() if "attention_c" not in k})
    with pytest.raises(ValueError, match="mask"):
        m(torch.zeros(1, 3, 384), mask=torch.ones(1, 3, dtype=torch.bool))


def _sizes(lib, dims, bags, rows):
    from stamp_amd import _lib

    cfg = _lib.AbmilCfg(*dims)
    return [fn(C.byref(cfg), bags, rows) for fn in (lib.amds_abmil_workspace_bytes, lib.amds_abmil_train_saved_bytes, lib.amds_abmil_train_workspace_bytes)]


def test_bytes_entries_accept_chiefs_geometries_and_bound_the_saved_state():
    from stamp_amd import _lib
    from stamp_amd.abmil import CHIEF_SIZES

    lib = _lib.lib()
    pad = lib.amds_abmil_row_pad()
    assert pad == 256
    for (F, L, D) in list(CHIEF_SIZES.values()) + [(48, 64, 32)]:
        for bags, rows in ((1, 1), (9, 500), (64, 65536)):
            ws, saved, tws = _sizes(lib, (F, L, D, 2), bags, rows)
            assert ws > 0 and saved > 0 and tws > 0
            rows_p = -(-rows // pad) * pad
            # (L + 2 D + 2) * 4 bytes per (padded) row + L * 4 per bag, five regions rounded up to 256 bytes; nothing rows x F
            assert saved <= (L + 2 * D + 2) * 4 * rows_p + bags * L * 4 + 5 * 255
            assert saved % 256 == 0 and ws % 256 == 0 and tws % 256 == 0


@pytest.mark.parametrize("dims,bags,rows,rule", [
    ((0, 64, 32, 2), 1, 10, "every width must be >= 1"),
    ((48, 64, 0, 2), 1, 10, "every width must be >= 1"),
    ((48, 64, 32, -1), 1, 10, "every width must be >= 1"),
    ((48, 64, 40000, 2), 1, 10, "D <= 32768"),
    ((65536, 65536, 32, 2), 1, 10, "at most 2^30 elements"),
    ((48, 64, 32, 2), 0, 10, "1 <= bags"),
    ((48, 64, 32, 2), 5, 4, "every bag holds at least one row"),
    ((48, 64, 32, 2), 1, 65535 * 64, "at most 65535 * 64 - 256 rows"),
])
def test_bytes_entries_refuse_and_name_the_rule(dims, bags, rows, rule):
    from stamp_amd import _lib

    lib = _lib.lib()
    assert _sizes(lib, dims, bags, rows) == [0, 0, 0]
    assert rule in lib.amds_last_error().decode()
    assert lib.amds_abmil_workspace_bytes(None, 1, 1) == 0 and "null config" in lib.amds_last_error().decode()


def test_grouping_is_mil_cores_without_a_class_row():
    from stamp_amd import abmil, mil_core

    lengths = [5, 7, 300, 2, 2, 40000, 9]
    assert abmil.group_bags(lengths, 3, 1 << 40) == mil_core.group_bags(lengths, 3, abmil.MAX_ROWS_PER_CALL, mil_core.MAX_SOLO_TILES, 0)
    assert abmil.group_bags([4, 4, 4], 8, 8) == [(0, 2), (2, 3)]            # 8 rows fit exactly: no extra row per bag
    assert mil_core.group_bags([4, 4, 4], 8, 8) == [(0, 1), (1, 2), (2, 3)]  # (the `vit` head's class token would not)
    assert abmil.group_bags(lengths, 100)[-1][1] == len(lengths)
    t = abmil.HipAbmilTrainer(abmil.GatedAttentionMIL(48, 64, 32, 3), device="cpu")
    assert t.group_valid_bags([4, 4, 4], 2) == [(0, 2), (2, 3)] and t.max_shared_tiles() == mil_core.MAX_SOLO_TILES
    assert t.P.numel() == sum(v.numel() for v in t.model.state_dict().values()) and t.current_loss_scale == 1.0
