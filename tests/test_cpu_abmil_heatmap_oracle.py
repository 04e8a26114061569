"""tests/abmil_heatmap_oracle.py: the closed form of the gated-attention head's Grad-CAM against autograd in fp64; both against what the reference's own
heat-map functions returned on its CHIEFModel (tests/golden/abmil_heatmap_xs.npz, made by tools/make_golden.py::golden_abmil_heatmap); and the host-only parts
of the heat-map route (method selection, the workspace size entry, the module's refusals).  No GPU."""
import ctypes as C
import dataclasses
from pathlib import Path

import numpy as np
import pytest
import torch

import abmil_heatmap_oracle as H
import abmil_oracle as O

GOLD = Path(__file__).resolve().parent / "golden"
RTOL, ATOL = 1e-5, 1e-6          # test_cpu_abmil_oracle.py's
LENGTHS = [1, 2, 17, 65, 257, 5]


@pytest.mark.parametrize("dims", [(48, 64, 32, 3), (384, 256, 256, 2), (48, 64, 32, 1), (40, 72, 24, 5)], ids=lambda d: "/".join(map(str, d)))
def test_closed_form_equals_autograd_in_fp64(dims):
    """Bar 1e-12 of the largest value: fp64 rounding through sums of up to 384 terms (2^-53 x a few hundred), nothing else -- the two are the same function."""
    F, L, D, Cc = dims
    w = O.random_weights(F, L, D, Cc, seed=21)
    x = torch.randn(sum(LENGTHS), F, generator=torch.Generator().manual_seed(22)) * 0.7
    ref = H.cam_autograd(x, LENGTHS, w, torch.float64)
    got = H.closed_form(x, LENGTHS, w, torch.float64)
    fwd = O.forward(x, LENGTHS, w, dtype=torch.float64)
    err = float((got["cam_raw"] - ref).abs().max() / ref.abs().max())
    print(f"abmil heatmap closed form {dims}: max difference / max value {err:.3e}")
    assert ref.shape == (Cc, sum(LENGTHS)) and float(ref.abs().max()) > 0 and err < 1e-12
    assert all(float(c.abs().max()) > 0 for c in ref) and (Cc == 1 or float((ref[0] - ref[1]).abs().max()) > 1e-3 * float(ref.abs().max()))
    # the bag term: sum_k P_k g_kc is the logit without its bias
    assert float((got["gbar"] + w[O.CLS_B].double() - fwd["logits"]).abs().max()) < 1e-13
    assert torch.equal(got["probs"], fwd["probs"]) and float((got["logits"] - fwd["logits"]).abs().max()) < 1e-13
    # a row's logits as a bag of its own: W_cls h_n + b_cls
    h = torch.relu(x.double() @ w[O.FC_W].double().T + w[O.FC_B].double())
    assert float((H.tile_logits(x, w, torch.float64) - (h @ w[O.CLS_W].double().T + w[O.CLS_B].double())).abs().max()) < 1e-13


def _fixture():
    fx, base, hm = np.load(GOLD / "abmil_xs.npz"), np.load(GOLD / "chief_gated_attention_xs.npz"), np.load(GOLD / "abmil_heatmap_xs.npz")
    w = {k: torch.from_numpy(base["w:" + k]) for k in O.KEYS if k.startswith("attention_net.")}
    w.update({k: torch.from_numpy(fx["w:" + k]) for k in O.KEYS if k.startswith("classifiers.")})
    return torch.from_numpy(fx["x"]).float(), [int(n) for n in fx["lengths"]], w, hm


def test_oracle_equals_the_references_own_heatmap_functions():
    x, lengths, w, hm = _fixture()
    assert lengths == [77, 40] == [int(n) for n in hm["lengths"]]
    raw_ref = np.concatenate([hm["cam_raw_77"], hm["cam_raw_40"]]).T          # [C, rows]
    assert raw_ref.shape == (2, 117) and raw_ref.max() > 100 * ATOL             # (the tolerance's absolute part is not what passes)
    for name, got in (("autograd fp32", H.cam_autograd(x, lengths, w, torch.float32)), ("closed form fp32", H.closed_form(x, lengths, w, torch.float32)["cam_raw"]),
                      ("closed form fp64", H.closed_form(x, lengths, w, torch.float64)["cam_raw"])):
        np.testing.assert_allclose(got.numpy(), raw_ref, rtol=RTOL, atol=ATOL, err_msg=name)
        for cam, n in zip(got.split(lengths, dim=1), lengths):                  # the softmax over the tiles of one slide (:55-56)
            np.testing.assert_allclose(torch.softmax(cam.float(), dim=1).T.numpy(), hm[f"cam_{n}"], rtol=RTOL, atol=ATOL, err_msg=name)
    np.testing.assert_allclose(H.tile_logits(x, w, torch.float32).numpy(), hm["tile_logits"], rtol=RTOL, atol=ATOL)


def test_method_selection_routes_the_gated_attention_head():
    from stamp_amd import heatmaps
    from stamp_amd.abmil import GatedAttentionMIL

    m = GatedAttentionMIL(48, 64, 32, 3)
    assert heatmaps._pick(m, "auto") == "library" and heatmaps._pick(m, "library") == "library" and heatmaps._pick(m, "jacrev") == "jacrev"
    with pytest.raises(ValueError, match="fused"):
        heatmaps._pick(m, "fused")
    with pytest.raises(ValueError, match="GatedAttentionMIL"):
        heatmaps._pick(torch.nn.Linear(4, 2), "library")
    assert heatmaps._pick(torch.nn.Linear(4, 2), "auto") == "jacrev"
    fields = [f.name for f in dataclasses.fields(heatmaps.SlideHeatmap)]
    assert fields[-1] == "tile_attention" and heatmaps.SlideHeatmap("regression", None, None, None, None).tile_attention is None
    # eval + no_grad only, no CPU fallback; refused on the host
    with pytest.raises(RuntimeError, match="eval mode"):
        m.heatmap_scores(torch.zeros(3, 48))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.eval().heatmap_scores(torch.zeros(3, 48))
        with pytest.raises(ValueError, match="features"):
            m.heatmap_scores([torch.zeros(3, 48), torch.zeros(3, 47)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        heatmaps.gradcam(m, torch.zeros(3, 48))


def test_workspace_entry_refuses_bad_configs_and_grows_with_the_rows():
    from stamp_amd import _lib
    from stamp_amd.abmil import CHIEF_SIZES

    lib = _lib.lib()
    size = lambda dims, bags, rows: lib.amds_abmil_heatmap_workspace_bytes(C.byref(_lib.AbmilCfg(*dims)), bags, rows)  # noqa: E731
    for dims, bags, rows, rule in (((0, 64, 32, 2), 1, 10, "every width must be >= 1"), ((48, 64, 40000, 2), 1, 10, "D <= 32768"), ((48, 64, 32, 2), 0, 10, "1 <= bags"),
                                   ((48, 64, 32, 2), 5, 4, "every bag holds at least one row"), ((48, 64, 32, 2), 1, 65535 * 64, "at most 65535 * 64 - 256 rows")):
        assert size(dims, bags, rows) == 0 and rule in lib.amds_last_error().decode() and "amds_abmil_heatmap_workspace_bytes" in lib.amds_last_error().decode()
    assert lib.amds_abmil_heatmap_workspace_bytes(None, 1, 1) == 0 and "null config" in lib.amds_last_error().decode()
    for (F, L, D) in list(CHIEF_SIZES.values()) + [(48, 64, 32), (40, 72, 24)]:
        cfg = _lib.AbmilCfg(F, L, D, 2)
        sizes = [size((F, L, D, 2), 1, rows) for rows in (1, 256, 257, 4200, 65536)]
        assert sizes[0] <= sizes[1] and all(a < b for a, b in zip(sizes[1:], sizes[2:])) and all(s % 256 == 0 for s in sizes)
        for rows, s in zip((1, 257, 65536), (sizes[0], sizes[2], sizes[4])):
            rows_p = -(-rows // 256) * 256
            ev = lib.amds_abmil_workspace_bytes(C.byref(cfg), 1, rows)
            # the eval forward's workspace plus r [rows_p][L] and an int per row: nothing rows x F beyond the staged rows, nothing per class
            assert ev < s <= ev + rows_p * L * 4 + rows * 4 + 2 * 255
        assert size((F, L, D, 2), 1, 4200) == size((F, L, D, 1000), 1, 4200)
