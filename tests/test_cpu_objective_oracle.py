"""tests/objective_oracle.py (the fp64 restatement the GPU test judges amds_objective_step / amds_objective_rows by) against `stamp_amd.losses` under
autograd in fp64 and against the recorded answers of the reference's own functions; the C ABI's declarations and exports; the host-side argument rules of
`FlatTrainer.step(objective=)` and `mil_train.fit(objective=)`."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import objective_cases as OC
import objective_oracle as O

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"


torch_loss = OC.torch_loss
CASES = OC.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_the_torch_losses_in_fp64(name):
    kind, x, y, w = CASES[name]
    loss, grad, has_grad = O.step(kind, x.numpy(), y.numpy(), None if w is None else w.numpy())
    ref, g = torch_loss(kind, x, y, w)
    assert np.isfinite(loss) and np.isfinite(grad).all()
    assert abs(loss - float(ref)) <= 1e-12 * max(abs(float(ref)), 1.0), (loss, float(ref))
    no_event = kind in (O.COX_EFRON, O.COX_BRESLOW) and float(y[:, 1].sum()) == 0
    assert has_grad == (0 if no_event else 1)
    if no_event:
        assert loss == 0.0 and not grad.any() and (g is None or not g.any())
        return
    gn = g.numpy()
    assert np.linalg.norm(grad - gn) <= 1e-12 * max(np.linalg.norm(gn), 1e-300), np.linalg.norm(grad - gn) / np.linalg.norm(gn)


def test_oracle_rows_are_one_row_batches():
    for name in ("ce-65x5-soft-w-n3", "ce-3x1024-onehot-now-pm80", "l1-65"):
        kind, x, y, w = CASES[name]
        wn = None if w is None else w.numpy()
        r = O.rows(kind, x.numpy(), y.numpy(), wn)
        for n in range(x.shape[0]):
            one = O.step(kind, x[n:n + 1].numpy(), y[n:n + 1].numpy(), wn)[0]
            assert abs(r[n] - one) <= 1e-14 * max(abs(one), 1.0)
        assert abs(r.mean() - O.step(kind, x.numpy(), y.numpy(), wn)[0]) <= 1e-12 * max(abs(r.mean()), 1.0)


def test_oracle_reproduces_the_recorded_reference_answers():
    """tests/golden/cox.npz and cox_slide.npz hold what the reference's own functions returned; the bars are those of the existing loss tests."""
    z = np.load(GOLD / "cox.npz")
    lh, tt, ev = z["log_hz"], z["time"], z["event"]
    assert abs(O.cox_efron(lh, tt, ev)[0] - float(z["efron"])) < 1e-5
    assert abs(O.cox_breslow(lh, tt, ev)[0] - float(z["breslow"])) < 1e-5
    assert abs(O.cox_efron(lh, np.arange(40.0), ev)[0] - float(z["notie"])) < 1e-5
    s = np.load(GOLD / "cox_slide.npz")
    loss, grad, _ = O.cox_breslow(s["scores"], s["times"], s["events"])
    assert abs(loss - float(s["loss"])) < 1e-6
    np.testing.assert_allclose(grad.reshape(s["grad"].shape), s["grad"], rtol=1e-5, atol=1e-8)


def test_nine_item_example_takes_the_tie_branch_with_single_event_groups():
    t, e = np.array(OC.NINE[0], float), np.array(OC.NINE[1], float)
    assert len(np.unique(t)) < len(t) and all(((t == u) & (e != 0)).sum() <= 1 for u in np.unique(t))
    lh = torch.randn(9, generator=torch.Generator().manual_seed(3)).double()
    ref, _ = torch_loss(O.COX_EFRON, lh[:, None], torch.stack([torch.from_numpy(t), torch.from_numpy(e)], 1), None)
    assert abs(O.cox_efron(lh.numpy(), t, e)[0] - float(ref)) < 1e-12


def test_header_declares_and_library_exports_the_objective_entries():
    from stamp_amd import _lib
    header = (ROOT / "include" / "amdstamp.h").read_text()
    declared = set(re.findall(r"\b(amds_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("amds_objective_step", "amds_objective_rows", "amds_objective_max_items"):
        assert name in declared, f"{name} is not declared in include/amdstamp.h"
        assert name in _lib.PROTOTYPES and hasattr(lib, name), f"{name} is not exported"
    assert lib.amds_objective_max_items() == OC.COX_LIMIT >= 4096
    # argument checks come before any launch, so they answer without a GPU
    assert lib.amds_objective_step(0, None, None, None, 1, 1, 1.0, None, None, None, None, None, None) == -1 and b"null pointer" in lib.amds_last_error()
    assert lib.amds_objective_step(7, None, None, None, 1, 1, 1.0, None, None, None, None, None, None) == -1 and b"kind=7" in lib.amds_last_error()
    assert lib.amds_objective_rows(2, None, None, None, 1, 1, None, None) == -1 and b"CE and L1" in lib.amds_last_error()
    one = 1          # any non-NULL address: the item limit is checked before anything is read
    assert lib.amds_objective_step(2, one, one, None, OC.COX_LIMIT + 1, 1, 1.0, None, one, one, one, None, None) == -1
    assert b"at most 4096" in lib.amds_last_error()


def test_wrappers_refuse_cpu_tensors():
    from stamp_amd import train_ops as T
    with pytest.raises(RuntimeError, match="GPU"):
        T.objective_step(T.OBJ_CE, torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        T.objective_rows(T.OBJ_L1, torch.zeros(2, 1), torch.zeros(2))


def test_loss_fn_selects_the_objective():
    from stamp_amd import losses, train_ops as T
    from stamp_amd.flat_trainer import check_objective, objective_kind
    assert (T.OBJ_CE, T.OBJ_L1, T.OBJ_COX_EFRON, T.OBJ_COX_BRESLOW) == (O.CE, O.L1, O.COX_EFRON, O.COX_BRESLOW)
    assert objective_kind(None) == T.OBJ_CE
    assert objective_kind(losses.l1_loss) == T.OBJ_L1
    assert objective_kind(losses.cox_survival_loss) == T.OBJ_COX_EFRON
    assert objective_kind(losses.cox_slide_survival_loss) == T.OBJ_COX_BRESLOW
    for foreign in (lambda a, b: (a - b).sum(), losses.cox_breslow_loss, torch.nn.functional.mse_loss, [1]):
        with pytest.raises(ValueError, match="l1_loss.*cox_survival_loss.*cox_slide_survival_loss"):
            objective_kind(foreign)
    assert check_objective("torch") == "torch" and check_objective("library") == "library"
    with pytest.raises(ValueError, match="objective"):
        check_objective("hip")


def test_fit_validates_objective_before_it_touches_the_trainer():
    from stamp_amd import losses
    from stamp_amd.mil_train import fit

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"fit read trainer.{name} before validating its arguments")

    none = lambda: iter(())          # noqa: E731
    with pytest.raises(ValueError, match="objective must be"):
        fit(Untouchable(), none, none, max_epochs=1, objective="kernel")
    with pytest.raises(ValueError, match="l1_loss"):
        fit(Untouchable(), none, none, max_epochs=1, objective="library", loss_fn=lambda a, b: a.sum())
    for fn in (losses.cox_survival_loss, losses.cox_slide_survival_loss):
        with pytest.raises(ValueError, match="val_cindex"):
            fit(Untouchable(), none, none, max_epochs=1, objective="library", loss_fn=fn)


def test_feature_table_valid_batches_keeps_its_iteration_and_gains_block():
    from stamp_amd.cohort import FeatureTableView, _ValidEntries
    vb = FeatureTableView.valid_batches(object.__new__(FeatureTableView))
    assert isinstance(vb, _ValidEntries) and callable(vb) and callable(vb.block)
