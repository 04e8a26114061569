"""Host side of dynamic loss scaling: the C ABI's state layout as the Python wrappers address it, and `fit` recording the steps the
trainer skipped per epoch (warned through `log`)."""
import re
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent


def test_state_words_follow_the_header():
    """train_ops addresses amds_loss_scale_state as int32 words: the field order of include/amdstamp.h, 48 bytes."""
    from stamp_amd import train_ops as T

    header = (ROOT / "include" / "amdstamp.h").read_text()
    body = re.search(r"typedef struct amds_loss_scale_state \{(.*?)\} amds_loss_scale_state;", header, re.S).group(1)
    fields = re.findall(r"^\s*(?:float|int32_t)\s+(\w+);", body, re.M)
    assert len(fields) == T.LS_WORDS
    for name, idx in (("scale", T.LS_SCALE), ("inv_scale", T.LS_INV_SCALE), ("nonfinite", T.LS_NONFINITE), ("last_nonfinite", T.LS_LAST_NONFINITE),
                      ("clean_steps", T.LS_CLEAN_STEPS), ("skipped", T.LS_SKIPPED), ("growth_interval", T.LS_GROWTH_INTERVAL)):
        assert fields[idx] == name, (name, fields)


def test_fit_records_skipped_steps_per_epoch_and_warns():
    from stamp_amd import mil_train

    skips_per_epoch = [0, 2, 0, 1]

    class Stub:
        dev = torch.device("cpu")
        current_loss_scale = 256.0

        def __init__(self):
            self.P = torch.zeros(1)
            self.epoch = -1
            self.skipped_steps = 0

        def epoch_end(self):
            pass

        def _refresh(self):
            pass

        def step(self, bags, targets, cw, coords=None, loss_fn=None):
            if self.step_in_epoch < skips_per_epoch[self.epoch]:
                self.skipped_steps += 1
            self.step_in_epoch += 1
            return torch.tensor(0.5), None

        def predict(self, bags, coords=None):
            return torch.tensor([[1.0 - 0.1 * self.epoch]])

        def sync_to_model(self):
            pass

    st = Stub()

    def train_batches():
        st.epoch += 1
        st.step_in_epoch = 0
        return [(torch.zeros(2, 1, 1), None, None, torch.zeros(2, 1))] * 3

    lines = []
    hist = mil_train.fit(st, train_batches, lambda: [(torch.zeros(1, 1, 1), None, None, torch.zeros(1, 1))], max_epochs=4,
                         loss_fn=lambda lg, t: lg.sum(), log=lines.append)
    assert hist["skipped_steps"] == skips_per_epoch
    warnings = [s for s in lines if s.startswith("warning")]
    assert len(warnings) == 2
    assert "epoch 1: 2 of 3 optimiser steps skipped" in warnings[0] and "loss scale now 256" in warnings[0]
    assert "epoch 3: 1 of 3" in warnings[1]
