"""The barspoon training step alone: the HIP step (forward + backward + Adam) at float32_matmul_precision "high" (fp16 operands) and "medium" (bf16) against
the yardstick -- the SAME module's own torch containers trained by torch-ROCm autograd on the same card at "high": what a user has without the HIP path.

Geometry: the reference's defaults (src/stamp/modeling/models/barspoon.py:104-117: d_model 512, 8 + 8 heads, 2 + 2 layers, dim_feedforward 2048), 768-d
features, 4 targets, 64 bags of 512 tiles.  Warm-up, then timed steps between two device synchronisations.  Prints one JSON line and, with --out, writes it.

    python tools/barspoon_train_only.py --steps 20 --warmup 5 --out profiles/barspoon_train_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/barspoon_train_only.py --steps 5 --warmup 2 --only high        # the kernel table

--only high|medium|torch runs one side (for the profiler).  Cross-attention pair: their bytes (K | V read by the forward; K | V read and dK | dV written by the
backward, per decoder layer) are printed so that the kernel table's times turn into GB/s.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from stamp_amd import _lib  # noqa: E402
from stamp_amd import barspoon as bs  # noqa: E402
from stamp_amd.barspoon import EncDecTransformer  # noqa: E402
from stamp_amd.barspoon_train import HipBarspoonTrainer, multi_target_loss  # noqa: E402


def torch_forward(model: EncDecTransformer, x: torch.Tensor, pos: torch.Tensor) -> dict[str, torch.Tensor]:
    """The reference's forward (barspoon.py:164-205) on the module's own torch containers."""
    h = model.projector(x)
    if model.positional_encoding:
        d = h.shape[-1]
        a = pos.unsqueeze(-1) / 100_000 ** (torch.arange(d // 4, device=x.device).type_as(pos) / d)
        h = h + torch.cat([torch.sin(a).flatten(start_dim=-2), torch.cos(a).flatten(start_dim=-2)], dim=-1)
    h = model.transformer_encoder(h)
    t = torch.stack([model.class_tokens[bs.sanitize(k)] for k in model.target_labels]).expand(x.shape[0], -1, -1)
    t = model.transformer_decoder(tgt=t, memory=h)
    return {k: model.heads[bs.sanitize(k)](t[:, j]) for j, k in enumerate(model.target_labels)}


def timed(fn, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bags", type=int, default=64)
    ap.add_argument("--tiles", type=int, default=512)
    ap.add_argument("--features", type=int, default=768)
    ap.add_argument("--targets", type=int, default=4)
    ap.add_argument("--only", choices=["high", "medium", "torch"], default=None)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    targets_n = {f"t{j}": 2 + j for j in range(a.targets)}
    Bb, T = a.bags, a.tiles
    x = torch.randn(Bb, T, a.features, device=dev).half()
    pos = torch.rand(Bb, T, 2, device=dev) * 50000.0
    targets = {t: F.one_hot(torch.randint(0, n, (Bb,)), n).float().to(dev) for t, n in targets_n.items()}
    weights = {t: torch.ones(n, device=dev) for t, n in targets_n.items()}
    res: dict = {"workload": "barspoon_train_step", "bags": Bb, "tiles": T, "features": a.features, "targets": a.targets, "steps": a.steps, "warmup": a.warmup,
                 "device": torch.cuda.get_device_name(0)}
    before = torch.get_float32_matmul_precision()
    try:
        for prec in ("high", "medium"):
            if a.only not in (None, prec):
                continue
            torch.set_float32_matmul_precision(prec)
            torch.manual_seed(1)
            tr = HipBarspoonTrainer(EncDecTransformer(a.features, targets_n), device=dev)
            dt = timed(lambda: tr.step(x, pos, targets, weights), a.steps, a.warmup)
            res[f"hip_{prec}_step_ms"], res[f"hip_{prec}_bags_per_s"] = dt * 1e3, Bb / dt
            res[f"hip_{prec}_fp16_overflow_events"] = tr.model.fp16_overflow_events
            if "saved_arena_bytes" not in res:
                pack = bs.TrainPack(tr.model, lambda n: dict(tr.model.named_parameters())[n].detach().float(), torch.bfloat16, dev)
                res["saved_arena_bytes"] = int(_lib.lib().amds_barspoon_train_saved_bytes(C.byref(pack.cfg), Bb, T))
                res["backward_workspace_bytes"] = int(_lib.lib().amds_barspoon_train_workspace_bytes(C.byref(pack.cfg), Bb, T, 32))
                Hd = tr.model.num_decoder_heads
                kv = Bb * T * 2 * 64 * Hd * 2
                res["cross_attention_fwd_bytes_per_layer"], res["cross_attention_bwd_bytes_per_layer"] = kv, 2 * kv
            del tr
        if a.only in (None, "torch"):
            torch.set_float32_matmul_precision("high")
            torch.manual_seed(1)
            model = EncDecTransformer(a.features, targets_n).to(dev).train()
            opt = torch.optim.Adam(model.parameters(), lr=1e-4)
            xf = x.float()

            def torch_step():
                opt.zero_grad(set_to_none=True)
                loss = multi_target_loss(torch_forward(model, xf, pos), targets, weights)
                loss.backward()
                opt.step()

            dt = timed(torch_step, a.steps, a.warmup)
            res["torch_high_step_ms"], res["torch_high_bags_per_s"] = dt * 1e3, Bb / dt
    finally:
        torch.set_float32_matmul_precision(before)
    if "hip_high_bags_per_s" in res and "torch_high_bags_per_s" in res:
        res["ratio_hip_high_over_torch_high"] = res["hip_high_bags_per_s"] / res["torch_high_bags_per_s"]
        res["ratio_hip_medium_over_torch_high"] = res["hip_medium_bags_per_s"] / res["torch_high_bags_per_s"]
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
