"""One TransMIL training step in a loop, through `HipTransMilTrainer` (flat AdamW) and / or through the module + torch.optim.AdamW, for timing and rocprofv3.

    python tools/transmil_trainer_only.py --mode ab --rounds 3 --steps 10 [--out profiles/transmil_trainer_ab.txt]     interleaved rounds of both, a table
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/transmil_trainer_only.py --mode trainer --steps 5          one path alone (launches per step =
                                                                                                                        the trace's calls / (warmup + steps))
Geometry: BASELINE.json configs[2] -- 1 024 tiles x 1 024-d, dim_hidden 512, batch 64, torch's "high" (the reference's training setting, train.py:519),
Dropout live.  The module path is `tools/transmil_train_only.py`'s step: the unchanged comparison, not code under test."""
import argparse
import copy
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from stamp_amd.mil import TransMIL  # noqa: E402
from stamp_amd.transmil_train import HipTransMilTrainer  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("trainer", "module", "ab"), default="ab")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--feats", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="high")
    ap.add_argument("--out", default=None, help="write the A/B table here as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transmil_trainer_only.py measures on the GPU: none visible")
    torch.set_float32_matmul_precision(a.precision)
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = TransMIL(dim_output=2, dim_input=a.feats, dim_hidden=a.hidden)
    bags = torch.randn(a.batch, a.tiles, a.feats, device=dev)
    tg = torch.nn.functional.one_hot(torch.arange(a.batch, device=dev) % 2, 2).float()
    steps = {}
    if a.mode in ("trainer", "ab"):
        tr =HipTransMilTrainer(copy.deepcopy(model), device=dev, max_lr=1e-4, total_steps=1 << 20, sched_interval="step")
        steps["trainer"] = lambda: tr.step(bags, tg)[0]
    if a.mode in ("module", "ab"):
        tm = model.to(dev).train()
        opt = torch.optim.AdamW(tm.parameters(), lr=1e-4)

        def module_step():
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(tm(bags), tg)
            loss.backward()
            opt.step()
            return loss.detach()        # (an attached loss pins the step's arena)

        steps["module"] = module_step

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(loss)

    for fn in steps.values():
        timed(fn, a.warmup)
    ms = {k: [] for k in steps}
    for r in range(a.rounds if a.mode == "ab" else 1):
        for k, fn in steps.items():          # interleaved: each round times every path once, one after the other
            t, loss = timed(fn, a.steps)
            ms[k].append(t)
            print(f"round {r} {k:8s} {t:8.2f} ms/step  {a.batch / t * 1e3:8.0f} bags/s  loss {loss:.4f}", flush=True)
    lines = [f"TransMIL training step, batch {a.batch} x {a.tiles} tiles x {a.feats}-d, dim_hidden {a.hidden}, \"{a.precision}\", Dropout live; "
             f"{a.steps} steps per round after {a.warmup} warm-up steps, rounds interleaved",
             f"{'path':34s} {'ms/step (median)':>17s} {'bags/s':>8s} {'rounds (ms/step)':>30s} {'spread':>8s}"]
    names = {"trainer": "HipTransMilTrainer (flat AdamW)", "module": "module + torch.optim.AdamW"}
    for k, v in ms.items():
        med = statistics.median(v)
        lines.append(f"{names[k]:34s} {med:17.2f} {a.batch / med * 1e3:8.0f} {' '.join(f'{x:.2f}' for x in v):>30s} {max(v) - min(v):8.2f}")
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
