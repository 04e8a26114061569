#!/usr/bin/env python3
"""Times of the concordance pair counts (amds_concordance_counts through stamp_amd.metrics.concordance_counts) next to the same counts written as torch
broadcasting on the device.  One process, one GPU.  Three shapes: one validation set of 2 048 items, one of 32 768, and 1 000 bootstrap resamples of 2 000
items in one call.  Each leg: `--warmup` calls, then `--reps` calls timed one by one with HIP events; the median and the minimum are recorded.  The torch leg
builds the [P, n, n] comparison tensors the kernel never builds, so it is skipped where they do not fit into half of the free device memory.  The two legs'
counts are compared for equality on every shape.  Recorded, not gated: writes a text file (default profiles/rank_metrics_bench.txt)."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SHAPES = [(2048, 1), (32768, 1), (2000, 1000)]          # (items, problems); problems > 1 = resamples of one base problem


def torch_counts(score, time, event, idx):
    """The definition as broadcasting: [P, n, n] boolean tensors."""
    import torch
    if idx is not None:
        score, time, event = score[idx.long()], time[idx.long()], event[idx.long()]
    else:
        score, time, event = score[None], time[None], event[None]
    ev = event == 1
    perm = ev[:, :, None] & ((time[:, :, None] < time[:, None, :]) | ((time[:, :, None] == time[:, None, :]) & ~ev[:, None, :]))
    conc = (perm & (score[:, :, None] > score[:, None, :])).sum((1, 2))
    tied = (perm & (score[:, :, None] == score[:, None, :])).sum((1, 2))
    return torch.stack([conc, tied, perm.sum((1, 2)), torch.full_like(conc, score.shape[1])], 1)


def timed(fn, warmup: int, reps: int) -> list[float]:
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rank_metrics_bench.txt"))
    args = ap.parse_args()
    import torch

    from stamp_amd import metrics
    if not torch.cuda.is_available():
        print("rank_metrics_only.py needs a GPU: nothing measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    lines = [f"amds_concordance_counts vs torch broadcasting, {torch.cuda.get_device_name(0)}; per call, HIP events, ms: median (min) of {args.reps} / {args.torch_reps} calls",
             "pairs = problems x items^2 ordered pairs examined; the call with resamples ends in one 8-byte read of the out-of-range count", ""]
    g = torch.Generator().manual_seed(0)
    for n, P in SHAPES:
        score = (torch.randn(n, generator=g) * 4).round().div(4).to(dev)          # ties in every array, like rounded risk scores and follow-up months
        time = torch.randint(0, 120, (n,), generator=g).float().to(dev)
        event = (torch.rand(n, generator=g) < 0.6).to(torch.uint8).to(dev)
        idx = torch.randint(0, n, (P, n), generator=g, dtype=torch.int32).to(dev) if P > 1 else None
        got = metrics.concordance_counts(score, time, event, idx)
        k_ms = timed(lambda: metrics.concordance_counts(score, time, event, idx), args.warmup, args.reps)
        pairs = P * n * n
        line = f"n = {n:6d}  problems = {P:5d}  pairs = {pairs:.3e}   kernel {statistics.median(k_ms):9.4f} ({min(k_ms):9.4f})  {pairs / statistics.median(k_ms) / 1e6:9.1f} Gpairs/s"
        need = 10 * pairs                                                          # ~10 one-byte [P, n, n] temporaries live at the peak
        free = torch.cuda.mem_get_info(dev)[0]
        if need <= free // 2:
            want = torch_counts(score, time, event, idx)
            same = bool(torch.equal(got, want))
            del want
            t_ms = timed(lambda: torch_counts(score, time, event, idx), 1, args.torch_reps)
            line += f"   torch {statistics.median(t_ms):10.4f} ({min(t_ms):10.4f})   x{statistics.median(t_ms) / statistics.median(k_ms):7.1f}   counts equal: {same}"
        else:
            line += f"   torch: not run ([P, n, n] temporaries ~{need / 2 ** 30:.0f} GiB do not fit into half of the {free / 2 ** 30:.0f} GiB free)"
        torch.cuda.empty_cache()
        print(line, flush=True)
        lines.append(line)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
