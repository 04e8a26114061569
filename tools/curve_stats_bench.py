#!/usr/bin/env python3
"""Times ONE amds_binary_curves call that holds every bootstrap resample of a classifier's ROC and precision-recall curves (stamp_amd.metrics.binary_curves
with idx: 1000 resamples x a 1000-point grid, ROC + PR) at n = 1 000 and n = 10 000 validation items, with 8 score levels (heavy ties) and with continuous
scores, and -- where sklearn imports -- the same resamples through the reference's loop on the CPU (roc_curve / precision_recall_curve + np.interp per
resample, src/stamp/statistics/roc.py:188-197, prc.py:49-63).  Needs a GPU; writes profiles/curve_stats_bench.txt.

GPU times: a host clock around the call and a device synchronise, median of three after one warm-up call.  The CPU loop is timed once.  No ratio is a
requirement of anything; the file records what was measured."""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def reference_loop(y, s, idx, grid):
    from sklearn.metrics import auc, precision_recall_curve, roc_auc_score, roc_curve
    x = np.linspace(0, 1, grid)
    used = 0
    for r in idx:
        ys, ss = y[r], s[r]
        if len(np.unique(ys)) != 2:
            continue
        fpr, tpr, _ = roc_curve(ys, ss)
        np.interp(x, fpr, tpr)
        roc_auc_score(ys, ss)
        precision, recall, _ = precision_recall_curve(ys, ss)
        auc(x, np.interp(x, recall[::-1], precision[::-1]))
        used += 1
    return used


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--resamples", type=int, default=1000)
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "curve_stats_bench.txt")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("curve_stats_bench: needs a GPU", file=sys.stderr)
        return 1
    from stamp_amd import metrics
    try:
        import sklearn
        sk = sklearn.__version__
    except ImportError:
        sk = None
    dev = torch.device("cuda:0")
    lines = [f"one amds_binary_curves call: {a.resamples} resamples x grid {a.grid}, ROC + PR, on {torch.cuda.get_device_name(0)} "
             f"({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]})",
             "GPU: host clock around call + synchronise, median of 3 after a warm-up (min .. max); CPU: the reference's sklearn + np.interp loop over the "
             "same resamples, once" + (f" (sklearn {sk}, numpy {np.__version__})" if sk else " -- sklearn not installed: not measured"),
             f"{'n':>7} {'scores':>12} {'GPU ms':>10} {'min':>9} {'max':>9} {'defined':>8} {'CPU loop s':>11} {'CPU / GPU':>10}"]
    for n in a.sizes:
        for levels in (8, 0):
            rng = np.random.default_rng(n + levels)
            s = (rng.integers(0, levels, n) / levels if levels else rng.random(n)).astype(np.float32)
            y = rng.random(n) < np.clip(0.15 + 0.5 * s, 0, 1)                     # the score carries signal: curves away from the diagonal
            idx = rng.integers(0, n, (a.resamples, n)).astype(np.int32)
            sd, yd, ixd = torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(idx).to(dev)
            times = []
            for rep in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = metrics.binary_curves(sd, yd, idx=ixd, grid=a.grid)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            times = times[1:]
            defined = int((~res.ap.isnan()).sum())
            gpu_ms = statistics.median(times)
            cpu = ""
            ratio = ""
            if sk:
                t0 = time.perf_counter()
                used = reference_loop(y, s, idx, a.grid)
                cpu_s = time.perf_counter() - t0
                assert used == defined, (used, defined)
                cpu, ratio = f"{cpu_s:11.2f}", f"{cpu_s * 1e3 / gpu_ms:10.0f}"
            lines.append(f"{n:>7} {('8 levels' if levels else 'continuous'):>12} {gpu_ms:10.3f} {min(times):9.3f} {max(times):9.3f} {defined:>8} {cpu:>11} {ratio:>10}")
            print(lines[-1], flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text("\n".join(lines) + "\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
