#!/usr/bin/env python3
"""Times ONE amds_survival_groups call that holds every bootstrap resample of a survival report (stamp_amd.metrics.survival_groups with idx: 1000 resamples,
each with the log-rank sums, two Kaplan-Meier curves on a 256-point grid, the at-risk table and the medians) at n = 1 000 and n = 10 000 items, and beside
it a numpy loop over the same resamples on the CPU (per resample: a sort by time, the risk sets by cumulative sums, the log-rank sums, two cumulative
products and a searchsorted onto the grid -- lifelines, which the reference uses, is not installed).  Needs a GPU; writes
profiles/survival_stats_bench.txt.

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


def numpy_resample(s, t, e, cut, grid):
    """chi2 and the two curves on the grid for one resample, vectorised numpy in float64 -> (chi2, km [2, G]); NaN chi2 with an empty group."""
    order = np.argsort(t, kind="stable")
    t, e, high = t[order], e[order].astype(np.int64), (s[order] > cut).astype(np.int64)
    _, start = np.unique(t, return_index=True)
    groups = (1 - high, high)
    at_risk = [np.cumsum(g[::-1])[::-1][start] for g in groups]
    deaths = [np.add.reduceat(e * g, start) for g in groups]
    n_k, d_k = at_risk[0] + at_risk[1], deaths[0] + deaths[1]
    km = np.empty((2, len(grid)))
    upto = np.searchsorted(t[start], grid, side="right")
    for g in range(2):
        factor = np.where(deaths[g] > 0, (at_risk[g] - deaths[g]) / np.maximum(at_risk[g], 1), 1.0)
        km[g] = np.concatenate([[1.0], np.cumprod(factor)])[upto]
    if not (groups[0].any() and groups[1].any()):
        return np.nan, km
    frac = at_risk[1] / n_k
    expected = (d_k * frac).sum()
    more = n_k > 1
    var = (d_k[more] * (n_k[more] - d_k[more]) / (n_k[more] - 1) * frac[more] * (1 - frac[more])).sum()
    return ((deaths[1].sum() - expected) ** 2 / var if var > 0 else 0.0), km


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--resamples", type=int, default=1000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "survival_stats_bench.txt")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("survival_stats_bench: needs a GPU", file=sys.stderr)
        return 1
    from stamp_amd import metrics
    dev = torch.device("cuda:0")
    lines = [f"one amds_survival_groups call: {a.resamples} resamples x grid {a.grid} (log-rank sums, two Kaplan-Meier curves, at-risk table, medians), on "
             f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]})",
             "GPU: host clock around call + synchronise, median of 3 after a warm-up (min .. max); CPU: a numpy loop over the same resamples (sort, cumulative "
             f"sums and products, searchsorted; numpy {np.__version__}), once",
             f"{'n':>7} {'times':>12} {'GPU ms':>10} {'min':>9} {'max':>9} {'defined':>8} {'max |chi2 diff|':>16} {'CPU loop s':>11} {'CPU / GPU':>10}"]
    for n in a.sizes:
        for levels in (120, 0):
            rng = np.random.default_rng(n + levels)
            s = rng.random(n).astype(np.float32)
            t = rng.exponential(24.0 / (0.5 + s)).astype(np.float32)               # the score carries signal: the groups separate
            if levels:
                t = np.ceil(np.minimum(t, levels)).astype(np.float32)              # months, administratively censored: heavy ties
            e = (rng.random(n) < 0.7).astype(np.uint8)
            idx = rng.integers(0, n, (a.resamples, n)).astype(np.int32)
            grid = np.linspace(0, float(t.max()), a.grid).astype(np.float32)
            cut = float(np.median(s))
            sd, td, ed, ixd, gd = (torch.from_numpy(x).to(dev) for x in (s, t, e, idx, grid))
            times = []
            for rep in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = metrics.survival_groups(sd, td, ed, cut_off=cut, grid_times=gd, idx=ixd)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            times = times[1:]
            chi2 = metrics._chi2_p(res.observed, res.expected, res.variance)[0].cpu().numpy()
            defined = int((~np.isnan(chi2)).sum())
            gpu_ms = statistics.median(times)
            t0 = time.perf_counter()
            cpu_chi2 = np.array([numpy_resample(s[r], t[r], e[r], cut, grid)[0] for r in idx])
            cpu_s = time.perf_counter() - t0
            diff = float(np.nanmax(np.abs(cpu_chi2 - chi2))) if defined else float("nan")
            lines.append(f"{n:>7} {(f'{levels} levels' if levels else 'continuous'):>12} {gpu_ms:10.3f} {min(times):9.3f} {max(times):9.3f} {defined:>8} {diff:16.2e} "
                         f"{cpu_s:11.2f} {cpu_s * 1e3 / gpu_ms:10.0f}")
            print(lines[-1], flush=True)
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text("\n".join(lines) + "\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
