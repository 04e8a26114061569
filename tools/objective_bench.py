"""What `objective="library"` (amds_objective_step / amds_objective_rows) changes on the legs of profiles/mlp_train_bench.txt, at F = 768: the MLP head, batch
64, hidden 512, C = 2, 2 layers, dropout 0.25, 1 000 resident entries.  Writes <out>/objective_bench.txt (default out: profiles/).

Three routes: a checkout of the PARENT commit with its own built library (--parent DIR), this tree with objective="torch", this tree with
objective="library".  Each route runs in a process of its own that imports `stamp_amd` from its tree; three interleaved rounds (parent, torch, library;
again; again), per leg the median of the calls of a round timed by the host clock around call + synchronise, then the median and the spread [min .. max] of
the three rounds.  Legs: one training step; a training epoch of 1 000 as the bare step loop and as `fit` runs it (with its loss read-outs); the validation of
1 000 as `fit`'s batch-1 loop and as one call (valid_bags_per_call=1000).

    python tools/objective_bench.py --parent DIR [--out DIR] [--reps N]
    python tools/objective_bench.py --profile-call library|torch [--steps 20]      (for `rocprofv3 --kernel-trace --stats -- python ...`)
    python tools/objective_bench.py --kernel-stats DIR [--steps 20]                 (launches per step from the csv such a run left)"""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
F, BATCH, HIDDEN, CLASSES, ENTRIES = 768, 64, 512, 2, 1000
ROUTES = ("parent", "torch", "library")
LEGS = ("step", "train epoch of 1000, step loop", "train epoch of 1000, fit", "validation of 1000, batch-1 loop", "validation of 1000, one call")


def worker(route: str, tree: str, files_dir: str, reps: int, profile_steps: int = 0) -> None:
    """One route in this process: `stamp_amd` from `tree`; prints {leg: median seconds} as one JSON line."""
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from stamp_amd import h5io
    from stamp_amd.bags import PatientData
    from stamp_amd.cohort import ResidentFeatureTable
    from stamp_amd.mil import MLP
    from stamp_amd.mil_train import fit
    from stamp_amd.mlp_train import HipMlpTrainer
    kw = {} if route == "parent" else {"objective": route}

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    torch.manual_seed(1)
    tr = HipMlpTrainer(MLP(dim_input=F, dim_hidden=HIDDEN, dim_output=CLASSES, num_layers=2, dropout=0.25), device="cuda", max_lr=1e-4, total_steps=1000)
    x = torch.randn(BATCH, F).cuda()
    y = torch.nn.functional.one_hot(torch.arange(BATCH) % CLASSES, CLASSES).float().cuda()
    if profile_steps:
        for _ in range(profile_steps + 1):
            tr.step(x, y, **kw)
        torch.cuda.synchronize()
        return
    files = sorted(Path(files_dir).glob("*.h5"))
    if not files:
        rng = np.random.default_rng(2)
        for i in range(ENTRIES):
            p = Path(files_dir) / f"f{i:04d}.h5"
            h5io.write_slide_features(p, rng.standard_normal(F).astype(np.float16), encoder="bench", precision="fp16", code_hash="0", stamp_version="2.5.0")
            files.append(p)
    table = ResidentFeatureTable([PatientData(ground_truth="a" if i % 2 else "b", feature_files=[f]) for i, f in enumerate(files)], task="classification",
                                 device="cuda")
    train, valid = table.train_batches(BATCH), table.valid_batches()
    empty = lambda: ()  # noqa: E731

    def step_loop():
        for bags, _c, _s, targets in train():
            tr.step(bags, targets, **kw)

    work = {LEGS[0]: (lambda: tr.step(x, y, **kw), reps), LEGS[1]: (step_loop, 5), LEGS[2]: (lambda: fit(tr, train, empty, max_epochs=1, **kw), 5),
            LEGS[3]: (lambda: fit(tr, empty, valid, max_epochs=1, **kw), 3),
            LEGS[4]: (lambda: fit(tr, empty, valid, max_epochs=1, valid_bags_per_call=ENTRIES, **kw), 3)}
    print("RESULT " + json.dumps({k: timed(fn, n) for k, (fn, n) in work.items()}), flush=True)


def bench(args) -> None:
    trees = {"parent": str(Path(args.parent).resolve()), "torch": str(HERE), "library": str(HERE)}
    rounds = {r: {k: [] for k in LEGS} for r in ROUTES}
    with tempfile.TemporaryDirectory() as d:
        for _ in range(3):
            for r in ROUTES:
                out = subprocess.run([sys.executable, __file__, "--worker", r, "--tree", trees[r], "--files", d, "--reps", str(args.reps)], check=True,
                                     capture_output=True, text=True, timeout=300).stdout
                res = json.loads(next(l for l in out.splitlines() if l.startswith("RESULT "))[7:])
                for k in LEGS:
                    rounds[r][k].append(res[k])
    med = {r: {k: statistics.median(v) for k, v in rounds[r].items()} for r in ROUTES}
    spread = {r: {k: max(v) - min(v) for k, v in rounds[r].items()} for r in ROUTES}
    lines = [f"MLP head at F = {F}, batch {BATCH}, hidden {HIDDEN}, C = {CLASSES}, 2 layers, dropout 0.25, {ENTRIES} resident entries; one process per route, three "
             f"interleaved rounds (parent, torch, library); per round the median of {args.reps} steps / 5 epochs / 3 validations, host clock around call + "
             "synchronise; median [min .. max] of the rounds, ms"]
    for k in LEGS:
        lines.append(k)
        for r in ROUTES:
            v = rounds[r][k]
            lines.append(f"  {r:8s} {med[r][k] * 1e3:10.3f}  [{min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f}]")
    v_par, v_lib = med["parent"][LEGS[3]], med["library"][LEGS[4]]
    v_spread = max(spread["parent"][LEGS[3]], spread["library"][LEGS[4]])
    lines.append(f"validation of 1000: library one call {v_lib * 1e3:.3f} ms against the parent's batch-1 loop {v_par * 1e3:.3f} ms: {v_par / v_lib:.2f} x faster; "
                 f"difference {(v_par - v_lib) * 1e3:.3f} ms, larger spread {v_spread * 1e3:.3f} ms -> {'holds' if v_par - v_lib > v_spread else 'DOES NOT HOLD'}")
    for k in (LEGS[1], LEGS[2]):
        t_par, t_lib = med["parent"][k], med["library"][k]
        t_spread = max(spread["parent"][k], spread["library"][k])
        lines.append(f"{k}: library {t_lib * 1e3:.3f} ms against the parent's {t_par * 1e3:.3f} ms: ratio {t_lib / t_par:.3f}; "
                     f"larger spread {t_spread * 1e3:.3f} ms -> {'not slower' if t_lib - t_par <= t_spread else 'SLOWER'}")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "objective_bench.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


def kernel_stats(dirs, steps: int) -> None:
    """Launches per step from what a `rocprofv3 --kernel-trace --stats` run left under each DIR: its `*_results.db` (the `kernels` view), or the
    `*kernel_stats.csv` of a run with --output-format csv (tools/mlp_train_only.py reads those)."""
    import sqlite3
    for d in dirs:
        dbs = sorted(Path(d).rglob("*_results.db"))
        if not dbs:
            sys.path.insert(0, str(HERE / "tools"))
            from mlp_train_only import kernel_stats as csv_stats
            csv_stats([d], steps)
            continue
        for f in dbs:
            print(f"{d}: kernels of one step ({f.name}; calls / {steps + 1}, in order of first launch)")
            rows = list(sqlite3.connect(f).execute("select name, count(*) from kernels group by name order by min(start)"))
            for name, calls in rows:
                print(f"  {calls / (steps + 1):6.2f}  {name[:110]}")
            print(f"  {sum(c for _, c in rows) / (steps + 1):6.2f}  launches per step")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(HERE / "profiles"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--parent")
    ap.add_argument("--worker", choices=ROUTES)
    ap.add_argument("--tree", default=str(HERE))
    ap.add_argument("--files")
    ap.add_argument("--profile-call", choices=["torch", "library"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-stats", nargs="+")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, args.steps)
    if args.profile_call:
        return worker(args.profile_call, str(HERE), "", args.reps, profile_steps=args.steps)
    if args.worker:
        return worker(args.worker, args.tree, args.files, args.reps)
    if not args.parent:
        ap.error("--parent DIR: a checkout of the parent commit with its library built")
    bench(args)


if __name__ == "__main__":
    main()
