"""The MLP head on slide- / patient-level vectors: what the one-call path costs next to the ways the same work was done before.  Writes
<out>/mlp_train_bench.txt (default out: profiles/).

Geometry: batch 64, hidden 512, C = 2, num_layers 2 (the reference's default head), F = 768 / 1 536 / 2 560; three interleaved rounds on one box, per
measurement the median of --reps calls timed by the host clock around call + synchronise, and the spread of the three rounds' medians.
  1. one training step: `HipMlpTrainer.step` (amds_mlp_train_forward / _backward + amds_adamw) against `mil.MLP` under autograd + `torch.optim.AdamW`
     (one library call per operation), same batch, dropout live in both.
  2. one epoch of `fit`'s training loop on 1 000 entries: batches gathered from a `ResidentFeatureTable` against a host loop that reads each entry's file
     per item through `h5io.read_file` (the reference's feed restated: one file per item, stacked, `.float()`, copied to the device).
  3. the validation of 1 000 entries: the batch-1 loop (one forward and one host read per entry) against `fit(valid_bags_per_call=1000)`.

    python tools/mlp_train_only.py [--out DIR] [--reps N] [--feats 768,1536,2560]
    python tools/mlp_train_only.py --profile-call trainer|module [--feats 768] [--steps 20]
    python tools/mlp_train_only.py --kernel-stats DIR [DIR ...]

--profile-call: a warm-up step, then --steps steps of one route and nothing else (for `rocprofv3 --kernel-trace --stats -- python ...`).
--kernel-stats: prints kernel names and call counts per step from the `*kernel_stats.csv` such a run left under DIR (calls divided by steps + 1 warm-up)."""
import argparse
import csv
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

BATCH, HIDDEN, CLASSES, ENTRIES = 64, 512, 2, 1000


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def make_routes(F):
    """-> {"trainer": step(), "module": step()} on one fixed batch."""
    from stamp_amd.mil import MLP
    from stamp_amd.mlp_train import HipMlpTrainer
    torch.manual_seed(1)
    kw = dict(dim_input=F, dim_hidden=HIDDEN, dim_output=CLASSES, num_layers=2, dropout=0.25)
    x = torch.randn(BATCH, F).cuda()
    y = torch.nn.functional.one_hot(torch.arange(BATCH) % CLASSES, CLASSES).float().cuda()
    tr = HipMlpTrainer(MLP(**kw), device="cuda", max_lr=1e-4, total_steps=1000)
    mod = MLP(**kw).cuda().train()
    opt = torch.optim.AdamW(mod.parameters(), lr=1e-4)

    def module_step():
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(mod(x), y).backward()
        opt.step()

    return {"trainer": lambda: tr.step(x, y), "module": module_step}


def write_files(d, F, n=ENTRIES):
    from stamp_amd import h5io
    rng = np.random.default_rng(2)
    files = []
    for i in range(n):
        p = Path(d) / f"f{F}_{i:04d}.h5"
        h5io.write_slide_features(p, rng.standard_normal(F).astype(np.float16), encoder="bench", precision="fp16", code_hash="0", stamp_version="2.5.0")
        files.append(p)
    return files


def feeds(files, F):
    """-> (resident train feed, host-loop train feed, valid feed, trainer factory) over the same 1 000 files."""
    from stamp_amd import h5io
    from stamp_amd.bags import PatientData
    from stamp_amd.cohort import ResidentFeatureTable
    from stamp_amd.mil import MLP
    from stamp_amd.mlp_train import HipMlpTrainer
    labels = ["a" if i % 2 else "b" for i in range(len(files))]
    table = ResidentFeatureTable([PatientData(ground_truth=g, feature_files=[f]) for f, g in zip(files, labels)], task="classification", device="cuda")

    def host_epoch():
        order = torch.randperm(len(files)).tolist()
        for a in range(0, len(order), BATCH):
            idx = order[a:a + BATCH]
            rows = [torch.from_numpy(np.asarray(h5io.read_file(files[i])[0]["feats"]).reshape(-1)).float() for i in idx]
            yield torch.stack(rows).cuda(), None, None, table.targets[idx].cuda()

    def trainer():
        torch.manual_seed(3)
        return HipMlpTrainer(MLP(dim_input=F, dim_hidden=HIDDEN, dim_output=CLASSES, num_layers=2, dropout=0.25), device="cuda", total_steps=1000)

    return table.train_batches(BATCH), host_epoch, table.valid_batches(), trainer


def bench(args):
    from stamp_amd.mil_train import fit
    lines = [f"MLP head, batch {BATCH}, hidden {HIDDEN}, C = {CLASSES}, 2 layers, dropout 0.25; {torch.cuda.get_device_name(0)}; median of {args.reps} calls per round, "
             "three interleaved rounds: median [min .. max] of the rounds, host clock around call + synchronise"]
    with tempfile.TemporaryDirectory() as d:
        for F in args.feats:
            routes = make_routes(F)
            train_res, train_host, valid, make = feeds(write_files(d, F), F)
            tr = make()

            def epoch(feed):
                for bags, _c, _s, targets in feed():
                    tr.step(bags, targets)

            empty = lambda: ()  # noqa: E731
            work = {"step, one-call trainer": (routes["trainer"], args.reps), "step, module path + torch AdamW": (routes["module"], args.reps),
                    "train epoch of 1000, resident table": (lambda: epoch(train_res), 3), "train epoch of 1000, file per item": (lambda: epoch(train_host), 3),
                    "validation of 1000, batch-1 loop": (lambda: fit(tr, empty, valid, max_epochs=1), 3),
                    "validation of 1000, one call": (lambda: fit(tr, empty, valid, max_epochs=1, valid_bags_per_call=ENTRIES), 3)}
            rounds = {k: [] for k in work}
            for _ in range(3):
                for k, (fn, reps) in work.items():
                    rounds[k].append(timed(fn, reps))
            lines.append(f"F = {F}")
            for k, v in rounds.items():
                lines.append(f"  {k:42s} {statistics.median(v) * 1e3:10.3f} ms  [{min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f}]")
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / "mlp_train_bench.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


def kernel_stats(dirs, steps):
    for d in dirs:
        for f in sorted(Path(d).rglob("*kernel_stats.csv")):
            print(f"{d}: kernels of one step ({f.name}; calls / {steps + 1})")
            rows = list(csv.DictReader(f.open()))
            total = 0
            for r in rows:
                calls = int(r.get("Calls") or r.get("calls") or 0)
                total += calls
                print(f"  {calls / (steps + 1):6.2f}  {(r.get('Name') or r.get('name') or '')[:110]}")
            print(f"  {total / (steps + 1):6.2f}  launches per step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--feats", default="768,1536,2560")
    ap.add_argument("--profile-call", choices=["trainer", "module"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-stats", nargs="+")
    args = ap.parse_args()
    args.feats = [int(v) for v in args.feats.split(",")]
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, args.steps)
    if args.profile_call:
        step = make_routes(args.feats[0])[args.profile_call]
        for _ in range(args.steps + 1):
            step()
        torch.cuda.synchronize()
        return
    bench(args)


if __name__ == "__main__":
    main()
