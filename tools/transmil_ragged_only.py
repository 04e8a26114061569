"""The TransMIL head's inference forward over whole bags: the one-bag loop `deploy.predict_` runs by default (one call and one host read per bag) against
ragged calls of 16 and 64 bags (`TransMIL.forward_ragged`), plus the dense 64 x 1024 call for the varlen overhead.

Default head (dim_hidden 512), F = 1024, fp16 features, at torch's float32 matmul precision "medium" (the reference's deploy setting, deploy.py:398) and "high";
cohorts: (a) 256 bags, log-uniform 256 .. 16 384 tiles, seed 0; (b) 256 bags of 1024.  Timed with device events around each pass, one warm-up pass, best of --reps.

    python tools/transmil_ragged_only.py [--out DIR] [--reps N] [--side loop|ragged|all] [--commit HASH] [--loop-json FILE] [--profile-call]

--side loop: the one-bag loop alone (runs on a checkout without the ragged entry, e.g. the parent commit; --out then holds transmil_ragged_loop.json);
--loop-json: take the loop's rows from such a file instead of timing the loop again (both commits are recorded in the result);
--profile-call: one 64-bag ragged call of cohort (b) after a warm-up, nothing else (for `rocprofv3 --kernel-trace --stats -- python ...`)."""
import argparse
import json
import math
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from stamp_amd.mil import TransMIL  # noqa: E402


def cohorts():
    g = torch.Generator().manual_seed(0)
    a = [int(round(math.exp(math.log(256) + (math.log(16384) - math.log(256)) * u))) for u in torch.rand(256, generator=g).tolist()]
    return {"b_1024": [1024] * 256, "a_loguniform": a}


def make_bags(lengths, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(t, 1024, generator=g).half().cuda() for t in lengths]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--side", choices=("loop", "ragged", "all"), default="all")
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--loop-json", default=None)
    ap.add_argument("--profile-call", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(1)
    m = TransMIL(dim_output=2, dim_input=1024, dim_hidden=512).cuda().eval()
    torch.set_grad_enabled(False)
    if args.profile_call:
        torch.set_float32_matmul_precision("medium")
        bags = make_bags([1024] * 64)
        m.forward_ragged(bags)
        torch.cuda.synchronize()
        m.forward_ragged(bags)
        torch.cuda.synchronize()
        print("profiled one 64-bag ragged call")
        return
    loop_rows = {}
    loop_commit = args.commit
    if args.loop_json:
        prev = json.loads(Path(args.loop_json).read_text())
        loop_commit = prev["commit"]
        loop_rows = {(r["cohort"], r["precision"]): r for r in prev["rows"]}
    rows = []
    for name, lengths in cohorts().items():
        bags = make_bags(lengths)
        for precision in ("medium", "high"):
            torch.set_float32_matmul_precision(precision)

            def loop():
                for b in bags:
                    y = m(b[None])
                    float(y[0, 0])                                  # the host read of `predict_` (.cpu())

            def ragged(k):
                def run():
                    for s in range(0, len(bags), k):
                        y = m.forward_ragged(bags[s:s + k])
                        float(y[0, 0])
                return run

            res = {"cohort": name, "precision": precision, "bags": len(bags), "tiles": sum(lengths)}
            if (name, precision) in loop_rows:
                res["loop_ms"], res["loop_bags_per_s"] = loop_rows[(name, precision)]["loop_ms"], loop_rows[(name, precision)]["loop_bags_per_s"]
            elif args.side in ("loop", "all"):
                t = timed(loop, args.reps)
                res["loop_ms"], res["loop_bags_per_s"] = round(t * 1e3, 2), round(len(bags) / t, 1)
            if args.side in ("ragged", "all"):
                for k in (16, 64):
                    t = timed(ragged(k), args.reps)
                    res[f"ragged{k}_ms"], res[f"ragged{k}_bags_per_s"] = round(t * 1e3, 2), round(len(bags) / t, 1)
                if "loop_bags_per_s" in res:
                    res["speedup64"] = round(res["ragged64_bags_per_s"] / res["loop_bags_per_s"], 2)
            print(json.dumps(res), flush=True)
            rows.append(res)
        del bags
        torch.cuda.empty_cache()
    if args.side in ("ragged", "all"):      # the varlen overhead: 64 x 1024 as one dense call against one ragged call
        bags = make_bags([1024] * 64)
        dense = torch.stack(bags)
        for precision in ("medium", "high"):
            torch.set_float32_matmul_precision(precision)
            td = timed(lambda: m(dense), 10)
            tr = timed(lambda: m.forward_ragged(bags), 10)
            res = {"cohort": "dense_vs_ragged_64x1024", "precision": precision, "dense_ms": round(td * 1e3, 3), "ragged_ms": round(tr * 1e3, 3),
                   "ragged_over_dense": round(tr / td, 3)}
            print(json.dumps(res), flush=True)
            rows.append(res)
    if args.out:
        out = Path(args.out)
        out.mkdir(parents=True, exist_ok=True)
        name = "transmil_ragged_loop.json" if args.side == "loop" else "transmil_ragged_bench.json"
        doc = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "rows": rows}
        if args.side != "loop":
            doc = {"device": doc["device"], "loop_commit": loop_commit, "ragged_commit": args.commit, "rows": rows}
        (out / name).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
