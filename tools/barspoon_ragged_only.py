"""The barspoon head's deploy forward over whole bags: the one-bag loop `deploy.predict_` runs by default (one dense call and one host read per target
and bag) against ragged calls of 64 bags (`EncDecTransformer.forward_ragged`, one host read per target and call).

Default head (512 / 8 + 8 heads / 2048 / 2 + 2 layers), d_features = 1024, fp16 features, two targets, positional encoding on; cohorts: (a) 256 bags,
log-uniform 256 .. 16 384 tiles, seed 0; (b) 256 bags of 1024; (c) skewed: one bag of 30 000 and 63 of 300.  Both paths run in this process after every
shape was warmed, alternated in three pairs; device work ends in a synchronise; the outputs of the two paths on the timed inputs are compared with
torch.equal before anything is timed.

    python tools/barspoon_ragged_only.py [--out DIR] [--profile-call]

--profile-call: one 64-bag ragged call of cohort (b) after a warm-up, nothing else (for `rocprofv3 --kernel-trace --stats -- python ...`)."""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from stamp_amd.barspoon import EncDecTransformer  # noqa: E402

TARGETS = {"KRAS": 2, "MSI status": 3}
K = 64


def cohorts():
    g = torch.Generator().manual_seed(0)
    a = [int(round(math.exp(math.log(256) + (math.log(16384) - math.log(256)) * u))) for u in torch.rand(256, generator=g).tolist()]
    return {"a_loguniform": a, "b_1024": [1024] * 256, "c_skewed": [30000] + [300] * 63}


def make_bags(lengths, seed=1):
    g = torch.Generator().manual_seed(seed)
    bags = [torch.randn(t, 1024, generator=g).half().cuda() for t in lengths]
    pos = [(torch.rand(t, 2, generator=g) * 50000).cuda() for t in lengths]
    return bags, pos


def probs(out):
    """`predict_`'s host read: softmax per target on the device, then to the CPU"""
    return {t: torch.softmax(v.float(), 1).cpu() for t, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-call", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(1)
    m = EncDecTransformer(1024, TARGETS).cuda().eval()
    torch.set_grad_enabled(False)
    if args.profile_call:
        bags, pos = make_bags([1024] * K)
        m.forward_ragged(bags, pos)
        torch.cuda.synchronize()
        m.forward_ragged(bags, pos)
        torch.cuda.synchronize()
        print("profiled one 64-bag ragged call")
        return
    rows = []
    for name, lengths in cohorts().items():
        bags, pos = make_bags(lengths)

        def loop():
            return [probs(m(b[None], p[None])) for b, p in zip(bags, pos)]

        def ragged():
            return [probs(m.forward_ragged(bags[s:s + K], pos[s:s + K])) for s in range(0, len(bags), K)]

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        a, b = loop(), ragged()                                     # warms every shape of both paths
        equal = all(torch.equal(torch.cat([x[t] for x in a]), torch.cat([y[t] for y in b])) for t in TARGETS)
        tl, tr = [], []
        for _ in range(3):
            tl.append(timed(loop))
            tr.append(timed(ragged))
        res = {"cohort": name, "bags": len(bags), "tiles": sum(lengths), "outputs_equal": equal, "loop_ms": [round(x, 2) for x in tl],
               "loop_median_ms": round(statistics.median(tl), 2), f"ragged{K}_ms": [round(x, 2) for x in tr],
               f"ragged{K}_median_ms": round(statistics.median(tr), 2), "loop_spread_ms": round(max(tl) - min(tl), 2)}
        res["speedup"] = round(res["loop_median_ms"] / res[f"ragged{K}_median_ms"], 2)
        print(json.dumps(res), flush=True)
        rows.append(res)
        del bags, pos
        torch.cuda.empty_cache()
    if args.out:
        out = Path(args.out)
        out.mkdir(parents=True, exist_ok=True)
        (out / "barspoon_ragged_bench.json").write_text(json.dumps({"device": torch.cuda.get_device_name(0), "max_shared_tiles": m.max_shared_tiles("cuda:0"),
                                                                    "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
