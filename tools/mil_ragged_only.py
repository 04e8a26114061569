"""The MIL `vit` head's inference forward over whole bags: the one-bag loop `fit` and `deploy.predict_` run by default (one call and one host read
per bag) against ragged calls of 16 and 64 bags (`VisionTransformer.forward_ragged`), plus the dense 64 x 1024 call for the varlen overhead.

Default head (512 / 8 heads / 512 / 2 layers), F = 1024, fp16 features, plain and ALiBi; cohorts: (a) 256 bags, log-uniform 256 .. 16 384 tiles, seed 0;
(b) 256 bags of 1024; (c) skewed: one bag of 30 000 and 63 of 300.

    python tools/mil_ragged_only.py [--out DIR] [--reps N] [--profile-call]

--profile-call: one 64-bag ragged call of cohort (b) after a warm-up, nothing else (for `rocprofv3 --kernel-trace --stats -- python ...`)."""
import argparse
import json
import math
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from stamp_amd.mil import VisionTransformer  # noqa: E402


def cohorts():
    g = torch.Generator().manual_seed(0)
    a = [int(round(math.exp(math.log(256) + (math.log(16384) - math.log(256)) * u))) for u in torch.rand(256, generator=g).tolist()]
    return {"a_loguniform": a, "b_1024": [1024] * 256, "c_skewed": [30000] + [300] * 63}


def make_bags(lengths, seed=1):
    g = torch.Generator().manual_seed(seed)
    bags = [torch.randn(t, 1024, generator=g).half().cuda() for t in lengths]
    coords = [(torch.rand(t, 2, generator=g) * 50000).cuda() for t in lengths]
    return bags, coords


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile-call", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(1)
    models = {alibi: VisionTransformer(dim_output=2, dim_input=1024, dim_model=512, n_layers=2, n_heads=8, dim_feedforward=512, dropout=0.0,
                                       use_alibi=alibi).cuda().eval() for alibi in (False, True)}
    torch.set_grad_enabled(False)
    if args.profile_call:
        bags, _ = make_bags([1024] * 64)
        m = models[False]
        m.forward_ragged(bags)
        torch.cuda.synchronize()
        m.forward_ragged(bags)
        torch.cuda.synchronize()
        print("profiled one 64-bag ragged call")
        return
    rows = []
    for name, lengths in cohorts().items():
        bags, coords = make_bags(lengths)
        for alibi, m in models.items():
            cc = coords if alibi else None

            def loop():
                for i, b in enumerate(bags):
                    y = m(b[None], coords=None if cc is None else cc[i][None], mask=None)
                    float(y[0, 0])                                  # the host read of `fit` (float(loss)) / `predict_` (.cpu())

            def ragged(k):
                def run():
                    for s in range(0, len(bags), k):
                        y = m.forward_ragged(bags[s:s + k], coords=None if cc is None else cc[s:s + k])
                        float(y[0, 0])
                return run

            res = {"cohort": name, "alibi": alibi, "bags": len(bags), "tiles": sum(lengths)}
            t = timed(loop, args.reps)
            res["loop_ms"], res["loop_bags_per_s"] = round(t * 1e3, 2), round(len(bags) / t, 1)
            for k in (16, 64):
                t = timed(ragged(k), args.reps)
                res[f"ragged{k}_ms"], res[f"ragged{k}_bags_per_s"] = round(t * 1e3, 2), round(len(bags) / t, 1)
            res["speedup64"] = round(res["ragged64_bags_per_s"] / res["loop_bags_per_s"], 2)
            print(json.dumps(res), flush=True)
            rows.append(res)
        del bags, coords
        torch.cuda.empty_cache()
    # the varlen overhead: 64 x 1024 as one dense call against one ragged call
    bags, coords = make_bags([1024] * 64)
    dense = torch.stack(bags)
    dcoords = torch.stack(coords)
    for alibi, m in models.items():
        td = timed(lambda: m(dense, coords=dcoords if alibi else None, mask=None), 10)
        tr = timed(lambda: m.forward_ragged(bags, coords=coords if alibi else None), 10)
        res = {"cohort": "dense_vs_ragged_64x1024", "alibi": alibi, "dense_ms": round(td * 1e3, 3), "ragged_ms": round(tr * 1e3, 3),
               "ragged_over_dense": round(tr / td, 3)}
        print(json.dumps(res), flush=True)
        rows.append(res)
    if args.out:
        out = Path(args.out)
        out.mkdir(parents=True, exist_ok=True)
        (out / "mil_ragged_bench.json").write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
