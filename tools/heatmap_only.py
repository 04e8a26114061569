"""Grad-CAM scores of one slide: the fused path (one amds_mil_vit_gradcam call, no Jacobian) against `method="jacrev"` (one HIP backward per class through
torch.func.jacrev, the [C, N, F] Jacobian, then the reduction), alternated in one process; and the split of one whole `slide_heatmap` call.

Default head (512 / 8 heads / 512 / 2 layers), fp32 features, F in {1024, 1536}, C in {2, 4}, N in {1024, 8192, 32768, 65536}.  Per point: each method
warmed up, median of --reps calls (host clock around a device synchronise), the pair measured twice (run 0 / run 1: the spread), peak memory of each.

    python tools/heatmap_only.py [--out DIR] [--reps N] [--sizes 1024,8192] [--feats 1024] [--classes 2,4] [--alibi] [--precision high|medium]
    python tools/heatmap_only.py --profile-call [--sizes 8192]

--profile-call: one fused `gradcam` call at the first size / F / C after a warm-up, nothing else (for `rocprofv3 --kernel-trace --stats -- python ...`)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from stamp_amd import heatmaps, mil_core  # noqa: E402
from stamp_amd.mil import VisionTransformer  # noqa: E402


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


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


def slide(n, f, seed=1):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(n, f, generator=g).cuda()
    side = int(n ** 0.5) + 2
    cells = torch.randperm(side * side, generator=g)[:n]
    coords = (torch.stack([cells % side, cells // side], dim=1).float() * 256.0).cuda()
    return feats, coords


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,8192,32768,65536")
    ap.add_argument("--feats", default="1024,1536")
    ap.add_argument("--classes", default="2,4")
    ap.add_argument("--alibi", action="store_true")
    ap.add_argument("--precision", default="high", choices=["high", "medium"])
    ap.add_argument("--profile-call", action="store_true")
    args = ap.parse_args()
    sizes, fs, cs = ([int(v) for v in s.split(",")] for s in (args.sizes, args.feats, args.classes))
    torch.set_float32_matmul_precision(args.precision)

    def model(f, c):
        torch.manual_seed(1)
        return VisionTransformer(dim_output=c, dim_input=f, dim_model=512, n_layers=2, n_heads=8, dim_feedforward=512, dropout=0.0, use_alibi=args.alibi).cuda().eval()

    if args.profile_call:
        m = model(fs[0], cs[0])
        feats, coords = slide(sizes[0], fs[0])
        heatmaps.gradcam(m, feats, coords, raw=True)
        torch.cuda.synchronize()
        heatmaps.gradcam(m, feats, coords, raw=True)
        torch.cuda.synchronize()
        print(f"profiled one fused gradcam call: N={sizes[0]} F={fs[0]} C={cs[0]} alibi={args.alibi}")
        return
    rows, lines = [], []
    for f in fs:
        for c in cs:
            m = model(f, c)
            for n in sizes:
                feats, coords = slide(n, f)
                res = {"N": n, "F": f, "C": c, "alibi": args.alibi, "precision": args.precision}
                if args.alibi:          # the scaler buffers as training leaves them (the mean tile distance): at their initial 1.0 the distance term overflows fp16
                    with torch.no_grad():
                        md = torch.cdist(coords[:4096], coords[:4096]).mean()
                        for name, b in m.named_buffers():
                            if name.endswith("running_mean"):
                                b.fill_(md)
                m.fp16_overflow_events = 0
                fused = lambda: heatmaps.gradcam(m, feats, coords, raw=True)  # noqa: E731
                jac = lambda: heatmaps.gradcam(m, feats, coords, raw=True, method="jacrev")  # noqa: E731
                try:
                    for run in (0, 1):                              # the pair twice, alternated: run-to-run spread
                        res[f"jacrev_ms_run{run}"] = round(timed(jac, args.reps) * 1e3, 3)
                        res[f"fused_ms_run{run}"] = round(timed(fused, args.reps) * 1e3, 3)
                        res[f"ratio_run{run}"] = round(res[f"jacrev_ms_run{run}"] / res[f"fused_ms_run{run}"], 3)
                    res["fp16_overflow_events"] = m.fp16_overflow_events          # (> 0: both paths re-ran on bf16 operands; the point then times the fallback)
                    res["fused_peak_MiB"], res["jacrev_peak_MiB"] = round(peak(fused) / 2 ** 20, 1), round(peak(jac) / 2 ** 20, 1)
                    # one whole slide_heatmap call and its parts, each timed on its own
                    with torch.no_grad():
                        res["slide_score_forward_ms"] = round(timed(lambda: m(feats[None], coords=coords[None], mask=None), args.reps) * 1e3, 3)
                    tensors = dict(m.named_parameters())
                    tensors.update(dict(m.named_buffers()))
                    pk = mil_core.PackedVit(m.dims, lambda k: tensors[k].detach().float(), torch.float16 if args.precision == "high" else torch.bfloat16, True)
                    res["gradcam_train_forward_ms"] = round(timed(lambda: mil_core.forward_train(pk, feats[None], coords[None], training=False), args.reps) * 1e3, 3)
                    res["gradcam_ms"] = round(timed(lambda: heatmaps.gradcam(m, feats, coords), args.reps) * 1e3, 3)
                    res["tile_scores_ms"] = round(timed(lambda: heatmaps.tile_scores(m, feats, coords), args.reps) * 1e3, 3)
                    res["slide_heatmap_ms"] = round(timed(lambda: heatmaps.slide_heatmap(m, feats, coords, task="classification"), args.reps) * 1e3, 3)
                    res["rest_ms"] = round(res["slide_heatmap_ms"] - res["slide_score_forward_ms"] - res["gradcam_ms"] - res["tile_scores_ms"], 3)
                    lines.append(f"N={n:6d} F={f} C={c}: jacrev {res['jacrev_ms_run0']:9.2f} / {res['jacrev_ms_run1']:9.2f} ms, fused {res['fused_ms_run0']:9.2f} / "
                                 f"{res['fused_ms_run1']:9.2f} ms, ratio {res['ratio_run0']:.2f} / {res['ratio_run1']:.2f}; peak {res['jacrev_peak_MiB']:.0f} vs "
                                 f"{res['fused_peak_MiB']:.0f} MiB; slide_heatmap {res['slide_heatmap_ms']:.2f} ms = score forward {res['slide_score_forward_ms']:.2f} + gradcam "
                                 f"{res['gradcam_ms']:.2f} (its forward {res['gradcam_train_forward_ms']:.2f}) + tile scores {res['tile_scores_ms']:.2f} + rest {res['rest_ms']:.2f}; fp16 overflow events {res['fp16_overflow_events']}")
                except (RuntimeError, torch.OutOfMemoryError) as e:          # a size the library or the memory does not take: said, not hidden
                    res["skipped"] = str(e).splitlines()[0][:300]
                    lines.append(f"N={n:6d} F={f} C={c}: skipped ({res['skipped']})")
                print(lines[-1], flush=True)
                rows.append(res)
                del feats, coords
                torch.cuda.empty_cache()
    if args.out:
        out = Path(args.out)
        out.mkdir(parents=True, exist_ok=True)
        tag = "_alibi" if args.alibi else ""
        (out / f"heatmap_gradcam_ab{tag}.json").write_text(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, indent=1) + "\n")
        (out / f"heatmap_gradcam_ab{tag}.txt").write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
