"""Grad-CAM scores of one slide: the fused path (one amds_mil_vit_gradcam call, no Jacobian) against `method="jacrev"` (one HIP backward per class through
torch.func.jacrev, the [C, N, F] Jacobian, then the reduction), alternated in one process; and the split of one whole `slide_heatmap` call.

Default head (512 / 8 heads / 512 / 2 layers), fp32 features, F in {1024, 1536}, C in {2, 4}, N in {1024, 8192, 32768, 65536}.  Per point: each method
warmed up, median of --reps calls (host clock around a device synchronise), the pair measured twice (run 0 / run 1: the spread), peak memory of each.

    python tools/heatmap_only.py [--out DIR] [--reps N] [--sizes 1024,8192] [--feats 1024] [--classes 2,4] [--alibi] [--precision high|medium]
    python tools/heatmap_only.py --profile-call [--sizes 8192]
    python tools/heatmap_only.py --model transmil [--hidden 512] [--precision high|highest] [--routes library,jacrev] [--count-launches]

--profile-call: one fused `gradcam` call at the first size / F / C after a warm-up, nothing else (for `rocprofv3 --kernel-trace --stats -- python ...`); with
--model transmil the call is the first of --routes.
--model transmil: `stamp_amd.mil.TransMIL` (dim_hidden --hidden), routes "library" (one amds_transmil_gradcam call) and "jacrev" (one amds_transmil_train_backward
per class, the [C, N, F] Jacobian, the reduction), interleaved like the pair above; writes heatmap_transmil_ab_<precision>.{txt,json}.  --count-launches: the device kernels of
one call of each route (torch.profiler), also per class."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from stamp_amd import heatmaps, mil_core  # noqa: E402
from stamp_amd.mil import TransMIL, VisionTransformer  # noqa: E402


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


def count_kernels(fn):
    """Device kernels launched by one call of `fn` (None where the profiler gives no device events)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    return n or None


def main_transmil(args, sizes, fs, cs):
    routes = args.routes.split(",")
    assert all(r in ("library", "jacrev") for r in routes) and routes, routes
    call = lambda m, feats, route: heatmaps.gradcam(m, feats, raw=True, method=route)  # noqa: E731

    def model(f, c):
        torch.manual_seed(1)
        return TransMIL(dim_output=c, dim_input=f, dim_hidden=args.hidden).cuda().eval()

    if args.profile_call:
        m = model(fs[0], cs[0])
        feats, _ = slide(sizes[0], fs[0])
        for _ in range(2):
            call(m, feats, routes[0])
            torch.cuda.synchronize()
        print(f"profiled one TransMIL {routes[0]} gradcam call: N={sizes[0]} F={fs[0]} C={cs[0]} dim_hidden={args.hidden} precision={args.precision}")
        return
    rows, lines = [], []
    for f in fs:
        for c in cs:
            m = model(f, c)
            for n in sizes:
                feats, _ = slide(n, f)
                res = {"N": n, "F": f, "C": c, "dim_hidden": args.hidden, "precision": args.precision}
                try:
                    for run in (0, 1):                              # the routes twice, alternated: run-to-run spread
                        for r in reversed(routes):
                            res[f"{r}_ms_run{run}"] = round(timed(lambda: call(m, feats, r), args.reps) * 1e3, 3)
                    for r in routes:
                        res[f"{r}_peak_MiB"] = round(peak(lambda: call(m, feats, r)) / 2 ** 20, 1)
                        if args.count_launches:
                            res[f"{r}_kernels"] = count_kernels(lambda: call(m, feats, r))
                    line = f"N={n:6d} F={f} C={c} hidden={args.hidden} {args.precision}: " + ", ".join(
                        f"{r} {res[f'{r}_ms_run0']:9.2f} / {res[f'{r}_ms_run1']:9.2f} ms peak {res[f'{r}_peak_MiB']:.0f} MiB"
                        + (f" kernels {res[f'{r}_kernels']} ({(res[f'{r}_kernels'] or 0) / c:.1f} per class)" if args.count_launches else "") for r in routes)
                    if len(routes) == 2:
                        line += "; jacrev / library " + " / ".join(f"{res[f'jacrev_ms_run{k}'] / res[f'library_ms_run{k}']:.3f}" for k in (0, 1))
                    lines.append(line)
                except (RuntimeError, torch.OutOfMemoryError) as e:          # a size the library or the memory does not take: said, not hidden
                    res["skipped"] = str(e).splitlines()[0][:300]
                    lines.append(f"N={n:6d} F={f} C={c}: skipped ({res['skipped']})")
                print(lines[-1], flush=True)
                rows.append(res)
                del feats
                torch.cuda.empty_cache()
    if args.out:
        out = Path(args.out)
        out.mkdir(parents=True, exist_ok=True)
        (out / f"heatmap_transmil_ab_{args.precision}.json").write_text(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, indent=1) + "\n")
        (out / f"heatmap_transmil_ab_{args.precision}.txt").write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,8192,32768,65536")
    ap.add_argument("--feats", default="1024,1536")
    ap.add_argument("--classes", default="2,4")
    ap.add_argument("--alibi", action="store_true")
    ap.add_argument("--precision", default="high", choices=["high", "medium", "highest"])
    ap.add_argument("--profile-call", action="store_true")
    ap.add_argument("--model", default="vit", choices=["vit", "transmil"])
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--routes", default="library,jacrev")
    ap.add_argument("--count-launches", action="store_true")
    args = ap.parse_args()
    sizes, fs, cs = ([int(v) for v in s.split(",")] for s in (args.sizes, args.feats, args.classes))
    torch.set_float32_matmul_precision(args.precision)
    if args.model == "transmil":
        return main_transmil(args, sizes, fs, cs)
    if args.precision == "highest":
        ap.error("--precision highest is for --model transmil (the vit head's operands are 16-bit)")

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
