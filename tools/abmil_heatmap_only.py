"""Heat-map scores of the gated-attention MIL head (stamp_amd/abmil.py) in a loop, for timing: the ONE library call (`heatmap_scores` ->
amds_abmil_heatmap) next to the same outputs composed from the entries the head had before it:

    one `forward_infer` (logits, raw scores); per class a `forward_train` (p = 0) + `backward(need_x=True)` with dlogits = e_c and torch's
    ``(x * dx).mean(-1).abs()``; one `forward_infer` over every row as a bag of its own (the tile logits).

    python tools/abmil_heatmap_only.py [--rounds 3] [--steps 50] [--out profiles/abmil_heatmap_bench.txt]

Shape: one slide of 8 192 and of 32 768 tiles x 768-d, CHIEF's "small" geometry (768 / 512 / 256), 2 and 4 classes, fp32 rows, torch's "highest" and "high"
matmul precision.  Rounds are interleaved: every round times both routes once, one after the other; the table reports the median and the spread (max - min
over the rounds).  Host clock around the calls plus a device synchronise; the shader clock is sampled as tools/abmil_train_only.py does; peak memory is
torch's allocator peak above the resident state during one call of the route, after warm-up: outputs, saved arenas and dx -- inputs, weights and the
grow-only scratch workspaces of both routes are resident and not counted.  Before timing, the two routes' outputs are compared.
The condition printed per cell: the one call is not slower than the composed route by more than the two spreads."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from abmil_train_only import ClockSampler  # noqa: E402
from stamp_amd import abmil  # noqa: E402
from stamp_amd.abmil import CHIEF_SIZES, GatedAttentionMIL  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--size", default="small", choices=sorted(CHIEF_SIZES))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the table here as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("abmil_heatmap_only.py measures on the GPU: none visible")
    dev = torch.device("cuda")
    Fd, L, D = CHIEF_SIZES[a.size]
    lines = [f"gated-attention MIL head, heat-map scores of ONE slide x {Fd}-d, L {L}, D {D}, fp32 rows; {a.steps} calls per window after {a.warmup} warm-up calls, "
             f"{a.rounds} interleaved rounds; device {torch.cuda.get_device_name(0)}",
             "one call = amds_abmil_heatmap (logits, scores, weights, cam_raw of all classes, tile logits); composed = forward_infer + per class (forward_train + "
             "backward(dx) + torch row-dot) + forward_infer over one-row bags; peak MiB = allocator peak above the resident state during one call (scratch workspaces not counted)",
             f"{'precision':9s} {'tiles':>6s} {'C':>2s} {'route':9s} {'ms (median)':>12s} {'rounds (ms)':>26s} {'spread':>7s} {'peak MiB':>9s} {'sclk MHz':>9s}  ratio / condition"]
    clock = ClockSampler()

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def peak_mib(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        del out
        return (peak - base) / 2 ** 20

    for precision in ("highest", "high"):
        torch.set_float32_matmul_precision(precision)
        for N in a.tiles:
            for Cn in a.classes:
                torch.manual_seed(0)
                model = GatedAttentionMIL(Fd, L, D, Cn).to(dev).eval()
                w = model._c_weights(dev)
                dims = model.dims
                x = torch.randn(N, Fd, device=dev)
                offs, offs_rows = abmil._offsets([N], dev), torch.arange(N + 1, dtype=torch.int64, device=dev)
                eye = torch.eye(Cn, device=dev)

                def one_call():
                    with torch.no_grad():
                        return abmil.heatmap_scores(w, dims, x, offs, 1)

                def composed():
                    with torch.no_grad():
                        logits, raw = abmil.forward_infer(w, dims, x, offs, 1, return_attn=True)
                        cams = []
                        for c in range(Cn):
                            _, saved = abmil.forward_train(w, dims, x, offs, 1, p_fc=0.0, p_gate=0.0, seed=0)
                            _, dx = abmil.backward(saved, eye[c:c + 1], need_params=False, need_x=True)
                            cams.append((x * dx).mean(-1).abs())
                        tiles = abmil.forward_infer(w, dims, x, offs_rows, N)
                        return {"logits": logits, "attn_raw": raw, "cam_raw": torch.stack(cams), "tile_logits": tiles}

                paths = {"one call": one_call, "composed": composed}
                ra, rb = one_call(), composed()
                agree = {k: float((ra[k] - rb[k]).abs().max() / rb[k].abs().max()) for k in rb}
                print(f"{precision} {N} tiles C={Cn}: max |one call - composed| / max |composed|: " + ", ".join(f"{k} {v:.2e}" for k, v in agree.items()), flush=True)
                del ra, rb
                for fn in paths.values():
                    timed(fn, a.warmup)
                ms = {k: [] for k in paths}
                clk = {k: [] for k in paths}
                for r in range(a.rounds):
                    for k, fn in paths.items():
                        with clock:
                            t = timed(fn, a.steps)
                        ms[k].append(t)
                        if clock.mean() is not None:
                            clk[k].append(clock.mean())
                        print(f"{precision} {N} tiles C={Cn} round {r} {k:9s} {t:9.3f} ms", flush=True)
                mem = {k: peak_mib(fn) for k, fn in paths.items()}
                med = {k: statistics.median(v) for k, v in ms.items()}
                spread = {k: max(v) - min(v) for k, v in ms.items()}
                ok = med["one call"] <= med["composed"] + spread["one call"] + spread["composed"]
                for k, v in ms.items():
                    c = f"{sum(clk[k]) / len(clk[k]):9.0f}" if clk[k] else "      n/a"
                    tail = f"  composed / one call = {med['composed'] / med['one call']:.2f}; not slower: {'yes' if ok else 'NO'}; outputs agree to " \
                           f"{max(agree.values()):.1e}" if k == "one call" else ""
                    lines.append(f"{precision:9s} {N:6d} {Cn:2d} {k:9s} {med[k]:12.3f} {' '.join(f'{t:.3f}' for t in v):>26s} {spread[k]:7.3f} {mem[k]:9.1f} {c}{tail}")
    torch.set_float32_matmul_precision("highest")
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
