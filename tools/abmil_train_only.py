"""The gated-attention MIL head (stamp_amd/abmil.py) in a loop, for timing: eval forward, module step (autograd.Function + torch.optim.AdamW) and trainer
step (`HipAbmilTrainer`, flat AdamW), each next to the same arithmetic written in torch (tests/abmil_oracle.py, fp32, same GPU), at torch's "highest" and
"high" matmul precision.

    python tools/abmil_train_only.py [--rounds 3] [--steps 10] [--out profiles/abmil_train_bench.txt]

Shape: 64 bags x 1024 tiles x 768-d, CHIEF's "small" geometry (768 / 512 / 256), 2 classes; fp32 rows.  Rounds are interleaved: every round times every path
once, one after the other; the table reports the median and the spread.  The shader clock (and socket power) is sampled with `rocm-smi --showclocks` from a
host thread while each window runs and printed next to it.  HIP paths train with the reference's Dropout(0.25) live at all three sites; the torch yardstick
has no dropout (its three mask products would only add to its time).  No bar hangs on these numbers."""
import argparse
import copy
import re
import statistics
import subprocess
import sys
import threading
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import abmil_oracle as O  # noqa: E402
from stamp_amd.abmil import CHIEF_SIZES, GatedAttentionMIL, HipAbmilTrainer  # noqa: E402


class ClockSampler:
    """Mean shader clock (MHz) over the samples `rocm-smi --showclocks --csv` gives while a window runs; None when the tool or the field is missing."""

    def __init__(self):
        self.samples, self._stop, self._th = [], False, None

    def _run(self):
        while not self._stop:
            try:
                r = subprocess.run(["rocm-smi", "--showclocks", "--csv"], capture_output=True, text=True, timeout=10)
            except (OSError, subprocess.TimeoutExpired):
                return
            lines = [ln.split(",") for ln in r.stdout.strip().splitlines() if ln]
            if len(lines) >= 2:
                cols = [i for i, h in enumerate(lines[0]) if "sclk" in h.lower() and "level" not in h.lower()]
                m = re.search(r"(\d+)\s*mhz", lines[1][cols[0]].lower()) if cols and len(lines[1]) > cols[0] else None
                if m:
                    self.samples.append(int(m.group(1)))
            time.sleep(0.2)

    def __enter__(self):
        self.samples, self._stop = [], False
        self._th = threading.Thread(target=self._run, daemon=True)
        self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        self._th.join()

    def mean(self):
        return sum(self.samples) / len(self.samples) if self.samples else None


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--size", default="small", choices=sorted(CHIEF_SIZES))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the table here as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("abmil_train_only.py measures on the GPU: none visible")
    dev = torch.device("cuda")
    Fd, L, D = CHIEF_SIZES[a.size]
    torch.manual_seed(0)
    model = GatedAttentionMIL(Fd, L, D, 2)
    bags = torch.randn(a.batch, a.tiles, Fd, device=dev)
    x2 = bags.view(-1, Fd)
    lengths = [a.tiles] * a.batch
    tg = torch.nn.functional.one_hot(torch.arange(a.batch, device=dev) % 2, 2).float()

    tr = HipAbmilTrainer(copy.deepcopy(model), device=dev, max_lr=1e-4, total_steps=1 << 20, sched_interval="step")
    tm = copy.deepcopy(model).to(dev).train()
    opt = torch.optim.AdamW(tm.parameters(), lr=1e-4)
    te = copy.deepcopy(model).to(dev).eval()
    wt = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in model.state_dict().items()}
    opt_t = torch.optim.AdamW(list(wt.values()), lr=1e-4)

    def hip_eval():
        with torch.no_grad():
            return te(bags).sum()

    def torch_eval():
        with torch.no_grad():
            return O.forward(x2, lengths, wt)["logits"].sum()

    def hip_module():
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(tm(bags), tg)
        loss.backward()
        opt.step()
        return loss.detach()

    def torch_module():
        opt_t.zero_grad()
        loss = torch.nn.functional.cross_entropy(O.forward(x2, lengths, wt)["logits"], tg)
        loss.backward()
        opt_t.step()
        return loss.detach()

    paths = {"eval forward, HIP": hip_eval, "eval forward, torch fp32": torch_eval, "module step, HIP + torch AdamW": hip_module,
             "trainer step, HIP flat AdamW": lambda: tr.step(bags, tg)[0], "step, torch fp32 autograd + AdamW": torch_module}

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            v = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(v)

    lines = [f"gated-attention MIL head, {a.batch} bags x {a.tiles} tiles x {Fd}-d, L {L}, D {D}, 2 classes, fp32 rows; {a.steps} calls per window after {a.warmup} warm-up "
             f"calls, {a.rounds} interleaved rounds; device {torch.cuda.get_device_name(0)}",
             f"{'precision':9s} {'path':36s} {'ms (median)':>12s} {'bags/s':>9s} {'rounds (ms)':>26s} {'spread':>7s} {'sclk MHz':>9s}"]
    clock = ClockSampler()
    for precision in ("highest", "high"):
        torch.set_float32_matmul_precision(precision)
        for fn in paths.values():
            timed(fn, a.warmup)
        ms = {k: [] for k in paths}
        clk = {k: [] for k in paths}
        for r in range(a.rounds):
            for k, fn in paths.items():
                with clock:
                    t, v = timed(fn, a.steps)
                ms[k].append(t)
                if clock.mean() is not None:
                    clk[k].append(clock.mean())
                print(f"{precision} round {r} {k:36s} {t:9.3f} ms  {a.batch / t * 1e3:9.0f} bags/s  value {v:.4f}", flush=True)
        for k, v in ms.items():
            med = statistics.median(v)
            c = f"{sum(clk[k]) / len(clk[k]):9.0f}" if clk[k] else "      n/a"
            lines.append(f"{precision:9s} {k:36s} {med:12.3f} {a.batch / med * 1e3:9.0f} {' '.join(f'{x:.3f}' for x in v):>26s} {max(v) - min(v):7.3f} {c}")
    torch.set_float32_matmul_precision("highest")
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
