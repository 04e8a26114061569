"""Condense the `sharp|` lines of `python -m pytest tests/test_gpu_attention_sharp.py -s` (stdin) into profiles/attention_sharp_errors.txt's table (stdout):
per entry one row per (builder, tensor), one cell per shape holding kernel error / model error as bf16/fp16.  A cell in brackets is error / bar instead: the
model's error there is exactly 0 or below the fp32 term that then sets the bar (T = 1, `saturated` and `uniform` dq / dk, lse, fp32 outputs)."""
import math
import re
import sys

rows, order = {}, {}
worst = (0.0, "")
for line in sys.stdin:
    m = re.search(r"sharp\| (\S+(?: p=\S+)?)\s+(\w+)(\(\S+\)(?: \S+=\S+)?| bag of \d+)\s+(bf16|fp16) (\w+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)", line)
    if not m:
        continue
    entry, builder, shape, dt, tensor = m.group(1), m.group(2), m.group(3).strip(), m.group(4), m.group(5)
    rel, mrel, ratio, rl2, rmx = (float(x) for x in m.group(6, 7, 8, 9, 10))
    bar = max(rl2, rmx)
    if bar > worst[0]:
        worst = (bar, f"{entry} {builder}{shape} {dt} {tensor}")
    cell = f"{ratio:.2f}" if (not math.isnan(ratio) and 0.5 <= ratio <= 2.0 and tensor != "lse") else f"[{bar:.3f}]"
    order.setdefault(entry, [])
    if shape not in order[entry]:
        order[entry].append(shape)
    rows.setdefault(entry, {}).setdefault((builder, tensor), {}).setdefault(shape, {})[dt] = cell
print(f"largest error / bar: {worst[0]:.3f} ({worst[1]})\n")
for entry, table in rows.items():
    shapes = order[entry]
    print(f"{entry}\n  {'builder':10s} {'':4s} " + " ".join(f"{s:>15s}" for s in shapes))
    for (builder, tensor), cells in table.items():
        print(f"  {builder:10s} {tensor:4s} " + " ".join(f"{'/'.join(cells[s].get(d, '-') for d in ('bf16', 'fp16')) if s in cells else '':>15s}" for s in shapes))
    print()
