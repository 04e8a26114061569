"""TICON slide mode at the published geometry (dim 1536, 24 heads, depth 6, in_dim 1536; random weights): what one slide costs.

Per N in {1 024, 8 192, 32 768} tiles, on one GPU in one run:
  * `HipTiconSlide.forward` (fp16 operands, check=False): ms per slide and tiles/s -- device events around `reps` back-to-back calls after a warm-up;
  * `amds_attention_distbias` alone at (1, N, 24): ms and TF/s (4 N^2 64 heads flops, exp and distance work not counted) from a back-to-back loop between
    two device events, and its share of the slide = depth x that time / the slide's time;
  * yardstick (ii): `amds_attention` (no bias) at the same shape, same loop;
  * yardstick (i), N <= 8 192: a torch restatement of the model in fp16 that materialises the [24, N, N] bias, as the reference does;
  * the shader clock (and socket power) sampled from hwmon while the slide loop runs.
No pass / fail threshold: it reports what the path does.  Writes one JSON file (default profiles/ticon_slide_bench.json).

    python tools/ticon_slide_bench.py [--sizes 1024 8192 32768] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DIM, HEADS, DEPTH, IN_DIM, KEY = 1536, 24, 6, 1536, "hoptimus1"
HIDDEN = int(DIM * 16 / 3)


def random_state_dict(seed: int = 0) -> dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)

    def lin(n, k):
        return torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g) * 0.02

    sd: dict[str, torch.Tensor] = {}

    def put(name, n, k):
        sd[name + ".weight"], sd[name + ".bias"] = lin(n, k)

    def norm(name):
        sd[name + ".weight"], sd[name + ".bias"] = 1 + 0.1 * torch.randn(DIM, generator=g), 0.1 * torch.randn(DIM, generator=g)

    p = f"input_proj_dict.input_proj_{KEY}."
    put(p + "fc1", DIM, IN_DIM)
    put(p + "fc2", DIM, DIM)
    norm(p + "norm")
    for l in range(DEPTH):
        b = f"encoder.blocks.{l}."
        norm(b + "residual1.norm")
        for n in ("q_proj", "k_proj", "v_proj", "proj"):
            put(b + "residual1.fn." + n, DIM, DIM)
        sd[b + "residual1.gamma"] = 0.5 + 0.1 * torch.randn(DIM, generator=g)
        norm(b + "residual2.norm")
        put(b + "residual2.fn.fc1", HIDDEN, DIM)
        put(b + "residual2.fn.fc2", DIM, HIDDEN // 2)
        sd[b + "residual2.gamma"] = 0.5 + 0.1 * torch.randn(DIM, generator=g)
    norm("enc_norm")
    return sd


def torch_fp16_forward(emb, coords, sd, slopes):
    """The model in torch fp16 with the [heads, N, N] bias materialised (one slide)."""
    p = f"input_proj_dict.input_proj_{KEY}."
    x = F.linear(F.silu(F.linear(emb, sd[p + "fc1.weight"], sd[p + "fc1.bias"])), sd[p + "fc2.weight"], sd[p + "fc2.bias"])
    x = F.layer_norm(x, (DIM,), sd[p + "norm.weight"], sd[p + "norm.bias"])
    N = x.shape[0]
    bias = (-slopes[:, None, None] * torch.cdist(coords, coords)[None]).to(x.dtype)
    for l in range(DEPTH):
        b = f"encoder.blocks.{l}."
        h = F.layer_norm(x, (DIM,), sd[b + "residual1.norm.weight"], sd[b + "residual1.norm.bias"])
        q, k, v = (F.linear(h, sd[b + f"residual1.fn.{n}_proj.weight"], sd[b + f"residual1.fn.{n}_proj.bias"]).view(N, HEADS, 64).transpose(0, 1) for n in "qkv")
        w = torch.baddbmm(bias, q, k.transpose(1, 2), alpha=0.125)
        o = (torch.softmax(w, dim=-1) @ v).transpose(0, 1).reshape(N, DIM)
        x = x + sd[b + "residual1.gamma"] * F.linear(o, sd[b + "residual1.fn.proj.weight"], sd[b + "residual1.fn.proj.bias"])
        h = F.layer_norm(x, (DIM,), sd[b + "residual2.norm.weight"], sd[b + "residual2.norm.bias"])
        x1, x2 = F.linear(h, sd[b + "residual2.fn.fc1.weight"], sd[b + "residual2.fn.fc1.bias"]).chunk(2, dim=-1)
        x = x + sd[b + "residual2.gamma"] * F.linear(F.silu(x1) * x2, sd[b + "residual2.fn.fc2.weight"], sd[b + "residual2.fn.fc2.bias"])
    return F.layer_norm(x, (DIM,), sd["enc_norm.weight"], sd["enc_norm.bias"])


def timed(fn, min_s: float = 0.3, max_reps: int = 2000) -> tuple[float, int]:
    """ms per call: warm up, size the loop from one timed call, then device events around `reps` back-to-back calls."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(3, min(max_reps, int(min_s / max(time.perf_counter() - t0, 1e-6))))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 8192, 32768])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ticon_slide_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ticon_slide_bench needs a GPU: a CPU timing says nothing about this path")
    from bench import ClockPowerSampler
    from stamp_amd import _lib, ops
    from stamp_amd.ticon import HipTiconSlide, alibi_slopes

    dev = torch.device("cuda:0")
    sd = random_state_dict()
    model = HipTiconSlide(sd, key=KEY, device=dev, dtype=torch.float16, check=False)
    sd16 = {k: v.to(dev, torch.float16) for k, v in sd.items()}
    slopes = torch.tensor(alibi_slopes(HEADS), device=dev)
    lib, st = _lib.lib(), ops._stream()
    res = {"geometry": {"dim": DIM, "heads": HEADS, "depth": DEPTH, "in_dim": IN_DIM, "operands": "fp16"}, "device": torch.cuda.get_device_name(0), "sizes": []}
    for N in args.sizes:
        g = torch.Generator().manual_seed(N)
        emb = torch.randn(N, IN_DIM, generator=g).to(dev, torch.float16)
        side = int(N ** 0.5) + 1
        cells = torch.randperm(side * side, generator=g)[:N]
        coords = torch.stack([cells // side, cells % side], dim=1).float().to(dev)
        out = model(emb, coords)
        row: dict = {"n_tiles": N, "finite": bool(torch.isfinite(out).all())}
        with ClockPowerSampler(0) as sampler:
            ms, reps = timed(lambda: model(emb, coords), min_s=1.0)
        row.update({"slide_ms": round(ms, 3), "tiles_per_s": round(N / ms * 1e3, 1), "reps": reps, **sampler.summary()})
        qkv = torch.randn(N, 3 * DIM, generator=g).to(dev, torch.float16)
        att = torch.empty(N, DIM, dtype=torch.float16, device=dev)
        flops = 4.0 * N * N * 64 * HEADS
        ms_d, _ = timed(lambda: _lib.check(lib.amds_attention_distbias(qkv.data_ptr(), coords.data_ptr(), slopes.data_ptr(), att.data_ptr(), 1, N, HEADS, _lib.F16, st), "distbias"))
        ms_p, _ = timed(lambda: _lib.check(lib.amds_attention(qkv.data_ptr(), att.data_ptr(), 1, N, HEADS, _lib.F16, st), "attention"))
        row.update({"attn_distbias_ms": round(ms_d, 4), "attn_distbias_tflops": round(flops / ms_d / 1e9, 1), "attn_share_of_slide": round(DEPTH * ms_d / ms, 3),
                    "attn_plain_ms": round(ms_p, 4), "attn_plain_tflops": round(flops / ms_p / 1e9, 1)})
        if N <= 8192:
            with torch.no_grad():
                ref = torch_fp16_forward(emb, coords, sd16, slopes)
                ms_t, _ = timed(lambda: torch_fp16_forward(emb, coords, sd16, slopes), min_s=1.0)
            row.update({"torch_fp16_materialised_ms": round(ms_t, 3), "speedup_vs_torch_fp16": round(ms_t / ms, 2),
                        "rel_l2_vs_torch_fp16": round(((out.float() - ref.float()).norm() / ref.float().norm()).item(), 5)})
            del ref
        else:
            row["torch_fp16_materialised_ms"] = None      # [24, N, N] fp16 bias and weights: 2 x 51 GB at N = 32 768
        print(json.dumps(row), flush=True)
        res["sizes"].append(row)
        del emb, qkv, att, out
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
