#!/usr/bin/env python3
"""How far below the MIL `vit` trainer do its feeds sit?  One process, one GPU, a synthetic cohort of feature files:

    leg "dataloader0" / "dataloaderN"   bags.tile_bag_dataloader (the reference's feed) with 0 / N workers
    leg "resident"                      cohort.ResidentCohort.train_batches (features in HBM, one gather launch per batch); `--sampler device` draws the
                                        epoch's bags with one amds_bag_plan launch instead of the host's per-patient torch.randperm
    leg "ceiling"                       the trainer alone: the same number of steps on ONE pre-built device batch

Every leg runs `fit`'s training loop (HipMilVitTrainer.step per batch, the loss read on the host after every step) for one epoch and reports epoch bags/s;
the legs are alternated `--rounds` times after one warm-up epoch each.  Also: the cohort's load time and rate, its bytes in HBM, the host time of one epoch's
index plan, and the gather alone (HIP events, median) with its byte rate next to the 6.29 TB/s copy rate of DESIGN.md 4.17.  Writes one JSON file.

The worker processes of the N-worker loader are started (one host-only warm-up epoch) BEFORE this process touches the GPU, so that no worker ever has the device
open."""
from __future__ import annotations

import argparse
import json
import math
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def write_cohort(d: Path, patients: int, lo: int, hi: int, Fd: int, seed: int):
    """`patients` single-slide patients, tile counts log-uniform on [lo, hi], fp16 features cut from one random pool (their values do not matter here)."""
    from stamp_amd import h5io
    from stamp_amd.bags import PatientData
    rng = np.random.default_rng(seed)
    pool = rng.standard_normal((hi + 4096, Fd), dtype=np.float32).astype(np.float16)
    counts = np.exp(rng.uniform(math.log(lo), math.log(hi), patients)).round().astype(int).clip(lo, hi)
    pdata = []
    for i, n in enumerate(counts.tolist()):
        o = int(rng.integers(0, 4096))
        coords = np.stack([rng.integers(0, 200, n), rng.integers(0, 200, n)], 1).astype(np.float32) * 256.0
        p = d / f"patient_{i:04d}.h5"
        h5io.write_tile_features(p, pool[o:o + n], coords, extractor="synthetic", tile_size_um=256.0, tile_size_px=224, code_hash="0", stamp_version="2.4.0")
        pdata.append(PatientData(ground_truth="pos" if i % 2 else "neg", feature_files=[p]))
    return pdata, counts.tolist()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--patients", type=int, default=256)
    ap.add_argument("--min-tiles", type=int, default=256)
    ap.add_argument("--max-tiles", type=int, default=16384)
    ap.add_argument("--feats", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--bag", type=int, default=512)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="high")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sampler", choices=("torch", "device"), default="torch", help="who draws the resident leg's bags: the host generator or amds_bag_plan")
    ap.add_argument("--dir", default=None, help="where the synthetic files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cohort_feed_bench.json"))
    a = ap.parse_args()

    import torch

    from stamp_amd import bags as B
    from stamp_amd import h5io
    tmp =Path(a.dir) if a.dir else Path(tempfile.mkdtemp(prefix="cohort_feed_"))
    tmp.mkdir(parents=True, exist_ok=True)
    try:
        t0 = time.perf_counter()
        pdata, counts = write_cohort(tmp, a.patients, a.min_tiles, a.max_tiles, a.feats, a.seed)
        file_bytes = sum(p.stat().st_size for pd in pdata for p in pd.feature_files)
        print(f"wrote {a.patients} files, {sum(counts)} tiles, {file_bytes / 1e9:.2f} GB in {time.perf_counter() - t0:.1f} s", flush=True)
        torch.manual_seed(a.seed)
        loaders = {}
        for w in (a.workers, 0):          # the worker processes first, while this process has not opened the GPU
            dl, cats = B.tile_bag_dataloader(patient_data=pdata, bag_size=a.bag, task="classification", batch_size=a.batch, shuffle=True, num_workers=w, transform=None)
            loaders[w] = dl
        t0 = time.perf_counter()
        host_only = sum(b[0].shape[0] for b in loaders[a.workers])
        print(f"{a.workers}-worker loader: host-only warm-up epoch, {host_only} bags in {time.perf_counter() - t0:.1f} s", flush=True)

        from stamp_amd import ops
        from stamp_amd.cohort import ResidentCohort
        from stamp_amd.mil import VisionTransformer
        from stamp_amd.mil_train import HipMilVitTrainer
        if not torch.cuda.is_available():
            raise RuntimeError("this measurement needs the GPU (there is no CPU figure to report)")
        dev = torch.device("cuda:0")
        torch.set_float32_matmul_precision(a.precision)
        model = VisionTransformer(dim_output=2, dim_input=a.feats, dim_model=512, n_layers=2, n_heads=8, dim_feedforward=512, dropout=0.25, use_alibi=False)
        trainer = HipMilVitTrainer(model, device=dev, total_steps=100000, sched_interval="step", precision=a.precision)
        cohort = ResidentCohort(pdata, task="classification", categories=cats, device=dev)
        resident = cohort.train_batches(a.batch, a.bag, shuffle=True, sampler=a.sampler, seed=a.seed)
        fixed = next(iter(resident()))
        steps = math.ceil(a.patients / a.batch)
        feeds = {f"dataloader{a.workers}": lambda: loaders[a.workers], "dataloader0": lambda: loaders[0], "resident": resident,
                 "ceiling": lambda: (fixed for _ in range(steps))}

        def epoch(feed) -> float:          # `fit`'s training loop
            torch.cuda.synchronize()
            t = time.perf_counter()
            n = 0
            for bags, coords, _sizes, targets in feed():
                loss, _ = trainer.step(bags.to(dev), targets, None, coords=None if coords is None else coords.to(dev))
                float(loss)
                n += bags.shape[0]
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t)

        rates = {k: [] for k in feeds}
        for k, f in feeds.items():
            epoch(f)                       # warm-up: code objects, workspaces, the workers' file handles
        for r in range(a.rounds):
            for k, f in feeds.items():
                rates[k].append(round(epoch(f), 1))
            print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.0f}" for k, v in rates.items()) + " bags/s", flush=True)

        # one epoch's index plan on the host; the gather alone
        t0 = time.perf_counter()
        idx, _ = cohort.plan_indices(torch.randperm(len(cohort)).tolist(), a.bag)
        plan_ms = (time.perf_counter() - t0) * 1e3
        idx = idx[:a.batch].to(dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
        for _ in range(5):
            ops.bag_batch_gather(cohort.feats, cohort.coords, idx, torch.float32)
        for s, e in ev:
            s.record()
            ops.bag_batch_gather(cohort.feats, cohort.coords, idx, torch.float32)
            e.record()
        torch.cuda.synchronize()
        gather_us = statistics.median(s.elapsed_time(e) for s, e in ev) * 1e3
        # one epoch's index plan on the device: the upload of the patient order + the amds_bag_plan launch, host time until the plan is there
        plan_dev = []
        for _ in range(20):
            order = torch.randperm(len(cohort))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.bag_plan(cohort._offsets_dev, order.to(dev), a.bag, a.seed, 0)
            torch.cuda.synchronize()
            plan_dev.append((time.perf_counter() - t0) * 1e3)
        item = cohort.feats.element_size()
        gather_bytes = idx.numel() * (a.feats * (item + 4) + 8 + 16)          # a feature row read and written as fp32, its index, its coordinates in and out
        pairs = list(zip(rates["resident"], rates[f"dataloader{a.workers}"]))
        res = {
            "what": "epoch bags/s of HipMilVitTrainer (vit head, fit's loop: one step per batch, the loss read after every step) fed four ways; one process, one MI355X",
            "cohort": {"patients": a.patients, "tiles": "log-uniform %d-%d" % (a.min_tiles, a.max_tiles), "total_tiles": int(sum(counts)), "features": a.feats,
                       "file_dtype": "float16", "file_bytes": file_bytes, "h5_backend": h5io.backend()},
            "batch": a.batch, "bag_size": a.bag, "precision": a.precision, "rounds": a.rounds, "epoch_bags_per_s": rates,
            "median_bags_per_s": {k: statistics.median(v) for k, v in rates.items()},
            "resident_load": {"seconds": round(cohort.load_seconds, 3), "GB_per_s": round(cohort.nbytes / cohort.load_seconds / 1e9, 3), "hbm_bytes": cohort.nbytes,
                              "store_dtype": str(cohort.dtype)},
            "sampler": a.sampler,
            "epoch_ms": {k: round(1e3 * a.patients / statistics.median(v), 3) for k, v in rates.items()},
            "epoch_plan_host_ms": round(plan_ms, 2),
            "epoch_plan_device_ms": round(statistics.median(plan_dev), 3),
            "gather": {"us_per_batch_median": round(gather_us, 2), "bytes_per_batch": gather_bytes, "GB_per_s": round(gather_bytes / gather_us / 1e3, 1),
                       "copy_rate_GB_per_s_design_4_17": 6290},
            "condition_resident_ge_dataloader_workers_every_pair": all(x >= y for x, y in pairs),
            "resident_over_ceiling": round(statistics.median(rates["resident"]) / statistics.median(rates["ceiling"]), 3),
        }
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res))
        return 0 if res["condition_resident_ge_dataloader_workers_every_pair"] else 1
    finally:
        loaders = None                     # (ends the persistent worker processes)
        if not a.dir:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    raise SystemExit(main())
