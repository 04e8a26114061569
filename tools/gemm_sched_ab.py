"""A/B of the production GEMM's LDS-DMA schedules (kernel ids 12 / 13) on the four ViT-L shapes at one 1020-tile chunk, sustained:
every candidate is warmed for ~0.4 s, then 40 launches are timed between two events; two rounds.  python tools/gemm_sched_ab.py
[M [ids]], e.g. `262140 12,14` for the streamed against the one-phase 16-bit epilogue.  `planes` in place of the ids times the encoder's own residual
launch for proj and fc2 (amds_gemm_lnfold_planes on two fp16 planes, LayerScale) in its three forms -- one-phase (AMDS_GEMM_RESID_STREAM=0), streamed
with one tile per workgroup (AMDS_GEMM_PERSIST=0), streamed in the persistent tile walk -- and qkv / fc1 on id 12 three times as the unchanged controls."""
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from stamp_amd import _lib, ops  # noqa: E402

M = int(sys.argv[1]) if len(sys.argv) > 1 else 262140
PLANES = len(sys.argv) > 2 and sys.argv[2] == "planes"
CFGS = (12, 12, 12) if PLANES else tuple(int(c) for c in sys.argv[2].split(",")) if len(sys.argv) > 2 else (12, 13)
shapes = (("qkv", 3072, 1024, _lib.EPI_BIAS), ("proj", 1024, 1024, _lib.EPI_RESIDUAL), ("fc1", 4096, 1024, _lib.EPI_BIAS_GELU),
          ("fc2", 1024, 4096, _lib.EPI_RESIDUAL))
for rnd in range(2):
    for name, N, K, epi in shapes:
        a = torch.randn(M, K, device="cuda").half()
        w = (torch.randn(N, K, device="cuda") / K ** 0.5).half()
        b = torch.zeros(N, device="cuda")
        sc = torch.full((N,), 0.1, device="cuda") if epi == _lib.EPI_RESIDUAL else None
        out = torch.zeros(M, N, device="cuda") if epi == _lib.EPI_RESIDUAL else None
        line = f"{name:5s} N={N} K={K}:"
        planes = PLANES and epi == _lib.EPI_RESIDUAL
        if planes:
            hi, lo, _ = ops.ln_stats_split(torch.randn(M, N, device="cuda"), 1e-6)
            out = None
        for i, cfg in enumerate(CFGS):
            if planes:
                os.environ["AMDS_GEMM_RESID_STREAM"] = "011"[i]
                os.environ["AMDS_GEMM_PERSIST"] = "001"[i]

                def run():
                    ops.gemm_lnfold_planes(a, w, hi, lo, bias=b, scale=sc)
            else:
                def run():
                    ops.gemm(a, w, epi, bias=b, scale=sc, out=out, cfg=cfg)
            t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
            n_warm = max(4, int(0.4 / (2.0 * M * N * K / 1.0e15)))
            for _ in range(n_warm):
                run()
            t0.record()
            for _ in range(40):
                run()
            t1.record(); torch.cuda.synchronize()
            us = t0.elapsed_time(t1) / 40 * 1e3
            if planes:
                del os.environ["AMDS_GEMM_RESID_STREAM"], os.environ["AMDS_GEMM_PERSIST"]
            line += f"  {('one-phase', 'streamed', 'persist')[i] if planes else f'cfg {cfg}'}: {us:7.1f} us {2.0 * M * N * K / us / 1e6:6.0f} TF/s"
        print(line, flush=True)
        del a, w, out
