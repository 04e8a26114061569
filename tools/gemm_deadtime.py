"""Per-tile dead time of the production GEMM (gemm_4w16.h), from in-kernel s_memtime stamps of a TRACE build:

    make TRACE=1 OBJ=build/obj_trace LIB=build/trace/libamdstamp_trace.so
    AMDSTAMP_LIB=build/trace/libamdstamp_trace.so python tools/gemm_deadtime.py [M]

Lane 0 of wave 0 stamps every output tile at entry / K tile 0 landed / behind the last MFMA unit / exit and records the hardware id of its CU.  For
qkv (N 3072, K 1024, BIAS) and fc1 (N 4096, K 1024, BIAS_GELU) at M = 262 140 this prints, in microseconds at the clock measured inside the kernel,
median and p90 of
  one tile per workgroup (AMDS_GEMM_PERSIST=0), successive workgroups paired on their CU:
    (a) last MFMA -> exit of a workgroup          (b) exit of workgroup i -> K tile 0 landed of workgroup i + 1
  persistent (kernel id 16), successive tiles of a workgroup:
    (a') last MFMA -> the epilogue's last store issued          (c) last MFMA of tile i -> first fragment read of tile i + 1 (= (a) + (b) of this form)
For the RESIDUAL planes launch (amds_gemm_lnfold_planes: proj N 1024 K 1024, fc2 N 1024 K 4096, LayerScale, one tile per workgroup; `resid` as the
second argument runs only these; AMDS_GEMM_RESID_STREAM=0 in the environment for the one-phase epilogue) the exit stamp is taken when the tile's last store
has COMPLETED, and besides (a) and (b) this prints
    (s) the spread of the epilogue's start (last MFMA, on the 100 MHz s_memrealtime clock all XCDs share) across the CUs of one round of tiles.
The stamps are scalar-memory clock reads kept in registers and written once per tile; a TRACE build is never the product."""
import ctypes
import os
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from stamp_amd import _lib, ops  # noqa: E402

M = int(sys.argv[1]) if len(sys.argv) > 1 else 262140
SHAPES = (("qkv", 3072, 1024, _lib.EPI_BIAS), ("fc1", 4096, 1024, _lib.EPI_BIAS_GELU))
RESID_SHAPES = (("proj", 1024, 1024), ("fc2", 1024, 4096))
if len(sys.argv) > 2 and sys.argv[2] == "resid":
    SHAPES = ()


def records(cfg, a, w, b, epi, persist):
    if persist:
        os.environ.pop("AMDS_GEMM_PERSIST", None)
    else:
        os.environ["AMDS_GEMM_PERSIST"] = "0"
    tiles = -(-a.shape[0] // 256) * (w.shape[0] // 256)
    buf = torch.zeros(tiles * 8 + 2048 * 8, dtype=torch.int64, device="cuda")
    out = torch.empty(a.shape[0], w.shape[0], dtype=a.dtype, device="cuda")
    for _ in range(20):                                    # warm: clocks and caches as in a sustained run
        ops.gemm(a, w, epi, bias=b, out=out, cfg=cfg)
    buf.zero_()
    ops.gemm(a, w, epi, bias=b, out=out, pos=buf.view(torch.float32), cfg=cfg)
    torch.cuda.synchronize()
    r = buf.cpu().numpy().astype(np.uint64).reshape(-1, 8)
    return r[r[:, 0] != 0]


def stats(x):
    return f"median {np.median(x):6.2f}  p90 {np.percentile(x, 90):6.2f}  (n = {len(x)})"


for name, N, K, epi in SHAPES:
    a = torch.randn(M, K, device="cuda").half()
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).half()
    b = torch.randn(N, device="cuda")
    print(f"{name}: M={M} N={N} K={K}")
    # ---- one tile per workgroup
    r = records(12, a, w, b, epi, persist=False)
    mhz = float(np.median((r[:, 3] - r[:, 0]).astype(np.float64) / np.maximum((r[:, 7] - r[:, 6]).astype(np.float64), 1.0))) * 100.0
    us = 1.0 / mhz
    cu = (r[:, 4] >> np.uint64(8)) & np.uint64(0xFF) | ((r[:, 4] >> np.uint64(32)) & np.uint64(0xF)) << np.uint64(8)      # CU / SH / SE bits of HW_ID, XCC_ID
    a_int, b_int = [], []
    for key in np.unique(cu):
        q = r[cu == key]
        q = q[np.argsort(q[:, 0])]
        a_int += list((q[:, 3] - q[:, 2]).astype(np.float64) * us)
        b_int += list((q[1:, 1].astype(np.int64) - q[:-1, 3].astype(np.int64)).astype(np.float64) * us)
    print(f"  one tile per workgroup ({len(r)} workgroups on {len(np.unique(cu))} CUs, {mhz:.0f} MHz in the kernel)")
    print(f"    (a) last MFMA -> exit                         {stats(np.array(a_int))}")
    print(f"    (b) exit -> K tile 0 of the next workgroup    {stats(np.array(b_int))}")
    print(f"    whole tile, entry -> exit                     {stats((r[:, 3] - r[:, 0]).astype(np.float64) * us)}")
    # ---- persistent
    r = records(16, a, w, b, epi, persist=True)
    G = (torch.cuda.get_device_properties(0).multi_processor_count // 8) * 8
    tiles = -(-M // 256) * (N // 256)
    G = min(G, tiles)
    rounds = -(-tiles // G)
    rr = np.zeros((G * rounds, 8), dtype=np.uint64)
    # records are indexed (workgroup, round); rebuild that from the tile index: tile = workgroup + round * G
    wg, rnd = r[:, 5].astype(np.int64) % G, r[:, 5].astype(np.int64) // G
    rr[wg * rounds + rnd] = r
    rr = rr.reshape(G, rounds, 8)
    ok = (rr[:, 1:, 0] != 0) & (rr[:, :-1, 0] != 0)
    ap = (rr[:, :, 3].astype(np.int64) - rr[:, :, 2].astype(np.int64))[rr[:, :, 0] != 0].astype(np.float64) * us
    c = (rr[:, 1:, 1].astype(np.int64) - rr[:, :-1, 2].astype(np.int64))[ok].astype(np.float64) * us
    print(f"  persistent ({G} workgroups x {rounds} rounds)")
    print(f"    (a') last MFMA -> last store issued           {stats(ap)}")
    print(f"    (c) last MFMA -> first read of the next tile  {stats(c)}")
    print(f"    whole tile, first read -> first read          {stats((rr[:, 1:, 1].astype(np.int64) - rr[:, :-1, 1].astype(np.int64))[ok].astype(np.float64) * us)}")
    del a, w, b


def resid_records(a, w, hi, lo, b, sc):
    tiles = -(-a.shape[0] // 256) * (w.shape[0] // 256)
    buf = torch.zeros(tiles * 8 + 2048 * 8, dtype=torch.int64, device="cuda")
    set_buf = _lib.lib().amds_gemm_trace_buffer          # TRACE builds only
    set_buf.restype, set_buf.argtypes = None, [ctypes.c_void_p]
    for _ in range(20):
        ops.gemm_lnfold_planes(a, w, hi, lo, bias=b, scale=sc)
    set_buf(buf.data_ptr())
    ops.gemm_lnfold_planes(a, w, hi, lo, bias=b, scale=sc)
    torch.cuda.synchronize()
    set_buf(None)
    r = buf.cpu().numpy().astype(np.uint64).reshape(-1, 8)
    return r[r[:, 0] != 0]


for name, N, K in RESID_SHAPES:
    a = torch.randn(M, K, device="cuda").half()
    w = (torch.randn(N, K, device="cuda") / K ** 0.5).half()
    b = torch.randn(N, device="cuda")
    sc = torch.full((N,), 0.1, device="cuda")
    hi, lo, _ = ops.ln_stats_split(torch.randn(M, N, device="cuda"), 1e-6)
    form = "one-phase" if os.environ.get("AMDS_GEMM_RESID_STREAM", "1") == "0" else "streamed"
    print(f"{name}: M={M} N={N} K={K}  RESIDUAL on two fp16 planes, LayerScale, {form} epilogue")
    os.environ["AMDS_GEMM_RESID_PERSIST"] = "0"          # one tile per workgroup: the pairing below is by CU
    r = resid_records(a, w, hi, lo, b, sc)
    mhz = float(np.median((r[:, 3] - r[:, 0]).astype(np.float64) / np.maximum((r[:, 7] - r[:, 6]).astype(np.float64), 1.0))) * 100.0
    us = 1.0 / mhz
    cu = (r[:, 4] >> np.uint64(8)) & np.uint64(0xFF) | ((r[:, 4] >> np.uint64(32)) & np.uint64(0xF)) << np.uint64(8)
    a_int, b_int, starts = [], [], {}
    for key in np.unique(cu):
        q = r[cu == key]
        q = q[np.argsort(q[:, 0])]
        epi = (q[:, 3] - q[:, 2]).astype(np.float64) * us
        a_int += list(epi)
        b_int += list((q[1:, 1].astype(np.int64) - q[:-1, 3].astype(np.int64)).astype(np.float64) * us)
        for rnd, t in enumerate(q[:, 7].astype(np.float64) * 0.01 - epi):      # exit on the shared clock, less the epilogue
            starts.setdefault(rnd, []).append(t)
    full = [np.array(v) for v in starts.values() if len(v) == len(np.unique(cu))]
    print(f"  one tile per workgroup ({len(r)} workgroups on {len(np.unique(cu))} CUs, {mhz:.0f} MHz in the kernel)")
    print(f"    (a) last MFMA -> last store completed          {stats(np.array(a_int))}")
    print(f"    (b) exit -> K tile 0 of the next workgroup    {stats(np.array(b_int))}")
    print(f"    K loop, K tile 0 landed -> last MFMA          {stats((r[:, 2] - r[:, 1]).astype(np.float64) * us)}")
    print(f"    whole tile, entry -> exit                     {stats((r[:, 3] - r[:, 0]).astype(np.float64) * us)}")
    print(f"    (s) epilogue start over the CUs of a round: p90 - p10 {stats(np.array([np.percentile(v, 90) - np.percentile(v, 10) for v in full]))}")
    print(f"        max - min                                        {stats(np.array([v.max() - v.min() for v in full]))}")
    del a, w, b, hi, lo
