#!/usr/bin/env python3
"""sbx_slashburn_reorder in both hub modes on a symmetric RMAT graph (scale 18 and 20) and on the banded C5 shape
(n = 2^22, half-bandwidth 64), k = ceil(0.005 n): the median wall time of several calls behind warm-ups (the call is
synchronous), the call's statistics, and the kernel launches of one more call under the library's profiler, by kernel
group.  One JSON line per (input, mode).

  python tools/slashburn_probe.py [--scales 18 20] [--edge-factor 16] [--banded-n 4194304] [--reps 7] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebase_amd import ops, synth  # noqa: E402


def measure(name, rp, col, greedy, reps, warmup):
    n = rp.numel() - 1
    k = -(-n * 5 // 1000)
    for _ in range(warmup):
        ref, st = ops.slashburn_reorder(rp, col, k, greedy=greedy, return_stats=True)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = ops.slashburn_reorder(rp, col, k, greedy=greedy)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(got, ref), "the order changed between calls"
    ms = sorted(times)[len(times) // 2]
    ops.profile_enable(True)
    ops.profile_report()  # (drains what came before)
    ops.slashburn_reorder(rp, col, k, greedy=greedy)
    torch.cuda.synchronize()
    prof = ops.profile_report()
    ops.profile_enable(False)
    launches = {g: c for g, (t, c, b) in prof.items() if c}
    kernel_ms = {g: round(t, 3) for g, (t, c, b) in prof.items() if c}
    print(json.dumps(dict(input=name, mode="greedy" if greedy else "default", n=n, nnz=col.numel(), k=k, **st,
                          ms=round(ms, 3), launches=sum(launches.values()), launches_by_group=launches,
                          kernel_ms_by_group=kernel_ms, times_ms=[round(t, 3) for t in times])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="*", default=[18, 20])
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--banded-n", type=int, default=1 << 22)
    ap.add_argument("--modes", nargs="*", default=["default", "greedy"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    inputs = [(f"rmat{s}_ef{args.edge_factor}", lambda s=s: synth.rmat_symmetric_torch(s, args.edge_factor, seed=1))
              for s in args.scales]
    if args.banded_n:
        inputs.append((f"banded_w64_n{args.banded_n}",
                       lambda: synth.banded_symmetric_torch(args.banded_n, 64, per_row=12, seed=2)))
    for name, make in inputs:
        rp, col = make()
        for mode in args.modes:
            measure(name, rp, col, mode == "greedy", args.reps, args.warmup)
        del rp, col


if __name__ == "__main__":
    main()
