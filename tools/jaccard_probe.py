#!/usr/bin/env python3
"""sbx_csr_jaccard_weights on a symmetric RMAT graph and on the banded C5 shape: the median of several timed calls
behind a warm-up, with the kept edges (rule 1 of the feature) and the lookups they make (deg(u) searches per kept
edge).  One JSON line per input.

  python tools/jaccard_probe.py [--scale 20] [--reps 7] [--warmup 3] [--banded-n 4194304]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebase_amd import ops, synth  # noqa: E402


def kept_and_lookups(rp, col):
    n = rp.numel() - 1
    deg = (rp[1:] - rp[:-1]).to(torch.int64)
    u = torch.repeat_interleave(torch.arange(n, device=rp.device), deg)
    v = col.to(torch.int64)
    du, dv = deg[u], deg[v]
    kept = ~((dv < du) | ((dv == du) & (v > u)))
    return int(kept.sum()), int(du[kept].sum())


def measure(name, rp, col, reps, warmup):
    for _ in range(warmup):
        ops.csr_jaccard_weights(rp, col)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.csr_jaccard_weights(rp, col)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    ms = sorted(times)[len(times) // 2]
    kept, lookups = kept_and_lookups(rp, col)
    print(json.dumps(dict(input=name, n=rp.numel() - 1, nnz=col.numel(), max_deg=int((rp[1:] - rp[:-1]).max()),
                          kept=kept, lookups=lookups, ms=round(ms, 3), glookups_s=round(lookups / ms / 1e6, 2),
                          times_ms=[round(t, 3) for t in times])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--banded-n", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rp, col = synth.rmat_symmetric_torch(args.scale, args.edge_factor, seed=1)
    measure(f"rmat{args.scale}_ef{args.edge_factor}", rp, col, args.reps, args.warmup)
    del rp, col
    rp, col = synth.banded_symmetric_torch(args.banded_n, 64, per_row=12, seed=2)
    measure(f"banded_w64_n{args.banded_n}", rp, col, args.reps, args.warmup)


if __name__ == "__main__":
    main()
