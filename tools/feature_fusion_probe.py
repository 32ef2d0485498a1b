#!/usr/bin/env python3
"""The fused feature entry points of include/sbfx.h against the two calls each replaces, on the bench matrix (symmetric
RMAT, scale 22, edge factor 13: the matrix bench.py builds), timed with device events behind warm-ups.  One JSON line
per pair.

  bandwidth_profile             sbfx_csr_bandwidth_profile            against sbx_csr_bandwidth then sbx_csr_profile
  degrees_degree_distribution   sbfx_csr_degrees_degree_distribution  against sbx_csr_degrees then
                                                                      sbx_csr_degree_distribution (float32 and float64)

The fused call and the pair alternate in the same process on the same arrays (A B A B ...).  The yardstick is the pair
in the same run; the margin is the spread between the medians of the pair's even and odd repetitions.  `faster` is
true only if the fused call's median beats the pair's by more than that margin.

  python tools/feature_fusion_probe.py [--scale 22] [--edge-factor 13] [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebase_amd import ops, synth  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4)}


def compare(name, fused, pair, same, args, **extra):
    for _ in range(args.warmup):
        want_f, want_p = fused(), pair()
    torch.cuda.synchronize()
    assert same(want_f, want_p), name
    t_f, t_p = [], []
    for _ in range(args.reps):
        ms, _ = timed(fused)
        t_f.append(ms)
        ms, _ = timed(pair)
        t_p.append(ms)
    sf, sp = stats(t_f), stats(t_p)
    spread = abs(stats(t_p[0::2])["median_ms"] - stats(t_p[1::2])["median_ms"])
    print(json.dumps({"probe": name, **extra, "fused": sf, "pair": sp, "pair_even_odd_spread_ms": round(spread, 4),
                      "faster": sf["median_ms"] < sp["median_ms"] - spread,
                      "fused_over_pair": round(sf["median_ms"] / sp["median_ms"], 4), "reps": args.reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=13)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    rp, col = synth.rmat_symmetric_torch(args.scale, args.edge_factor, seed=1)
    n, nnz = rp.numel() - 1, col.numel()
    compare("bandwidth_profile", lambda: ops.csr_bandwidth_profile(rp, col),
            lambda: (ops.csr_bandwidth(rp, col), ops.csr_profile(rp, col)), lambda f, p: f == p, args, n=n, nnz=nnz)
    for dt in (torch.float32, torch.float64):
        compare("degrees_degree_distribution", lambda: ops.csr_degrees_degree_distribution(rp, nnz, dtype=dt),
                lambda: (ops.csr_degrees(rp), ops.csr_degree_distribution(rp, nnz, dtype=dt)),
                lambda f, p: all(torch.equal(a, b) for a, b in zip(f, p)), args, n=n, nnz=nnz,
                feature_type=str(dt).replace("torch.", ""))


if __name__ == "__main__":
    main()
