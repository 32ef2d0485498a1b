#!/usr/bin/env python3
"""sbx_boba_reorder and sbx_csr_reorder_heatmap on the bench matrix (symmetric RMAT, scale 22, edge factor 13, seed 1:
bench.py's default) and the orderings' effect on it.  Every figure is the median wall time of several calls behind
warm-ups, each ended by a device synchronise:
  boba_coo      BOBA from the COO sbx_csr_to_coo gives
  boba_csr      BOBA from the CSR: the conversion to COO plus the call
  rcm           RCM on the same CSR, for scale
  heatmap_b     the heatmap (identity orders) at b = 3 and b = 1024
and then the bandwidth and profile of the matrix permuted by the identity, Degree, RCM and BOBA orders.  One JSON line.

  python tools/boba_probe.py [--scale 22] [--edge-factor 13] [--reps 9] [--warmup 3]
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


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, round(sorted(times)[len(times) // 2], 3), [round(t, 3) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=13)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rp, col = synth.rmat_symmetric_torch(args.scale, args.edge_factor, seed=1)
    n, nnz = rp.numel() - 1, col.numel()
    row, ccol, _ = ops.csr_to_coo(n, n, rp, col)
    res = dict(input=f"rmat{args.scale}_ef{args.edge_factor}", n=n, nnz=nnz)
    boba, res["boba_coo_ms"], res["boba_coo_times_ms"] = timed(lambda: ops.boba_reorder(row, ccol, n, n), args.reps,
                                                              args.warmup)

    def from_csr():
        r, c, _ = ops.csr_to_coo(n, n, rp, col)
        return ops.boba_reorder(r, c, n, n)

    boba2, res["boba_csr_ms"], res["boba_csr_times_ms"] = timed(from_csr, args.reps, args.warmup)
    assert torch.equal(boba, boba2)
    rcm, res["rcm_ms"], _ = timed(lambda: ops.rcm_reorder(rp, col), args.reps, args.warmup)
    ident = torch.arange(n, dtype=col.dtype, device=col.device)
    for b in (3, 1024):
        _, res[f"heatmap_b{b}_ms"], res[f"heatmap_b{b}_times_ms"] = timed(
            lambda: ops.csr_reorder_heatmap(rp, col, ident, ident, b), args.reps, args.warmup)
    ops.profile_enable(True)
    ops.profile_report()  # (drains what came before)
    ops.boba_reorder(row, ccol, n, n)
    torch.cuda.synchronize()
    res["boba_kernel_ms_by_group"] = {g: round(t, 3) for g, (t, c, b) in ops.profile_report().items() if c}
    ops.csr_reorder_heatmap(rp, col, ident, ident, 3)
    torch.cuda.synchronize()
    res["heatmap_b3_kernel_ms_by_group"] = {g: round(t, 3) for g, (t, c, b) in ops.profile_report().items() if c}
    ops.profile_enable(False)
    quality = {}
    for name, order in [("identity", None), ("degree", ops.degree_reorder(rp)), ("rcm", rcm), ("boba", boba)]:
        if order is None:
            prp, pcol = rp, col
        else:
            prp, pcol, _ = ops.permute_csr(n, n, rp, col, None, order, order)
        quality[name] = dict(bandwidth=ops.csr_bandwidth(prp, pcol), profile=ops.csr_profile(prp, pcol))
        del prp, pcol
    res["quality"] = quality
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
