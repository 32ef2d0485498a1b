#!/usr/bin/env python3
"""sbx_csr_triangle_count in both modes and both directions, on a symmetric RMAT graph and on the banded C5 shape:
the median wall time of several calls behind a warm-up (the call is synchronous: it returns the count), with the
work counted from the shapes.  One JSON line per (input, mode, direction).

  reference mode  searched = nonzeros (node, v) with node < v < n, each one search in row v (directed: two)
  exact mode      items = oriented edges (undirected: (deg, id) order) or arcs a -> b with a < b (directed);
                  lookups = the entries of the shorter list of every item, each one search in the other list

  python tools/triangle_probe.py [--scale 20] [--edge-factor 16] [--banded-n 4194304] [--reps 7] [--warmup 3]
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


def _simple(n, a, b):
    ok = (b >= 0) & (b < n) & (a != b)
    keys = torch.unique(a[ok] * n + b[ok])  # sorted
    off = torch.searchsorted(keys, torch.arange(n + 1, device=keys.device) * n)
    return keys, off


def work(rp, col, directed, exact):
    n = rp.numel() - 1
    row = torch.repeat_interleave(torch.arange(n, device=rp.device), (rp[1:] - rp[:-1]).to(torch.int64))
    c = col.to(torch.int64)
    if not exact:
        q = int(((c > row) & (c < n)).sum())
        return dict(searched=q, searches=q * (2 if directed else 1))
    if directed:
        arcs, out_off = _simple(n, row, c)
        a, b = arcs // n, arcs % n
        rev = torch.sort(b * n + a).values
        in_off = torch.searchsorted(rev, torch.arange(n + 1, device=rp.device) * n)
        fw = a < b
        a, b = a[fw], b[fw]
        ol = out_off[b + 1] - torch.searchsorted(arcs, b * n + a + 1)
        il = in_off[a + 1] - torch.searchsorted(rev, a * n + a + 1)
        return dict(items=int(fw.sum()), lookups=int(torch.minimum(ol, il).sum()))
    sym, off = _simple(n, torch.cat([row, c]), torch.cat([c, row]))
    u, v = sym // n, sym % n
    deg = off[1:] - off[:-1]
    keep = (deg[u] < deg[v]) | ((deg[u] == deg[v]) & (u < v))
    ori = sym[keep]
    ooff = torch.searchsorted(ori, torch.arange(n + 1, device=rp.device) * n)
    u, v = ori // n, ori % n
    lu, lv = ooff[u + 1] - ooff[u], ooff[v + 1] - ooff[v]
    return dict(items=int(ori.numel()), lookups=int(torch.minimum(lu, lv).sum()))


def measure(name, rp, col, directed, exact, reps, warmup):
    for _ in range(warmup):
        count = ops.csr_triangle_count(rp, col, directed=directed, exact=exact)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = ops.csr_triangle_count(rp, col, directed=directed, exact=exact)
        times.append((time.perf_counter() - t0) * 1e3)
        assert got == count, "the count changed between calls"
    ms = sorted(times)[len(times) // 2]
    w = work(rp, col, directed, exact)
    rate = (w["lookups"] if exact else w["searches"]) / ms / 1e6
    print(json.dumps(dict(input=name, mode="exact" if exact else "reference", directed=directed, n=rp.numel() - 1,
                          nnz=col.numel(), max_deg=int((rp[1:] - rp[:-1]).max()), count=count, **w, ms=round(ms, 3),
                          g_per_s=round(rate, 2), times_ms=[round(t, 3) for t in times])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--banded-n", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    inputs = [(f"rmat{args.scale}_ef{args.edge_factor}", lambda: synth.rmat_symmetric_torch(args.scale, args.edge_factor,
                                                                                             seed=1)),
              (f"banded_w64_n{args.banded_n}", lambda: synth.banded_symmetric_torch(args.banded_n, 64, per_row=12,
                                                                                    seed=2))]
    for name, make in inputs:
        rp, col = make()
        for exact in (False, True):
            for directed in (False, True):
                measure(name, rp, col, directed, exact, args.reps, args.warmup)
        del rp, col


if __name__ == "__main__":
    main()
