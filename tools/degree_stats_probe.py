#!/usr/bin/env python3
"""sbxstat_csr_off_diag_block_nnz and sbxstat_degree_stats on the bench matrix (symmetric RMAT, scale 22, edge factor
13: the matrix bench.py builds), timed with device events behind warm-ups.  One JSON line per measurement.

OffDiagBlockNNZ with h = w in 8, 64, 4096 against sbx_csr_bandwidth on the same arrays in the same process, the two
alternating (A B A B ...): sbx_csr_bandwidth reads the same bytes and does strictly more per entry, so the new call must
not be slower than it beyond the spread that two runs of sbx_csr_bandwidth alone (its even against its odd
repetitions) show.  The achieved share of the 8 TB/s HBM peak is taken from 4 nnz bytes.

Degree statistics on the bench matrix's row_ptr with and without SBXSTAT_MEDIAN and SBXSTAT_LOG.  The hot-bin folding
is a compile-time constant: run the probe once more with SBX_PROBE_LIB=<variant> for a library built by
  python tools/build_variant.py nofold sbx_stats.hip -DSBXSTAT_FOLD=0

  python tools/degree_stats_probe.py [--scale 22] [--edge-factor 13] [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebase_amd import capi  # noqa: E402
if os.environ.get("SBX_PROBE_LIB"):  # a variant built by tools/build_variant.py
    capi.LIB_PATH = os.path.join(ROOT, "sparsebase_amd", "lib", f"libsbx_{os.environ['SBX_PROBE_LIB']}.so")
from sparsebase_amd import ops, synth  # noqa: E402

HBM_PEAK = 8e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=13)
    ap.add_argument("--blocks", type=int, nargs="*", default=[8, 64, 4096])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    lib = os.environ.get("SBX_PROBE_LIB") or "product"
    rp, col = synth.rmat_symmetric_torch(args.scale, args.edge_factor, seed=1)
    n, nnz = rp.numel() - 1, col.numel()
    for b in args.blocks:
        off = lambda: ops.csr_off_diag_block_nnz(rp, col, n, b, b)
        bw = lambda: ops.csr_bandwidth(rp, col)
        for _ in range(args.warmup):
            count, band = off(), bw()
        torch.cuda.synchronize()
        t_off, t_bw = [], []
        for _ in range(args.reps):
            ms, got = timed(off)
            assert got == count
            t_off.append(ms)
            ms, got = timed(bw)
            assert got == band
            t_bw.append(ms)
        so, sb = stats(t_off), stats(t_bw)
        even, odd = stats(t_bw[0::2]), stats(t_bw[1::2])
        spread = abs(even["median_ms"] - odd["median_ms"])
        print(json.dumps({"probe": "off_diag_block_nnz", "lib": lib, "n": n, "nnz": nnz, "h": b, "w": b, "count": count,
                          "off_diag": so, "csr_bandwidth": sb, "csr_bandwidth_even_odd_spread_ms": round(spread, 4),
                          "not_slower": so["median_ms"] <= sb["median_ms"] + spread,
                          "hbm_share": round(4 * nnz / (so["median_ms"] * 1e-3) / HBM_PEAK, 4), "reps": args.reps}), flush=True)
    for median, log in ((True, True), (False, True), (True, False), (False, False)):
        call = lambda: ops.degree_stats(rp, median=median, log=log)
        for _ in range(args.warmup):
            ref = call()
        torch.cuda.synchronize()
        t = []
        for _ in range(args.reps):
            ms, got = timed(call)
            assert got == ref
            t.append(ms)
        print(json.dumps({"probe": "degree_stats", "lib": lib, "n": n, "median": median, "log": log, **stats(t),
                          "max": ref["max"], "median_lo": ref["median_lo"], "median_hi": ref["median_hi"],
                          "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
