#!/usr/bin/env python3
"""Records the RCM statistics tests/test_rcm_bu_epilogue_gpu.py compares with: tools/record_rcm_stats.py [out.json]
runs every case of that test three times on the library that is built (SBX_PROBE_LIB=<name>: a variant built by
tools/build_variant.py) and writes the fields edges_scanned, edges_scanned_bottom_up, bfs_levels and bfs_sweeps of the
cases whose three runs agree; the others are listed under "unstable" with what they gave.  It is run on the commit
BEFORE a change to the statistics' bookkeeping: the record is what that change must reproduce."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from sparsebase_amd import capi, ops
if os.environ.get("SBX_PROBE_LIB"):
    capi.LIB_PATH = os.path.join(ROOT, "sparsebase_amd", "lib", f"libsbx_{os.environ['SBX_PROBE_LIB']}.so")
from test_rcm_bu_blocks_gpu import graph, want

FIELDS = ("edges_scanned", "edges_scanned_bottom_up", "bfs_levels", "bfs_sweeps")
CASES = ["n=2047", "n=2048", "n=2049", "big", "empty_blocks", "second_wheel_behind"]
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "rcm_bu_epilogue_stats.json")
stats, unstable = {}, {}
for name in CASES:
    for bits in (32, 64):
        rp, col, _ = graph(name, bits)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        runs = []
        for _ in range(3):
            got, st = ops.rcm_reorder(d(rp), d(col), return_stats=True)
            assert np.array_equal(got.cpu().numpy(), want(name)), (name, bits)
            runs.append({f: int(st[f]) for f in FIELDS})
        key = "%s/%d" % (name, bits)
        if runs[0] == runs[1] == runs[2]:
            stats[key] = runs[0]
        else:
            unstable[key] = runs
        print(key, runs[0] if key in stats else runs, flush=True)
with open(out, "w") as f:
    json.dump({"library": os.environ.get("SBX_PROBE_LIB") or "product", "runs_per_case": 3, "stats": stats,
               "unstable": unstable}, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out, "-", len(stats), "cases,", len(unstable), "unstable")
