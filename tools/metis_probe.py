#!/usr/bin/env python3
"""METIS graph files on the device: sbgr_metis_parse (vertex lines resident in HBM -> COO in (row, col) order, row
offsets) and sbgr_metis_format (CSR -> vertex lines), on a generated symmetric graph of about `entries` entries with
float32 edge weights, and beside them sbx_edge_list_parse on an edge list of the same entries: the nearest yardstick
the library has (per-entry parsing without lines).

One JSON line: the text sizes, parse / format / edge-list parse ms (medians of warm calls, each ending in a device
synchronise, with minimum and maximum) and text GB/s.  The graph's text is written by the formatter itself at precision
9, and the parse is checked to give the arrays back.

  tools/metis_probe.py [entries] [--hub]      (run it under `timeout`: it has no limit of its own)
  --hub: one vertex is adjacent to four fifths of the others (n = entries / 16 vertices; its line holds entries / 20
         neighbours, a twentieth of the entries)

The clock is the host's (perf_counter up to a device synchronise), not device events as in the sibling probes: both
entry points are synchronous, they read counts and lengths back between their kernels, so the host's wait is part of
what a caller pays, and events on the stream would leave it out.
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebase_amd import ops  # noqa: E402

REPS = 7


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    entries = int(args[0]) if args else 10_000_000
    assert torch.cuda.is_available(), "the probe measures the GPU path: there is nothing to fall back to"
    n = max(2, entries // 16)
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randint(0, n, (entries // 2,), device="cuda", generator=g)
    b = torch.randint(0, n, (entries // 2,), device="cuda", generator=g)
    if "--hub" in sys.argv:
        k = entries // 20
        a[:k], b[:k] = 0, torch.randperm(n - 1, device="cuda", generator=g)[:k] + 1
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    key = torch.unique(lo * n + hi)
    key = key[key // n != key % n]
    lo, hi = (key // n).to(torch.int32), (key % n).to(torch.int32)
    w = torch.randn(lo.numel(), device="cuda", generator=g)
    row, col, val = torch.cat([lo, hi]), torch.cat([hi, lo]), torch.cat([w, w])
    ops.coo_sort_(n, n, row, col, val)
    rp, col, val = ops.coo_to_csr(n, n, row, col, val, rows_sorted=True)
    m = lo.numel()
    text = ops.metis_format(rp, col, val, precision=9, edge_weights=True)
    fmt_ms = timed(lambda: ops.metis_format(rp, col, val, precision=9, edge_weights=True))
    parse_ms = timed(lambda: ops.metis_parse(text, n, m, 1, 1, True, torch.int32, torch.float32))
    _, r2, c2, v2, _, rp2 = ops.metis_parse(text, n, m, 1, 1, True, torch.int32, torch.float32)
    same = bool(torch.equal(c2, col) and torch.equal(v2.view(torch.int32), val.view(torch.int32)) and torch.equal(rp2, rp))
    edges = ops.text_format_coordinate(row, col, val, index_base=0, precision=9)
    edge_ms = timed(lambda: ops.edge_list_parse(edges, weighted=True, read_undirected=False, value_dtype=torch.float32))
    print(json.dumps(dict(n=n, entries=2 * m, hub="--hub" in sys.argv, graph_text_mb=round(text.numel() / 1e6, 1),
                          edge_list_mb=round(edges.numel() / 1e6, 1), parse_ms=parse_ms, format_ms=fmt_ms,
                          edge_list_parse_ms=edge_ms, parse_text_gb_s=round(text.numel() / parse_ms[0] / 1e6, 2),
                          format_text_gb_s=round(text.numel() / fmt_ms[0] / 1e6, 2),
                          edge_list_text_gb_s=round(edges.numel() / edge_ms[0] / 1e6, 2), round_trip_identical=same)), flush=True)


if __name__ == "__main__":
    main()
