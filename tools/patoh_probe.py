#!/usr/bin/env python3
"""PaToH hypergraph files on the device: sbhg_patoh_parse (the lines behind the header resident in HBM -> the nets x cells
CSR in file order, the cells x nets CSR, the weights) with and without the transpose, sbhg_cells_to_nets alone, and
sbhg_patoh_format + sbhg_patoh_format_weights, on a generated hypergraph of about `pins` pins: nets of about 10 pins and
one net of pins / 20 pins, net and cell weights (scheme 3), float32 values.  In the same run, as the yardstick,
sbgr_metis_parse on a METIS file of as many tokens: the same passes with one role rule less.

One JSON line: the text sizes and token counts, the ms of each (medians of warm calls, each ending in a device
synchronise, with minimum and maximum) and text GB/s.  The text is written by the formatters themselves, and the parse is
checked to give the arrays back.

  tools/patoh_probe.py [pins]      (run it under `timeout`: it has no limit of its own)

The clock is the host's (perf_counter up to a device synchronise), as in tools/metis_probe.py: every entry point is
synchronous, it reads counts and lengths back between its kernels, so the host's wait is part of what a caller pays.
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
    pins = int(args[0]) if args else 10_000_000
    assert torch.cuda.is_available(), "the probe measures the GPU path: there is nothing to fall back to"
    g = torch.Generator(device="cuda").manual_seed(5)
    big = pins // 20
    nets = max(2, (pins - big) // 10)
    cells = max(2, nets // 2)
    deg = torch.randint(5, 16, (nets,), device="cuda", generator=g)
    deg[nets // 2] = big
    xpin = torch.zeros(nets + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(deg, 0, out=xpin[1:])
    total = int(xpin[-1])
    xpin = xpin.to(torch.int32)
    pin = torch.randint(0, cells, (total,), device="cuda", generator=g, dtype=torch.int32)
    nw = torch.randint(1, 1000, (nets,), device="cuda", generator=g).to(torch.float32)
    cw = torch.randint(1, 1000, (cells,), device="cuda", generator=g).to(torch.float32)

    def fmt():
        return torch.cat([ops.patoh_format(xpin, pin, nw, net_weights=True), ops.patoh_format_weights(cw)])
    text = fmt()
    fmt_ms = timed(fmt)
    parse = lambda tr: ops.patoh_parse(text, cells, nets, total, 0, 3, torch.int32, torch.float32, transpose=tr)
    parse_ms = timed(lambda: parse(True))
    plain_ms = timed(lambda: parse(False))
    tr_ms = timed(lambda: ops.cells_to_nets(xpin, pin, cells, 0))
    xp2, p2, xn2, n2, nw2, cw2 = parse(True)
    xn3, n3 = ops.cells_to_nets(xpin, pin, cells, 0)
    same = bool(torch.equal(xp2, xpin) and torch.equal(p2, pin) and torch.equal(nw2, nw) and torch.equal(cw2, cw) and
                torch.equal(xn2, xn3) and torch.equal(n2, n3))
    tokens = total + nets + cells
    # the yardstick: a METIS file of as many tokens (a symmetric graph of tokens / 2 edges, unweighted: every token an id)
    n = max(2, tokens // 16)
    a = torch.randint(0, n, (tokens // 2,), device="cuda", generator=g)
    b = torch.randint(0, n, (tokens // 2,), device="cuda", generator=g)
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    key = torch.unique(lo * n + hi)
    key = key[key // n != key % n]
    lo, hi = (key // n).to(torch.int32), (key % n).to(torch.int32)
    row, col = torch.cat([lo, hi]), torch.cat([hi, lo])
    ops.coo_sort_(n, n, row, col)
    rp, col, _ = ops.coo_to_csr(n, n, row, col, None, rows_sorted=True)
    mtext = ops.metis_format(rp, col)
    metis_ms = timed(lambda: ops.metis_parse(mtext, n, lo.numel(), 0, 0, True, torch.int32, None))
    print(json.dumps(dict(cells=cells, nets=nets, pins=total, longest_net=big, tokens=tokens,
                          text_mb=round(text.numel() / 1e6, 1), parse_ms=parse_ms, parse_without_transpose_ms=plain_ms,
                          cells_to_nets_ms=tr_ms, format_ms=fmt_ms, metis_tokens=int(col.numel()),
                          metis_text_mb=round(mtext.numel() / 1e6, 1), metis_parse_ms=metis_ms,
                          parse_text_gb_s=round(text.numel() / parse_ms[0] / 1e6, 2),
                          plain_parse_text_gb_s=round(text.numel() / plain_ms[0] / 1e6, 2),
                          format_text_gb_s=round(text.numel() / fmt_ms[0] / 1e6, 2),
                          metis_text_gb_s=round(mtext.numel() / metis_ms[0] / 1e6, 2),
                          plain_parse_over_metis_per_token=round((plain_ms[0] / tokens) / (metis_ms[0] / int(col.numel())), 2),
                          round_trip_identical=same)), flush=True)


if __name__ == "__main__":
    main()
