#!/usr/bin/env python3
"""sbmm_csr_spmm (ops.csr_spmm, float32 values, 32-bit ids) on the bench matrix (symmetric RMAT, scale 22, edge factor
13: the matrix bench.py builds) for k = 1, 4, 16, 32, 64, 128, 256 columns under three orderings: the generator's own, RCM
and a seeded random permutation, each applied with Permute2D (ops.permute_csr, rows and columns).  One JSON line per
(ordering, k), appended to --out.

Every figure is taken with device events behind warm-ups, as the median (with the minimum and the maximum) of single
products.  (a) and (b), the two sides of the acceptance condition, are taken ALTERNATELY — a, b, a, b, ... — with the same
number of warm-ups and of timed products each (--warmup, --reps), so that whatever drifts during a point drifts for both.
For each point, in the same run and on the same arrays:
  (a) ops.csr_spmm on the row-major X;
  (b) k calls of ops.csr_spmv on a column-major copy of X, one event pair around the k calls: the only way the library
      computed the product before it had sbmm.h;
  (c) the vendor path through torch, torch.sparse_csr_tensor(row_ptr, col, val) @ X, where this torch build runs it (if it
      does not, the line says so and the probe carries on; a product that takes more than two seconds is timed once);
  (d) computed, not measured: the time the algorithmic bytes nnz (I + V) + n Z + (m + n) k V take at the rate at which
      the microarchitecture guide's "Indexed rows" section measured whole rows gathered by index from a table of the size
      of X (8.6 TB/s from a table that fits the Infinity Cache's 38 MB point, 7.4 TB/s up to 256 MiB, 5.5 TB/s beyond,
      the register-gather figure for a buffer far larger than the Infinity Cache), and beside it the same for the bytes
      the entries actually ask for, nnz (I + V + k V) + n Z + n k V: every entry gathers its own row of X.
The acceptance condition is (a) < (b) for every k >= 4; each line carries `a_below_b`.  (a) and (b) are also compared:
max |Y_a - Y_b| over max |Y_a| (the orders of the sums differ).

  python tools/spmm_probe.py [--scale 22] [--edge-factor 13] [--reps 20] [--warmup 5] [--out profiles/spmm_probe.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebase_amd import ops, synth  # noqa: E402

KS = (1, 4, 16, 32, 64, 128, 256)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(fn, warmup, reps):
    first = timed(fn)
    if first > 2000.0:  # a product of seconds: the one call is the figure
        return {"median_ms": round(first, 4), "min_ms": round(first, 4), "max_ms": round(first, 4), "reps": 1}
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    single = sorted(timed(fn) for _ in range(reps))
    return {"median_ms": round(single[len(single) // 2], 4), "min_ms": round(single[0], 4), "max_ms": round(single[-1], 4),
            "reps": reps}


def _stats(times):
    times = sorted(times)
    return {"median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4),
            "reps": len(times)}


def measure_alternating(fa, fb, warmup, reps):
    """The two sides of a comparison, alternated call by call: the same warm-ups, the same number of timed products."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa))
        tb.append(timed(fb))
    return _stats(ta), _stats(tb)


def gather_rate(table_bytes):
    """TB/s of whole rows gathered by index, by where a table of this size is served from (MI355X, "Indexed rows")."""
    if table_bytes <= 38e6:
        return 8.6
    if table_bytes <= 256 * 2 ** 20:
        return 7.4
    return 5.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=13)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", type=int, nargs="*", default=list(KS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_probe.jsonl"))
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least ten warm calls"
    rp, col = synth.rmat_symmetric_torch(args.scale, args.edge_factor, seed=1)
    n, nnz = rp.numel() - 1, col.numel()
    dev = col.device
    gen = torch.Generator(device="cpu").manual_seed(5)
    val = (torch.rand(nnz, generator=gen) * 2 - 1).to(dev)

    def order_of(name):
        if name == "generator":
            return None
        if name == "random":
            return torch.randperm(n, generator=torch.Generator(device="cpu").manual_seed(7)).to(dev).to(col.dtype)
        return ops.rcm_reorder(rp, col)

    out = open(args.out, "a")
    for name in ("generator", "rcm", "random"):
        order = order_of(name)
        if order is None:
            brp, bcol, bval = rp, col, val
        else:
            brp, bcol, bval = ops.permute_csr(n, n, rp, col, val, order, order)
        del order
        for k in args.ks:
            line = {"probe": "spmm", "ordering": name, "k": k, "n": n, "nnz": nnz, "value_type": "f32", "index_type": "i32"}
            try:
                X = torch.rand((n, k), generator=torch.Generator(device="cpu").manual_seed(11 + k)).to(dev) * 2 - 1
                Y = torch.empty((n, k), dtype=X.dtype, device=dev)
                Xc, Yc = X.t().contiguous(), torch.empty((k, n), dtype=X.dtype, device=dev)

                def k_calls():
                    for j in range(k):
                        ops.csr_spmv(brp, bcol, Xc[j], val=bval, out=Yc[j])
                line["a_spmm"], line["b_k_spmv_calls"] = measure_alternating(
                    lambda: ops.csr_spmm(brp, bcol, X, val=bval, out=Y), k_calls, args.warmup, args.reps)
                line["a_b_alternated"] = True
                line["a_below_b"] = line["a_spmm"]["median_ms"] < line["b_k_spmv_calls"]["median_ms"]
                line["ratio_a_to_b"] = round(line["a_spmm"]["median_ms"] / line["b_k_spmv_calls"]["median_ms"], 3)
                line["max_difference_a_b_over_max_y"] = float((Y - Yc.t()).abs().max() / Y.abs().max())
                del Xc, Yc
                alg = nnz * (4 + 4) + n * 4 + (n + n) * k * 4
                asked = nnz * (4 + 4 + k * 4) + n * 4 + n * k * 4
                rate = gather_rate(n * k * 4)
                line["algorithmic_bytes"], line["gather_rate_TBps"] = alg, rate
                line["d_algorithmic_bytes_at_gather_rate_ms"] = round(alg / (rate * 1e12) * 1e3, 4)
                line["bytes_the_entries_ask_for"] = asked
                line["d_asked_bytes_at_gather_rate_ms"] = round(asked / (rate * 1e12) * 1e3, 4)
                line["ratio_a_to_d"] = round(line["a_spmm"]["median_ms"] / line["d_algorithmic_bytes_at_gather_rate_ms"], 3)
                line["ratio_a_to_d_asked"] = round(line["a_spmm"]["median_ms"] / line["d_asked_bytes_at_gather_rate_ms"], 3)
                try:
                    A = torch.sparse_csr_tensor(brp, bcol, bval, size=(n, n))
                    line["c_torch_sparse_csr"] = measure(lambda: A @ X, 1, 10)
                    line["ratio_a_to_c"] = round(line["a_spmm"]["median_ms"] / line["c_torch_sparse_csr"]["median_ms"], 4)
                    del A
                except Exception as e:  # an operation torch does not have is written down, and the probe carries on
                    oom = isinstance(e, torch.cuda.OutOfMemoryError)
                    if not oom and ("hip" in str(e).lower() or "memory access" in str(e).lower()):
                        raise  # (a device error is not: nothing more is started on this device)
                    line["c_torch_sparse_csr"] = f"did not run: {type(e).__name__}: {str(e)[:200]}"
                del X, Y
            except Exception as e:
                line["error"] = f"{type(e).__name__}: {str(e)[:300]}"
            print(json.dumps(line), flush=True)
            out.write(json.dumps(line) + "\n")
            out.flush()
            if "error" in line:  # the device may be in any state: the probe ends here
                out.close()
                sys.exit(1)
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
