#!/usr/bin/env python3
"""sbdd_csr_sddmm (ops.csr_sddmm, float32 values, 32-bit ids) on the bench matrix (symmetric RMAT, scale 22, edge factor
13: the matrix bench.py builds) for k = 1, 4, 16, 32, 64, 128, 256 columns under three orderings: the generator's own, RCM
and a seeded random permutation, each applied with Permute2D (ops.permute_csr, rows and columns).  U and V are uniform in
(-1, 1).  One JSON line per (ordering, k), appended to --out.

Every figure is taken with device events behind warm-ups, as the median (with the minimum and the maximum) of single
calls.  (a) and (b), the two sides of the acceptance condition, are taken ALTERNATELY — a, b, a, b, ... — with the same
number of warm-ups and of timed calls each (--warmup, --reps), so that whatever drifts during a point drifts for both.
For each point, in the same run and on the same arrays:
  (a) ops.csr_sddmm;
  (b) the only way to compute it without sbdd.h: val * (U[rows] * V[col]).sum(1) in torch, `rows` computed outside the
      timed region, the entries in chunks of --chunk-elements / k (so that a temporary of chunk x k values is 2 GiB of
      float32 by default; the line carries the chunk size), one event pair per chunk, the chunks' times summed;
  (c) ops.csr_spmm at the same k on V: it gathers the same rows of V;
  (d') computed, not measured: the bytes the entries ask for, nnz (I + 2 V + k V) + (row runs) k V + n Z — every entry
      gathers its row of V, every run of entries of one row loads its row of U once — at the rate at which the
      microarchitecture guide's "Indexed rows" section measured whole rows gathered by index from a table of the size of V
      (8.6 TB/s from a table that fits the Infinity Cache's 38 MB point, 7.4 TB/s up to 256 MiB, 5.5 TB/s beyond).
The acceptance condition is (a) < (b) for every k >= 4; each line carries `a_below_b`.  (a) and (b) are also compared:
max |out_a - out_b| over max |out_a| (the orders of the sums differ).

  python tools/sddmm_probe.py [--scale 22] [--edge-factor 13] [--reps 20] [--warmup 5] [--out profiles/sddmm_probe.jsonl]
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


def _stats(times):
    times = sorted(times)
    return {"median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4),
            "reps": len(times)}


def measure(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return _stats([timed(fn) for _ in range(reps)])


def measure_alternating(fa, fb, warmup, reps):
    """The two sides of a comparison, alternated call by call: the same warm-ups, the same number of timed calls.  Each
    of fa, fb returns its own time in milliseconds."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(fa())
        tb.append(fb())
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
    ap.add_argument("--chunk-elements", type=int, default=2 ** 29)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sddmm_probe.jsonl"))
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
        lengths = (brp[1:] - brp[:-1]).long()
        rows = torch.repeat_interleave(torch.arange(n, device=dev), lengths)  # (outside every timed region)
        cols = bcol.long()
        row_runs = int((lengths > 0).sum())
        del lengths
        for k in args.ks:
            line = {"probe": "sddmm", "ordering": name, "k": k, "n": n, "nnz": nnz, "value_type": "f32", "index_type": "i32"}
            try:
                U = torch.rand((n, k), generator=torch.Generator(device="cpu").manual_seed(11 + k)).to(dev) * 2 - 1
                V = torch.rand((n, k), generator=torch.Generator(device="cpu").manual_seed(211 + k)).to(dev) * 2 - 1
                oa, ob = (torch.empty(nnz, dtype=U.dtype, device=dev) for _ in range(2))
                chunk = max(1, min(nnz, args.chunk_elements // k))

                def torch_way():
                    total = 0.0
                    for p0 in range(0, nnz, chunk):
                        p1 = min(nnz, p0 + chunk)

                        def piece():
                            ob[p0:p1] = bval[p0:p1] * (U[rows[p0:p1]] * V[cols[p0:p1]]).sum(1)
                        total += timed(piece)
                    return total
                line["a_sddmm"], line["b_torch_gather_multiply_sum"] = measure_alternating(
                    lambda: timed(lambda: ops.csr_sddmm(brp, bcol, U, V, val=bval, out=oa)), torch_way, args.warmup, args.reps)
                line["b_chunk_entries"], line["b_chunks"] = chunk, (nnz + chunk - 1) // chunk
                line["a_b_alternated"] = True
                a_ms = line["a_sddmm"]["median_ms"]
                line["a_below_b"] = a_ms < line["b_torch_gather_multiply_sum"]["median_ms"]
                line["ratio_a_to_b"] = round(a_ms / line["b_torch_gather_multiply_sum"]["median_ms"], 4)
                line["max_difference_a_b_over_max_out"] = float((oa - ob).abs().max() / oa.abs().max())
                del ob
                Y = torch.empty((n, k), dtype=U.dtype, device=dev)
                line["c_spmm_same_k"] = measure(lambda: ops.csr_spmm(brp, bcol, V, val=bval, out=Y), args.warmup, args.reps)
                line["ratio_a_to_c"] = round(a_ms / line["c_spmm_same_k"]["median_ms"], 3)
                del Y
                alg = nnz * (4 + 2 * 4) + n * 4 + (n + n) * k * 4
                asked = nnz * (4 + 2 * 4 + k * 4) + row_runs * k * 4 + n * 4
                rate = gather_rate(n * k * 4)
                line["algorithmic_bytes"], line["gather_rate_TBps"], line["row_runs"] = alg, rate, row_runs
                line["bytes_the_entries_ask_for"] = asked
                line["d_asked_bytes_at_gather_rate_ms"] = round(asked / (rate * 1e12) * 1e3, 4)
                line["ratio_a_to_d_asked"] = round(a_ms / line["d_asked_bytes_at_gather_rate_ms"], 3)
                del U, V, oa
            except Exception as e:
                line["error"] = f"{type(e).__name__}: {str(e)[:300]}"
            print(json.dumps(line), flush=True)
            out.write(json.dumps(line) + "\n")
            out.flush()
            if "error" in line:  # the device may be in any state: the probe ends here
                out.close()
                sys.exit(1)
            torch.cuda.empty_cache()
        del rows, cols
    out.close()


if __name__ == "__main__":
    main()
