#!/usr/bin/env python3
"""sbmv_csr_spmv (ops.csr_spmv, float32 values) on the bench matrix (symmetric RMAT, scale 22, edge factor 13: the matrix
bench.py builds) under five orderings: the generator's own, a seeded random permutation, and RCM, Degree and Gray, each
applied with Permute2D (ops.permute_csr, rows and columns).  One JSON line per ordering, appended to --out.

Every call is timed with device events behind warm-ups: the median of --reps single calls, and the mean of one batch of
--reps calls between two events (what a loop of an experiment pays: the calls are asynchronous).  Two yardsticks are
taken in the same run on the same arrays:
  - the vendor path through torch, torch.sparse_csr_tensor(row_ptr, col, val) @ x, where this torch build runs it (if it
    does not, the line says so and the probe carries on);
  - this project's own gather floor: DESIGN §4.4 measured 190 - 220 G gathered entries per second chip-wide in the
    permute, about 0.50 ms for the bench matrix's 105 M entries; the line carries nnz / 220e9 and nnz / 190e9.
Each line also carries the algorithmic bytes nnz (I + V) + n (Z + V) + m V and the rate they give, and the mean number of
distinct 128-byte lines of x that 64 consecutive entries touch (the lines a wave's gather instruction asks for), counted
on a sample of the entries: what the address-path account of §4.4 says an ordering changes.

  python tools/spmv_probe.py [--scale 22] [--edge-factor 13] [--reps 20] [--warmup 5] [--out profiles/spmv_probe.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebase_amd import ops, synth  # noqa: E402


def timed(fn, calls=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls, out


def measure(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    single = sorted(timed(fn)[0] for _ in range(reps))
    batch, _ = timed(fn, reps)
    return {"median_ms": round(single[len(single) // 2], 4), "min_ms": round(single[0], 4), "max_ms": round(single[-1], 4),
            "batch_mean_ms": round(batch, 4)}


def lines_per_gather(col, sample_waves=1 << 16, seed=3):
    """Mean number of distinct 128-byte lines of a float32 x among 64 consecutive entries, over a sample of aligned groups."""
    groups = col.numel() // 64
    g = torch.Generator(device="cpu").manual_seed(seed)
    pick = torch.randint(0, groups, (min(sample_waves, groups),), generator=g).to(col.device)
    idx = (pick[:, None] * 64 + torch.arange(64, device=col.device)[None, :]).reshape(-1)
    lines = (col[idx].long() >> 5).reshape(-1, 64).sort(dim=1).values
    return round(float((1 + (lines[:, 1:] != lines[:, :-1]).sum(dim=1)).float().mean()), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=13)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmv_probe.jsonl"))
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least ten warm calls"
    rp, col = synth.rmat_symmetric_torch(args.scale, args.edge_factor, seed=1)
    n, nnz = rp.numel() - 1, col.numel()
    dev = col.device
    gen = torch.Generator(device="cpu").manual_seed(5)
    val = (torch.rand(nnz, generator=gen) * 2 - 1).to(dev)
    x = (torch.rand(n, generator=gen) * 2 - 1).to(dev)
    y0 = ops.csr_spmv(rp, col, x, val=val)
    scale_of = torch.zeros(n, device=dev).index_add_(  # S_i = sum |val||x|, the scale a difference is read against
        0, torch.repeat_interleave(torch.arange(n, device=dev), (rp[1:] - rp[:-1]).long()), val.abs() * x[col.long()].abs())

    def order_of(name):
        if name == "generator":
            return None
        if name == "random":
            return torch.randperm(n, generator=torch.Generator(device="cpu").manual_seed(7)).to(dev).to(col.dtype)
        if name == "rcm":
            return ops.rcm_reorder(rp, col)
        if name == "degree":
            return ops.degree_reorder(rp, True, id_dtype=col.dtype)
        return ops.gray_reorder(n, rp, col, 32, 10, 4)

    out = open(args.out, "a")
    for name in ("generator", "random", "rcm", "degree", "gray"):
        line = {"probe": "spmv", "ordering": name, "n": n, "nnz": nnz, "value_type": "f32", "index_type": "i32", "reps": args.reps}
        try:
            order = order_of(name)
            if order is None:
                brp, bcol, bval, bx = rp, col, val, x
            else:
                brp, bcol, bval = ops.permute_csr(n, n, rp, col, val, order, order)
                bx = torch.empty_like(x)
                bx[order.long()] = x
            y = torch.empty(n, dtype=x.dtype, device=dev)
            line["spmv"] = measure(lambda: ops.csr_spmv(brp, bcol, bx, val=bval, out=y), args.warmup, args.reps)
            back = y if order is None else y[order.long()]
            line["max_difference_from_generator_over_S"] = float(((back - y0).abs() / scale_of.clamp_min(1e-30)).max())
            line["lines_of_x_per_64_entries"] = lines_per_gather(bcol)
            alg_bytes = nnz * (4 + 4) + n * (4 + 4) + n * 4
            line["algorithmic_bytes"] = alg_bytes
            line["algorithmic_TBps"] = round(alg_bytes / (line["spmv"]["median_ms"] * 1e-3) / 1e12, 3)
            line["gathered_G_entries_per_s"] = round(nnz / (line["spmv"]["median_ms"] * 1e-3) / 1e9, 1)
            line["gather_floor_ms"] = [round(nnz / 220e9 * 1e3, 4), round(nnz / 190e9 * 1e3, 4)]
            try:
                A = torch.sparse_csr_tensor(brp, bcol, bval, size=(n, n))
                yt = A @ bx
                line["torch_sparse_csr"] = measure(lambda: A @ bx, args.warmup, args.reps)
                line["max_difference_from_torch_over_S"] = float(
                    ((yt - y).abs() / (scale_of if order is None else scale_of.new_zeros(n).index_copy_(0, order.long(), scale_of))
                     .clamp_min(1e-30)).max())
                line["ratio_to_torch"] = round(line["spmv"]["median_ms"] / line["torch_sparse_csr"]["median_ms"], 3)
                del A, yt
            except Exception as e:  # written down, and the probe carries on
                line["torch_sparse_csr"] = f"did not run: {type(e).__name__}: {str(e)[:200]}"
        except Exception as e:
            line["error"] = f"{type(e).__name__}: {str(e)[:300]}"
        print(json.dumps(line), flush=True)
        out.write(json.dumps(line) + "\n")
        out.flush()
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
