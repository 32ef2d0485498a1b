#!/usr/bin/env python3
"""sbsm_csr_row_softmax and sbsm_csr_row_softmax_backward (ops.csr_row_softmax, ops.csr_row_softmax_backward, float32
values, 32-bit offsets) on two matrices: the bench matrix (symmetric RMAT, scale 22, edge factor 13: the matrix bench.py
builds) and `hub`, one row of 2^24 entries followed by 2^20 rows of 8 (every entry of the hub takes the carry and the
fix-up).  The values are normal with sigma = 4; the backward takes s from the forward and g uniform in (-1, 1).  One JSON
line per (matrix, direction), appended to --out.

Every figure is taken with device events behind warm-ups, as the median (with the minimum and the maximum) of single
calls.  The three legs are taken ALTERNATELY — a, b, c, a, b, c, ... — with the same number of warm-ups and of timed
calls each (--warmup, --reps), so that whatever drifts during a point drifts for all of them.  In the same run and on the
same arrays:
  (a) the kernel;
  (b) the torch composition that was the only way before: forward scatter_reduce_(amax), gather, exp, index_add_, gather
      and divide; backward index_add_ of s g, gather, subtract and multiply; `rows` is built outside the timed region;
  (c) the streaming yardstick for the same bytes: out.copy_(val) for the forward, torch.mul(s, g, out=dz) for the backward.
The acceptance condition is (a) < (b) on the bench matrix; each line carries `a_below_b`.  a / c is reported without a
threshold.  (a) and (b) are also compared: max |out_a - out_b| (the orders of the sums differ).  float64 is not here: the
library does not build it yet (include/sbsm.h).

  python tools/softmax_probe.py [--scale 22] [--edge-factor 13] [--reps 20] [--warmup 5] [--matrices bench hub]
                               [--out profiles/softmax_probe.jsonl]
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
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(times):
    times = sorted(times)
    return {"median_ms": round(times[len(times) // 2], 4), "min_ms": round(times[0], 4), "max_ms": round(times[-1], 4),
            "reps": len(times)}


def measure_alternating(legs, warmup, reps):
    """The legs of a comparison, alternated call by call: the same warm-ups, the same number of timed calls."""
    for _ in range(warmup):
        for fn in legs:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in legs]
    for _ in range(reps):
        for t, fn in zip(times, legs):
            t.append(timed(fn))
    return [_stats(t) for t in times]


def hub_matrix(dev):
    lengths = torch.full((1 + 2 ** 20,), 8, dtype=torch.int64)
    lengths[0] = 2 ** 24
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths, 0)]).to(torch.int32).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=13)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--matrices", nargs="*", default=["bench", "hub"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_probe.jsonl"))
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least ten warm calls"
    dev = torch.device("cuda", torch.cuda.current_device())
    out = open(args.out, "a")
    for name in args.matrices:
        if name == "bench":
            rp, col = synth.rmat_symmetric_torch(args.scale, args.edge_factor, seed=1)
            del col
        else:
            rp = hub_matrix(dev)
        n, nnz = rp.numel() - 1, int(rp[-1])
        rows = torch.repeat_interleave(torch.arange(n, device=dev), (rp[1:] - rp[:-1]).long())  # (outside every timed region)
        for dtype, vt in ((torch.float32, "f32"),):
            val = (torch.randn(nnz, generator=torch.Generator(device="cpu").manual_seed(5), dtype=torch.float32) * 4).to(dev).to(dtype)
            g = (torch.rand(nnz, generator=torch.Generator(device="cpu").manual_seed(6)) * 2 - 1).to(dev).to(dtype)
            oa, ob, oc = (torch.empty(nnz, dtype=dtype, device=dev) for _ in range(3))
            s = ops.csr_row_softmax(rp, val)

            def torch_forward():
                m = torch.full((n,), float("-inf"), dtype=dtype, device=dev)
                m.scatter_reduce_(0, rows, val, "amax")
                e = torch.exp(val - m[rows])
                total = torch.zeros(n, dtype=dtype, device=dev).index_add_(0, rows, e)
                torch.div(e, total[rows], out=ob)

            def torch_backward():
                sg = s * g
                d = torch.zeros(n, dtype=dtype, device=dev).index_add_(0, rows, sg)
                torch.mul(s, g - d[rows], out=ob)
            for direction, legs, bytes_ in (
                    ("forward", (lambda: ops.csr_row_softmax(rp, val, out=oa), torch_forward, lambda: oc.copy_(val)),
                     nnz * 2 * val.element_size() + n * 4),
                    ("backward", (lambda: ops.csr_row_softmax_backward(rp, s, g, out=oa), torch_backward,
                                  lambda: torch.mul(s, g, out=oc)), nnz * 3 * val.element_size() + n * 4)):
                line = {"probe": "softmax", "matrix": name, "direction": direction, "n": n, "nnz": nnz, "value_type": vt,
                        "index_type": "i32"}
                try:
                    a, b, c = measure_alternating(legs, args.warmup, args.reps)
                    line["a_kernel"], line["b_torch_composition"], line["c_streaming_yardstick"] = a, b, c
                    line["legs_alternated"] = True
                    line["a_below_b"] = a["median_ms"] < b["median_ms"]
                    line["ratio_a_to_b"] = round(a["median_ms"] / b["median_ms"], 4)
                    line["ratio_a_to_c"] = round(a["median_ms"] / c["median_ms"], 3)
                    line["algorithmic_bytes"] = bytes_
                    line["a_TBps"] = round(bytes_ / (a["median_ms"] * 1e-3) / 1e12, 3)
                    line["max_difference_a_b"] = float((oa - ob).abs().max())
                except Exception as e:
                    line["error"] = f"{type(e).__name__}: {str(e)[:300]}"
                print(json.dumps(line), flush=True)
                out.write(json.dumps(line) + "\n")
                out.flush()
                if "error" in line:  # the device may be in any state: the probe ends here
                    out.close()
                    sys.exit(1)
            del val, g, oa, ob, oc, s
            torch.cuda.empty_cache()
        del rows, rp
    out.close()


if __name__ == "__main__":
    main()
