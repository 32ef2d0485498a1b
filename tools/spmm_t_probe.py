#!/usr/bin/env python3
"""sbmt_csr_transpose_plan and sbmt_csr_spmm_t (ops.csr_transpose_plan, ops.csr_spmm_t, float32 values, 32-bit ids) on
the bench matrix (symmetric RMAT, scale 22, edge factor 13: the matrix bench.py builds), as loaded and under RCM (applied
with ops.permute_csr, rows and columns), for k = 1, 8, 32, 64, 128 columns.  One JSON line per ordering for the plan and
one per (ordering, k) for the product, appended to --out.

Every figure is taken with device events behind warm-ups, as the median (with the minimum and the maximum) of single
calls; the two sides of a comparison are taken ALTERNATELY — a, b, a, b, ... — with the same number of warm-ups and of
timed calls each (--warmup, --reps), so that whatever drifts during a point drifts for both.  In the same run and on the
same arrays:
  (1) the plan, ops.csr_transpose_plan, against ops.csr_to_csc with float32 values: what is sorted once against what
      the workaround sorts on every step;
  (2) ops.csr_spmm_t(plan, X, val) against ops.csr_spmm on the materialised transpose (col_ptr, row, val[perm]): what the
      indirection through perm costs inside the same kernel (the two results are compared bit for bit as well);
  (3) the per-step alternative the plan replaces, ops.csr_to_csc with values followed by ops.csr_spmm on its output, against
      (2)'s ops.csr_spmm_t: one event pair around both calls;
  (4) the forward product ops.csr_spmm on A at the same k, for scale.
The spread of a figure is its (max - min) / median; a ratio is said to exceed 1 only beyond the spread of its two sides.

  python tools/spmm_t_probe.py [--scale 22] [--edge-factor 13] [--reps 20] [--warmup 5] [--out profiles/spmm_t_probe.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparsebase_amd import ops, synth  # noqa: E402
from spmm_probe import measure, measure_alternating  # noqa: E402

KS = (1, 8, 32, 64, 128)


def spread(stat):
    return round((stat["max_ms"] - stat["min_ms"]) / stat["median_ms"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=13)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ks", type=int, nargs="*", default=list(KS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_t_probe.jsonl"))
    args = ap.parse_args()
    assert args.reps >= 10, "the median of at least ten warm calls"
    rp, col = synth.rmat_symmetric_torch(args.scale, args.edge_factor, seed=1)
    n, nnz = rp.numel() - 1, col.numel()
    dev = col.device
    val = (torch.rand(nnz, generator=torch.Generator(device="cpu").manual_seed(5)) * 2 - 1).to(dev)

    out = open(args.out, "a")

    def emit(line):
        print(json.dumps(line), flush=True)
        out.write(json.dumps(line) + "\n")
        out.flush()
        if "error" in line:  # the device may be in any state: the probe ends here
            out.close()
            sys.exit(1)

    for name in ("generator", "rcm"):
        if name == "generator":
            brp, bcol, bval = rp, col, val
        else:
            order = ops.rcm_reorder(rp, col)
            brp, bcol, bval = ops.permute_csr(n, n, rp, col, val, order, order)
            del order
        line = {"probe": "spmm_t_plan", "ordering": name, "n": n, "nnz": nnz, "value_type": "f32", "index_type": "i32"}
        try:
            line["plan"], line["csr_to_csc_f32"] = measure_alternating(
                lambda: ops.csr_transpose_plan(brp, bcol, n), lambda: ops.csr_to_csc(n, n, brp, bcol, bval), args.warmup, args.reps)
            line["ratio_1_plan_to_csr_to_csc"] = round(line["plan"]["median_ms"] / line["csr_to_csc_f32"]["median_ms"], 3)
            plan = ops.csr_transpose_plan(brp, bcol, n)
            tval = bval[plan.perm.long()]  # the values of the materialised transpose
        except Exception as e:
            line["error"] = f"{type(e).__name__}: {str(e)[:300]}"
        emit(line)
        for k in args.ks:
            line = {"probe": "spmm_t", "ordering": name, "k": k, "n": n, "nnz": nnz, "value_type": "f32", "index_type": "i32"}
            try:
                X = torch.rand((n, k), generator=torch.Generator(device="cpu").manual_seed(11 + k)).to(dev) * 2 - 1
                Y, Y2 = torch.empty((n, k), dtype=X.dtype, device=dev), torch.empty((n, k), dtype=X.dtype, device=dev)
                if k == 1:  # (the materialised side would take the SpMV's kernels at unit strides: a slice keeps it on the span kernel)
                    Xw, Yw = torch.zeros((n, 2), dtype=X.dtype, device=dev), torch.empty((n, 2), dtype=X.dtype, device=dev)
                    Xw[:, :1] = X
                    xm, ym = Xw[:, :1], Yw[:, :1]
                else:
                    xm, ym = X, Y2
                spmm_t = lambda: ops.csr_spmm_t(plan, X, bval, out=Y)
                line["spmm_t"], line["spmm_on_materialised_transpose"] = measure_alternating(
                    spmm_t, lambda: ops.csr_spmm(plan.col_ptr, plan.row, xm, val=tval, m=n, out=ym), args.warmup, args.reps)
                line["ratio_2_spmm_t_to_materialised"] = round(
                    line["spmm_t"]["median_ms"] / line["spmm_on_materialised_transpose"]["median_ms"], 3)
                line["spread_2"] = [spread(line["spmm_t"]), spread(line["spmm_on_materialised_transpose"])]
                line["bits_equal_2"] = bool(torch.equal(Y.view(torch.int32), ym.contiguous().view(torch.int32)))

                def per_step():
                    cp, ro, vo = ops.csr_to_csc(n, n, brp, bcol, bval)
                    ops.csr_spmm(cp, ro, X, val=vo, m=n, out=Y2)
                line["spmm_t_again"], line["csr_to_csc_then_spmm"] = measure_alternating(spmm_t, per_step, args.warmup, args.reps)
                line["ratio_3_spmm_t_to_per_step_alternative"] = round(
                    line["spmm_t_again"]["median_ms"] / line["csr_to_csc_then_spmm"]["median_ms"], 3)
                line["spread_3"] = [spread(line["spmm_t_again"]), spread(line["csr_to_csc_then_spmm"])]
                line["forward_spmm"] = measure(lambda: ops.csr_spmm(brp, bcol, X, val=bval, out=Y2), args.warmup, args.reps)
                line["ratio_4_spmm_t_to_forward"] = round(line["spmm_t"]["median_ms"] / line["forward_spmm"]["median_ms"], 3)
                # bytes the entries ask for: ids, positions, gathered values and a row of X each; the materialised side has no perm
                line["bytes_asked_spmm_t"] = nnz * (4 + 4 + 4 + k * 4) + n * 4 + n * k * 4
                line["bytes_asked_materialised"] = nnz * (4 + 4 + k * 4) + n * 4 + n * k * 4
                del X, Y, Y2
            except Exception as e:
                line["error"] = f"{type(e).__name__}: {str(e)[:300]}"
            emit(line)
            torch.cuda.empty_cache()
        del plan, tval
    out.close()


if __name__ == "__main__":
    main()
