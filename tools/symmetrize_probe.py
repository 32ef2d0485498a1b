#!/usr/bin/env python3
"""sbsym_csr_missing_mirrors and sbsym_csr_symmetrize on the bench matrix (symmetric RMAT, scale 22, edge factor 13: the
matrix bench.py builds), timed with device events behind warm-ups.  One JSON line per measurement.

Two matrices: the bench matrix, which is structurally symmetric and takes the fast path (the transposed keys equal the
matrix's own, no search runs), and its strict upper triangle, where every entry needs its mirror.  On each:
sbsym_csr_missing_mirrors, sbsym_csr_symmetrize in pattern mode and with float32 values, every one alternating with
sbx_csr_to_csc on the same arrays (A B A B ...) as the yardstick: the transposition is what the new calls cannot do
without.  The margin is the spread of the yardstick's even against its odd repetitions.  Outputs are allocated before
the timed region.

The fast path is a compile-time constant: run the probe once more with SBX_PROBE_LIB=<variant> for a library built by
  python tools/build_variant.py nofast sbx_symmetrize.hip -DSBSYM_FASTPATH=0

  python tools/symmetrize_probe.py [--scale 22] [--edge-factor 13] [--reps 30] [--warmup 5]
"""
import argparse
import ctypes as C
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


def upper_triangle(rp, col):
    n = rp.numel() - 1
    row = torch.repeat_interleave(torch.arange(n, device=rp.device, dtype=torch.int64), (rp[1:] - rp[:-1]).long())
    keep = col.long() > row
    deg = torch.bincount(row[keep], minlength=n)
    rp2 = torch.zeros(n + 1, dtype=rp.dtype, device=rp.device)
    rp2[1:] = torch.cumsum(deg, 0).to(rp.dtype)
    return rp2, col[keep].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=13)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    lib = os.environ.get("SBX_PROBE_LIB") or "product"
    rp, col = synth.rmat_symmetric_torch(args.scale, args.edge_factor, seed=1)
    for name, (rp, col) in (("symmetric", (rp, col)), ("upper", upper_triangle(rp, col))):
        n, nnz = rp.numel() - 1, col.numel()
        val = torch.rand(nnz, dtype=torch.float32, device=col.device)
        hd = ops.handle_for(col.device)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rpo, co, vo = torch.empty_like(rp), torch.empty(2 * nnz, dtype=col.dtype, device=col.device), \
            torch.empty(2 * nnz, dtype=torch.float32, device=col.device)
        cp, ro, cvo = torch.empty_like(rp), torch.empty_like(col), torch.empty_like(val)

        def symmetrize(v, v_out):
            k, added = C.c_int64(0), C.c_int64(0)
            hd.check(hd.lib.sbsym_csr_symmetrize(hd.h, capi.SBX_I32, capi.V_F32 if v is not None else capi.V_NONE, n, nnz,
                                                 p(rp), p(col), p(v), 0, 2 * nnz, p(rpo), p(co), p(v_out), C.byref(k),
                                                 C.byref(added)))
            return k.value, added.value

        def to_csc(v, v_out):
            hd.check(hd.lib.sbx_csr_to_csc(hd.h, capi.SBX_I32, capi.V_F32 if v is not None else capi.V_NONE, n, n, nnz, p(rp),
                                           p(col), p(v), p(cp), p(ro), p(v_out)))

        calls = (("missing_mirrors", lambda: ops.csr_missing_mirrors(rp, col), lambda: to_csc(None, None)),
                 ("symmetrize_pattern", lambda: symmetrize(None, None), lambda: to_csc(None, None)),
                 ("symmetrize_f32", lambda: symmetrize(val, vo), lambda: to_csc(val, cvo)))
        for what, call, yard in calls:
            for _ in range(args.warmup):
                ref = call()
                yard()
            torch.cuda.synchronize()
            t_new, t_yard = [], []
            for _ in range(args.reps):
                ms, got = timed(call)
                assert got == ref
                t_new.append(ms)
                t_yard.append(timed(yard)[0])
            sn, sy = stats(t_new), stats(t_yard)
            spread = abs(stats(t_yard[0::2])["median_ms"] - stats(t_yard[1::2])["median_ms"])
            print(json.dumps({"probe": "symmetrize", "lib": lib, "matrix": name, "call": what, "n": n, "nnz": nnz,
                              "result": ref, "new": sn, "csr_to_csc": sy, "csr_to_csc_even_odd_spread_ms": round(spread, 4),
                              "ratio_to_csr_to_csc": round(sn["median_ms"] / sy["median_ms"], 3),
                              "within_yardstick_plus_margin": sn["median_ms"] <= sy["median_ms"] + spread,
                              "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
