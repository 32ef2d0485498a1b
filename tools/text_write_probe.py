#!/usr/bin/env python3
"""The text-output path (include/sbx_text.h) on the bench matrix — symmetric RMAT, scale 22, edge factor 13, seed 1
(bench.py's default), as a COO with f32 values — timed with device events behind warm-ups:

  format_coordinate     sizing call + writing call of sbx_text_format_coordinate (what ops.text_format_coordinate does)
  format_coordinate_1   the writing call alone, into a buffer that is there (what a streaming caller pays per chunk)
  format_values         sbx_text_format_values over the values
  symmetry_check        sbx_coo_symmetry_check (the entries are (row, col)-sorted: no scratch sort)
  undirected_unique     sbx_coo_undirected_unique on a copy (the copies are outside the timed region)
  d2h                   the text, device -> page-locked host memory
  write_pipeline        what io/writer.h does for WriteHIPCOO, from Python: chunks of 2^24 entries, each formatted,
                        copied into pinned memory and written with one write() to a file on a RAM-backed path
  host_stream_loop      the plain `ostream <<` loop over the same entries on the host (what the reference executes),
                        compiled here with g++ -O2 and writing to the same RAM-backed path

Achieved bytes/s = (bytes read + bytes written, from the shapes) / time, against the 8.0 TB/s HBM peak of the MI355X.
One JSON line.  The kernel breakdown comes from a separate run under rocprofv3 --kernel-trace --stats.

  python tools/text_write_probe.py [--scale 22] [--edge-factor 13] [--reps 5] [--warmup 2] [--precision 6]
                                   [--dir /dev/shm] [--host-entries N]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsebase_amd import capi, ops, synth  # noqa: E402

HBM_PEAK = 8.0e12
CHUNK = 1 << 24

HOST_LOOP = r"""
#include <chrono>
#include <cstdio>
#include <fstream>
#include <vector>
int main(int argc, char **argv) {
  const long nnz = atol(argv[2]);
  std::vector<int> row(nnz), col(nnz);
  std::vector<float> val(nnz);
  FILE *f = fopen(argv[1], "rb");
  if (!f || fread(row.data(), 4, nnz, f) != (size_t)nnz || fread(col.data(), 4, nnz, f) != (size_t)nnz ||
      fread(val.data(), 4, nnz, f) != (size_t)nnz) return 2;
  fclose(f);
  const auto t0 = std::chrono::steady_clock::now();
  std::ofstream out(argv[3]);
  for (long i = 0; i < nnz; i++) out << row[i] + 1 << " " << col[i] + 1 << " " << val[i] << "\n";
  out.close();
  printf("%.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return 0;
}
"""


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return round(sorted(times)[len(times) // 2], 3), [round(t, 3) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=13)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", type=int, default=6)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--host-entries", type=int, default=None, help="entries of the host loop (default: all)")
    a = ap.parse_args()
    rp, col = synth.rmat_symmetric_torch(a.scale, a.edge_factor, seed=1)
    n, nnz = rp.numel() - 1, col.numel()
    row, col, _ = ops.csr_to_coo(n, n, rp, col)
    lo, hi = torch.minimum(row, col), torch.maximum(row, col)
    val = ((lo * 31 + hi * 17) % 100003).to(torch.float32) / 64.0 + 0.001  # (symmetric: the same weight both ways)
    del lo, hi, rp
    res = dict(input=f"rmat{a.scale}_ef{a.edge_factor}", n=n, nnz=nnz, precision=a.precision, hbm_peak_bytes_per_s=HBM_PEAK)
    hd = ops.handle_for(row.device)
    p = lambda t: C.c_void_p(t.data_ptr())

    def rate(name, ms, nbytes):
        res[name + "_bytes"] = int(nbytes)
        res[name + "_GBps"] = round(nbytes / ms / 1e6, 1)
        res[name + "_of_hbm_peak"] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)

    text = ops.text_format_coordinate(row, col, val, precision=a.precision)
    nbytes = text.numel()
    res["text_bytes"] = nbytes
    res["format_coordinate_ms"], res["format_coordinate_times_ms"] = timed(
        lambda: ops.text_format_coordinate(row, col, val, precision=a.precision), a.reps, a.warmup)
    # per call: 12 B of input per entry read twice (lengths, write), the 16-byte records written once and read twice
    per_call = nnz * (4 + 16) + 2 * nnz * (8 + 16)
    rate("format_coordinate", res["format_coordinate_ms"], 2 * per_call - 0 + nbytes)
    wrote = C.c_int64(0)

    def write_only():
        hd.check(hd.lib.sbx_text_format_coordinate(hd.h, capi.SBX_I32, capi.V_F32, nnz, p(row), p(col), p(val), 1, a.precision, 0,
                                                   p(text), nbytes, C.byref(wrote)))
    res["format_coordinate_1_ms"], res["format_coordinate_1_times_ms"] = timed(write_only, a.reps, a.warmup)
    rate("format_coordinate_1", res["format_coordinate_1_ms"], per_call + nbytes)
    vtext = ops.text_format_values(val, precision=a.precision)
    res["format_values_ms"], _ = timed(lambda: ops.text_format_values(val, precision=a.precision), a.reps, a.warmup)
    rate("format_values", res["format_values_ms"], 2 * (nnz * (4 + 16) + 2 * nnz * 16) + vtext.numel())
    del vtext
    sym = ops.coo_symmetry_check(n, row, col, val)
    res["symmetry_result"] = list(sym)
    res["symmetry_check_ms"], _ = timed(lambda: ops.coo_symmetry_check(n, row, col, val), a.reps, a.warmup)
    r2, c2, v2 = row.clone(), col.clone(), val.clone()

    def unique():
        r2.copy_(row), c2.copy_(col), v2.copy_(val)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ops.coo_undirected_unique_(r2, c2, v2)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out[0].numel()
    runs = [unique() for _ in range(a.warmup + a.reps)][a.warmup:]
    res["undirected_unique_ms"] = round(sorted(t for t, _ in runs)[len(runs) // 2], 3)
    res["undirected_unique_left"] = runs[0][1]
    del r2, c2, v2
    # the profiler's groups for one formatting call
    ops.profile_enable(True)
    ops.profile_report()
    ops.text_format_coordinate(row, col, val, precision=a.precision)
    torch.cuda.synchronize()
    res["format_coordinate_kernel_ms_by_group"] = {g: round(t, 3) for g, (t, c, b) in ops.profile_report().items() if c}
    ops.profile_enable(False)
    # device -> host
    pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    res["d2h_ms"], _ = timed(lambda: pinned.copy_(text, non_blocking=True), a.reps, a.warmup)
    res["d2h_GBps"] = round(nbytes / res["d2h_ms"] / 1e6, 1)
    del text, pinned
    # the writer's pipeline: chunk by chunk through pinned memory into a file on a RAM-backed path
    path = os.path.join(a.dir, "sbx_text_probe.mtx")

    def pipeline():
        d_text, h_text = None, None
        with open(path, "wb", buffering=0) as f:
            f.write(b"%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, nnz))
            for b in range(0, nnz, CHUNK):
                e = min(nnz, b + CHUNK)
                got = C.c_int64(0)
                cap = 0 if d_text is None else d_text.numel()
                rc = hd.lib.sbx_text_format_coordinate(hd.h, capi.SBX_I32, capi.V_F32, e - b, p(row[b:e]), p(col[b:e]), p(val[b:e]),
                                                       1, a.precision, 0, None if d_text is None else p(d_text), cap, C.byref(got))
                if d_text is None or got.value > cap:
                    d_text = torch.empty(got.value + got.value // 8, dtype=torch.uint8, device=row.device)
                    h_text = torch.empty(d_text.numel(), dtype=torch.uint8, pin_memory=True)
                    rc = hd.lib.sbx_text_format_coordinate(hd.h, capi.SBX_I32, capi.V_F32, e - b, p(row[b:e]), p(col[b:e]),
                                                           p(val[b:e]), 1, a.precision, 0, p(d_text), d_text.numel(), C.byref(got))
                hd.check(rc)
                h_text[:got.value].copy_(d_text[:got.value])
                f.write(memoryview(h_text.numpy())[:got.value])
    walls = []
    for _ in range(1 + max(1, a.reps // 2)):
        t0 = time.perf_counter()
        pipeline()
        walls.append((time.perf_counter() - t0) * 1e3)
    res["write_pipeline_wall_ms"] = round(sorted(walls[1:])[len(walls[1:]) // 2], 1)
    res["file_bytes"] = os.path.getsize(path)
    os.remove(path)
    # the host's stream loop over the same entries
    cnt = nnz if a.host_entries is None else min(nnz, a.host_entries)
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp, tempfile.TemporaryDirectory() as build:  # (a RAM-backed path may be noexec)
        src, exe, data = os.path.join(build, "loop.cc"), os.path.join(build, "loop"), os.path.join(tmp, "entries.bin")
        with open(src, "w") as f:
            f.write(HOST_LOOP)
        subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", exe])
        with open(data, "wb") as f:
            for t in (row, col, val):
                f.write(t[:cnt].cpu().numpy().tobytes())
        out = subprocess.run([exe, data, str(cnt), os.path.join(tmp, "host.mtx")], capture_output=True, text=True, check=True)
        res["host_stream_loop_entries"] = cnt
        res["host_stream_loop_ms"] = float(out.stdout.strip())
        res["host_stream_loop_bytes"] = os.path.getsize(os.path.join(tmp, "host.mtx"))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
