#!/usr/bin/env python3
"""Array-format Matrix Market ingest on the device: sbio_mtx_parse_values (text resident in HBM -> n * m values) and
sbio_dense_to_coo (column-major values -> COO in (row, col) order), on an n x n float32 array file at about 1 % and at
100 % nonzeros, written by the library's own formatter at precision 9.

Per density one JSON line: parse ms and text GB/s; dense_to_coo ms (count + scan + place, one call with outputs of
exactly nnz entries) and its fraction of the 8 TB/s HBM peak over the algorithmic bytes
n * m * vb read + nnz * (2 * ib + vb) written.  Times are medians of warm calls, each ending in a device synchronise.
With --ref the real reference's MTXReader::ReadCOO reads the same file on the host (oracle/_ref), and the results are
compared (the reference reports the dimensions swapped).

  tools/mtx_array_probe.py [n] [--ref]        (run it under `timeout`: it has no limit of its own)
"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sparsebase_amd import ops  # noqa: E402

HBM_GBS = 8000.0
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
    return statistics.median(ms), min(ms), max(ms)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 4096
    with_ref = "--ref" in sys.argv
    assert torch.cuda.is_available(), "the probe measures the GPU path: there is nothing to fall back to"
    for density in (0.01, 1.0):
        g = torch.Generator(device="cuda").manual_seed(7)
        vals = torch.randn(n * n, device="cuda", generator=g) * 10.0 ** torch.randint(-6, 6, (n * n,), device="cuda", generator=g)
        vals[vals == 0] = 1.0
        if density < 1.0:
            vals[torch.rand(n * n, device="cuda", generator=g) >= density] = 0.0
        text = ops.text_format_values(vals, precision=9)
        nbytes = text.numel()
        parse = timed(lambda: ops.mtx_parse_values(text, n * n, torch.float32))
        dense = ops.mtx_parse_values(text, n * n, torch.float32)
        assert torch.equal(dense.view(torch.int32), vals.view(torch.int32)), "the parse is not the identity"
        row, col, val = ops.dense_to_coo(n, n, dense)
        nnz = row.numel()
        hd = ops.handle_for(dense.device)
        import ctypes as C
        from sparsebase_amd import capi
        k = C.c_int64(0)
        p = lambda t: C.c_void_p(t.data_ptr())

        def fill():
            hd.bind_stream()
            hd.check(hd.lib.sbio_dense_to_coo(hd.h, capi.SBX_I32, capi.V_F32, n, n, p(dense), nnz, p(row), p(col), p(val), C.byref(k)))

        def count():
            hd.bind_stream()
            hd.check(hd.lib.sbio_dense_to_coo(hd.h, capi.SBX_I32, capi.V_F32, n, n, p(dense), 0, None, None, None, C.byref(k)))
        d2c, cnt = timed(fill), timed(count)
        alg = n * n * 4 + nnz * (2 * 4 + 4)
        res = dict(n=n, density=density, nnz=nnz, text_mb=round(nbytes / 1e6, 1),
                   parse_ms=round(parse[0], 3), parse_ms_min_max=[round(parse[1], 3), round(parse[2], 3)],
                   parse_text_gb_s=round(nbytes / parse[0] / 1e6, 1),
                   dense_to_coo_ms=round(d2c[0], 3), dense_to_coo_ms_min_max=[round(d2c[1], 3), round(d2c[2], 3)],
                   dense_to_coo_alg_gb_s=round(alg / d2c[0] / 1e6, 1), dense_to_coo_frac_hbm=round(alg / d2c[0] / 1e6 / HBM_GBS, 4),
                   count_mode_ms=round(cnt[0], 3), read_ms_parse_count_fill=round(parse[0] + cnt[0] + d2c[0], 3))
        if with_ref:
            import orc
            if not orc.ref_available():
                raise SystemExit("--ref: oracle/_ref/libsbref.so is not built")
            path = os.path.join(tempfile.mkdtemp(), "array.mtx")
            with open(path, "wb") as f:
                f.write(f"%%MatrixMarket matrix array real general\n{n} {n}\n".encode())
                f.write(text.cpu().numpy().tobytes())
            t = time.perf_counter()
            rn, rm, rrow, rcol, rval = orc.Ref().mtx_read(path, True, False, np.int32, np.float32, cap=nnz + 8)
            ref_s = time.perf_counter() - t
            os.remove(path)
            res.update(reference_s=round(ref_s, 2), speedup=round(ref_s * 1e3 / res["read_ms_parse_count_fill"], 1),
                       identical=bool(np.array_equal(row.cpu().numpy(), rrow) and np.array_equal(col.cpu().numpy(), rcol)
                                      and val.cpu().numpy().tobytes() == rval.tobytes()))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
