"""The stream-order contract (include/sbx.h, Conventions) for the entry points of include/sbfx.h, on a caller's stream
that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams fixtures)
with this file's own cases and its own synchronous table.

sbfx_csr_degrees_degree_distribution returns with its kernel enqueued, as the two entry points it fuses do;
sbfx_csr_bandwidth_profile reads both results back and waits for the handle's stream.  Every decoy has the shape of the
real input: the same n and nnz with the degrees in another order; the same offsets with other columns — a premature read
shows as a wrong value, never as a fault or another size.

tests/test_extract_abi.py (no GPU) checks that every name of capi.EXTRACT_PROTOTYPES is the target of a case here and has
a row in SYNCHRONOUS.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stream_order_gpu as so  # noqa: E402
from test_stream_order_gpu import Job, ctx, delay, held_back, streams  # noqa: E402,F401  (fixtures by name)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SYNCHRONOUS = {"sbfx_csr_degrees_degree_distribution": False, "sbfx_csr_bandwidth_profile": True}

CASES = []  # (id, entry point, builder of the Job, read-out modes)


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


def _tdt(dt):
    return torch.from_numpy(np.zeros(0, dt)).dtype


def _degrees_distribution(tup, fb):
    def build():
        ra, rb = so._row_ptrs()  # the same n and nnz, the degrees in another order
        ot, idt = so.TUPLES[tup]
        fdt = np.float32 if fb == 4 else np.float64
        nnz = int(ra[-1])
        n = len(ra) - 1

        def run(ctx, bufs, outs):
            ctx.ops.csr_degrees_degree_distribution(bufs[0], nnz, out=(outs[0], outs[1]))
            return list(outs), None

        def want(r):
            deg = np.diff(r)
            return [so._cast(deg, idt), deg.astype(fdt) / fdt(nnz)], None
        return Job([so._cast(ra, ot)], [so._cast(rb, ot)], run, want(ra), want(rb), outs=[(n, idt), (n, fdt)])
    return build


def _bandwidth_profile(tup):
    def build():
        n, rp, ca, cb = so._square()
        ca, cb = so._relabel_cols(rp, ca, n, 0), so._relabel_cols(rp, cb, n, 1)  # (sorted rows, the same offsets)
        ot, idt = so.TUPLES[tup]
        run = lambda ctx, bufs, outs: ([], ctx.ops.csr_bandwidth_profile(bufs[0], bufs[1]))
        rows = so._row_ids(rp)
        first = rp[:-1][np.diff(rp) > 0]

        def want(c):
            head_row, head_col = rows[first], c[first]
            return [], (int(np.abs(rows - c).max()) + 1, int(np.maximum(head_row - head_col, 0).sum()))
        return Job([so._cast(rp, ot), so._cast(ca, idt)], [so._cast(rp, ot), so._cast(cb, idt)], run, want(ca), want(cb))
    return build


case("csr_degrees_degree_distribution-i32-f32", "sbfx_csr_degrees_degree_distribution", other_stream=True)(
    _degrees_distribution("i32", 4))
case("csr_degrees_degree_distribution-i64-f64", "sbfx_csr_degrees_degree_distribution")(_degrees_distribution("i64", 8))
case("csr_bandwidth_profile-i32", "sbfx_csr_bandwidth_profile")(_bandwidth_profile("i32"))
case("csr_bandwidth_profile-i64", "sbfx_csr_bandwidth_profile")(_bandwidth_profile("i64"))

PARAMS = [pytest.param(cid, entry, build, mode, id=f"{cid}/{mode}") for cid, entry, build, modes in CASES for mode in modes]
OBSERVED = {}  # entry point -> {case id: returned while the delay was pending}: this file's own, not the other file's


@pytest.mark.parametrize("cid,entry,build,mode", PARAMS)
def test_case(ctx, delay, streams, cid, entry, build, mode, monkeypatch):
    monkeypatch.setattr(so, "OBSERVED", OBSERVED)  # (held_back records there; the other file's table stays its own)
    why = held_back(ctx, delay[0], streams, cid, entry, build(), mode)
    assert why is None, f"{entry} on a held-back stream: {why}"


def test_synchronous_table():
    """Entry point by entry point: returned while the delay was pending, or waited — against SYNCHRONOUS, the rows of
    INTEGRATION.md's "Streams" table."""
    if not OBSERVED:
        return
    wrong = [(key, "returned early" if early else "waited") for entry, seen in OBSERVED.items() for key, early in seen.items()
             if early != (not SYNCHRONOUS[entry])]
    assert not wrong, f"not as SYNCHRONOUS (and INTEGRATION.md) say: {wrong}"
    if sum(len(s) for s in OBSERVED.values()) == len(PARAMS):
        assert sorted(OBSERVED) == sorted(SYNCHRONOUS)
