"""The stream-order contract (include/sbx.h, Conventions) for the entry point of include/sbdd.h, on a caller's stream
that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams fixtures)
with this file's own cases and its own synchronous table, as tests/test_mm_stream_order_gpu.py has them.

sbdd_csr_sddmm has no read-back: it must be seen to return while the caller's stream is still held, and `out` is read
in stream order (on the caller's stream, and for one case behind an event on a second stream).  Every decoy has the shape
of the real input: the same n, m, nnz, k and row_ptr, the columns renamed, other values, another U and another V — a
premature read shows as a wrong value, never as a fault.  The values are small integers, so every dot is exact and
`out` does not depend on the order of the sum.  k = 3 takes the groups-of-lanes form of the kernel (four lanes per
entry), k = 64 the wide form at one column per lane and a group of 16 lanes at 16 bytes per lane.

tests/test_dd_abi.py (no GPU) checks that every name of capi.DD_PROTOTYPES is the target of a case here for every index
tuple and has a row in SYNCHRONOUS.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sddmm_restate as dd  # noqa: E402
import test_stream_order_gpu as so  # noqa: E402
from test_stream_order_gpu import Job, ctx, delay, held_back, streams  # noqa: E402,F401  (fixtures by name)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SYNCHRONOUS = {"sbdd_csr_sddmm": False}

CASES = []  # (id, entry point, builder of the Job, read-out modes)
N, M = 2000, 1500


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


@functools.lru_cache(None)
def _data():
    """2000 x 1500, 16800 entries with duplicates; (rp, col A, col B)."""
    from sparsebase_amd import synth
    rp, col = synth.random_rect_csr(N, M, 16000, seed=51, idx_dtype=np.int64, sort_rows=True, dup_frac=0.05)
    return rp, col, so._relabel_cols(rp, col, M, 53)


def _sddmm(tup, dt, pattern, k):
    def build():
        rp, ca, cb = _data()
        ot, idt = so.TUPLES[tup]
        g = np.random.default_rng(61 + k)
        ua, ub = (g.integers(-8, 9, N * k).astype(dt) for _ in range(2))
        xa, xb = (g.integers(-8, 9, M * k).astype(dt) for _ in range(2))
        va, vb = (None if pattern else g.integers(-1000, 1000, len(ca)).astype(dt) for _ in range(2))

        def run(ctx, bufs, outs):
            ctx.ops.csr_sddmm(bufs[0], bufs[1], bufs[3].view(N, k), bufs[4].view(M, k), val=bufs[2], out=outs[0])
            return [outs[0]], None

        def want(c, v, u, x):  # (exact: |val| * k * 64 < 2^24)
            return [dd.sddmm_wide(rp, c, u.reshape(N, k), x.reshape(M, k), k, v, m=M)[0].astype(dt)], None
        return Job([so._cast(rp, ot), so._cast(ca, idt), va, ua, xa], [so._cast(rp, ot), so._cast(cb, idt), vb, ub, xb], run,
                   want(ca, va, ua, xa), want(cb, vb, ub, xb), outs=[(len(ca), dt)])
    return build


case("csr_sddmm-i32-f32-k3", "sbdd_csr_sddmm", other_stream=True)(_sddmm("i32", np.float32, False, 3))
case("csr_sddmm-i32-f32-k64", "sbdd_csr_sddmm")(_sddmm("i32", np.float32, False, 64))
case("csr_sddmm-i64-f32-k64", "sbdd_csr_sddmm")(_sddmm("i64", np.float32, False, 64))
case("csr_sddmm-i64-f32-k3-pattern", "sbdd_csr_sddmm")(_sddmm("i64", np.float32, True, 3))
case("csr_sddmm-i32_n64-f32-k3", "sbdd_csr_sddmm")(_sddmm("i32_n64", np.float32, False, 3))
case("csr_sddmm-i32_n64-f32-k64-pattern", "sbdd_csr_sddmm")(_sddmm("i32_n64", np.float32, True, 64))

PARAMS = [pytest.param(cid, entry, build, mode, id=f"{cid}/{mode}") for cid, entry, build, modes in CASES for mode in modes]
OBSERVED = {}  # entry point -> {case id: returned while the delay was pending}: this file's own, not the other file's


@pytest.mark.parametrize("cid,entry,build,mode", PARAMS)
def test_case(ctx, delay, streams, cid, entry, build, mode, monkeypatch):
    monkeypatch.setattr(so, "OBSERVED", OBSERVED)  # (held_back records there; the other file's table stays its own)
    why = held_back(ctx, delay[0], streams, cid, entry, build(), mode)
    assert why is None, f"{entry} on a held-back stream: {why}"
    if not SYNCHRONOUS[entry]:  # seen NOT to have run while the caller's stream was held
        assert OBSERVED[entry][f"{cid}/{mode}"], f"{entry} waited for the held-back stream: it must return with its work enqueued"


def test_synchronous_table():
    """Returned while the delay was pending, or waited — against SYNCHRONOUS, the row of INTEGRATION.md's "Streams" table."""
    if not OBSERVED:
        return
    wrong = [(key, "returned early" if early else "waited") for entry, seen in OBSERVED.items() for key, early in seen.items()
             if early != (not SYNCHRONOUS[entry])]
    assert not wrong, f"not as SYNCHRONOUS (and INTEGRATION.md) say: {wrong}"
    if sum(len(s) for s in OBSERVED.values()) == len(PARAMS):
        assert sorted(OBSERVED) == sorted(SYNCHRONOUS)
