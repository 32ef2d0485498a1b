"""The stream-order contract (include/sbx.h, Conventions) for the entry points of include/sbmv.h, on a caller's stream
that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams fixtures)
with this file's own cases and its own synchronous table.

sbmv_csr_check reads its verdict back and waits for the handle's stream.  sbmv_csr_spmv has no read-back: it must be
seen to return while the caller's stream is still held, and y is read out in stream order (on the caller's stream, and
for one case behind an event on a second stream).  Every decoy has the shape of the real input: the same n, m, nnz and
row_ptr, the columns renamed, other values and another x — a premature read shows as a wrong value, never as a fault.
The values are small integers, so every sum is exact and y does not depend on the order of the sum.

tests/test_mv_abi.py (no GPU) checks that every name of capi.MV_PROTOTYPES is the target of a case here for every index
tuple and has a row in SYNCHRONOUS.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmv_restate as mv  # noqa: E402
import test_stream_order_gpu as so  # noqa: E402
from test_stream_order_gpu import Job, ctx, delay, held_back, streams  # noqa: E402,F401  (fixtures by name)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SYNCHRONOUS = {"sbmv_csr_check": True, "sbmv_csr_spmv": False}

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


def _check(tup):
    def build():
        rp, ca, cb = _data()
        ot, idt = so.TUPLES[tup]
        ca, cb = ca.copy(), cb.copy()
        ca[1234], cb[77] = M, -1  # both refused, at different positions: the message is the host result

        def run(ctx, bufs, outs):
            try:
                ctx.ops.csr_check(bufs[0], bufs[1], M)
            except ctx.capi.SbxError as e:
                return [], str(e)
            return [], "accepted"
        return Job([so._cast(rp, ot), so._cast(ca, idt)], [so._cast(rp, ot), so._cast(cb, idt)], run,
                   ([], _refusal(1234)), ([], _refusal(77)))
    return build


def _refusal(pos):
    return f"sbx status 1 (bad argument): sbmv_csr_check: the column at position {pos} lies outside [0, {M})"


def _spmv(tup, dt, pattern):
    def build():
        rp, ca, cb = _data()
        ot, idt = so.TUPLES[tup]
        g = np.random.default_rng(57)
        xa, xb = (g.integers(-8, 9, M).astype(dt) for _ in range(2))
        va, vb = (None if pattern else g.integers(-1000, 1000, len(ca)).astype(dt) for _ in range(2))

        def run(ctx, bufs, outs):
            ctx.ops.csr_spmv(bufs[0], bufs[1], bufs[3], val=bufs[2], out=outs[0])
            return [outs[0]], None

        def want(c, v, x):
            if np.issubdtype(dt, np.integer):
                return [mv.spmv_int(rp, c, x, v)], None
            return [mv.spmv_wide(rp, c, x, v)[0].astype(dt)], None  # (exact: integer values, sums far below 2^24)
        return Job([so._cast(rp, ot), so._cast(ca, idt), va, xa], [so._cast(rp, ot), so._cast(cb, idt), vb, xb], run,
                   want(ca, va, xa), want(cb, vb, xb), outs=[(N, dt)])
    return build


case("csr_check-i32", "sbmv_csr_check", other_stream=True)(_check("i32"))
case("csr_check-i64", "sbmv_csr_check")(_check("i64"))
case("csr_check-i32_n64", "sbmv_csr_check")(_check("i32_n64"))
case("csr_spmv-i32-f32", "sbmv_csr_spmv", other_stream=True)(_spmv("i32", np.float32, False))
case("csr_spmv-i64-f64", "sbmv_csr_spmv")(_spmv("i64", np.float64, False))
case("csr_spmv-i32_n64-i64-pattern", "sbmv_csr_spmv")(_spmv("i32_n64", np.int64, True))

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
    """Entry point by entry point: returned while the delay was pending, or waited — against SYNCHRONOUS, the rows of
    INTEGRATION.md's "Streams" table."""
    if not OBSERVED:
        return
    wrong = [(key, "returned early" if early else "waited") for entry, seen in OBSERVED.items() for key, early in seen.items()
             if early != (not SYNCHRONOUS[entry])]
    assert not wrong, f"not as SYNCHRONOUS (and INTEGRATION.md) say: {wrong}"
    if sum(len(s) for s in OBSERVED.values()) == len(PARAMS):
        assert sorted(OBSERVED) == sorted(SYNCHRONOUS)
