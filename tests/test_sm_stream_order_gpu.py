"""The stream-order contract (include/sbx.h, Conventions) for the two entry points of include/sbsm.h, on a caller's
stream that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams
fixtures) with this file's own cases and its own synchronous table, as tests/test_dd_stream_order_gpu.py has them.

Neither call has a read-back: each must be seen to return while the caller's stream is still held, and its output is
read in stream order (on the caller's stream, and for one case per entry point behind an event on a second stream).
Every decoy has the shape of the real input: the same n, nnz and row_ptr, other values — a premature read shows as a
wrong value, never as a fault.  The values make the result exact: the forward takes rows of one constant and -inf (every
exp is 1 or 0, out is 1 / count or +0 in any order), the backward small integers.

tests/test_sm_abi.py (no GPU) checks that every name of capi.SM_PROTOTYPES is the target of a case here for every index
tuple and has a row in SYNCHRONOUS.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stream_order_gpu as so  # noqa: E402
from test_stream_order_gpu import Job, ctx, delay, held_back, streams  # noqa: E402,F401  (fixtures by name)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SYNCHRONOUS = {"sbsm_csr_row_softmax": False, "sbsm_csr_row_softmax_backward": False}

CASES = []  # (id, entry point, builder of the Job, read-out modes)
N = 2000


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


@functools.lru_cache(None)
def _data():
    """2000 rows, 16800 entries, rows of 0 to about 20 entries and one of 5000 (it crosses spans); (rp, rows)."""
    g = np.random.default_rng(51)
    lengths = g.integers(0, 13, N)
    lengths[700] = 5000
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rp, so._row_ids(rp)


def _forward(tup, dt, pattern=False):
    def build():
        rp, rows = _data()
        ot, _ = so.TUPLES[tup]
        g = np.random.default_rng(61)

        def values():  # one constant per row, -inf at a third of the positions
            v = g.integers(-30, 31, N).astype(dt)[rows]
            v[g.random(len(rows)) < 1.0 / 3] = -np.inf
            return v

        def want(v):
            count = np.bincount(rows[np.isfinite(v)], minlength=N).astype(dt)
            with np.errstate(divide="ignore"):
                return [np.where(np.isfinite(v), dt(1) / count[rows], dt(0)).astype(dt)], None

        def run(ctx, bufs, outs):
            ctx.ops.csr_row_softmax(bufs[0], bufs[1], out=outs[0])
            return [outs[0]], None
        va, vb = values(), values()
        return Job([so._cast(rp, ot), va], [so._cast(rp, ot), vb], run, want(va), want(vb), outs=[(len(rows), dt)])
    return build


def _backward(tup, dt):
    def build():
        rp, rows = _data()
        ot, _ = so.TUPLES[tup]
        g = np.random.default_rng(62)

        def want(s, gr):  # (exact: integers in [-8, 8], rows of at most 5000 entries)
            d = np.zeros(N, np.int64)
            np.add.at(d, rows, s.astype(np.int64) * gr.astype(np.int64))
            return [s * (gr.astype(np.int64) - d[rows]).astype(dt)], None

        def run(ctx, bufs, outs):
            ctx.ops.csr_row_softmax_backward(bufs[0], bufs[1], bufs[2], out=outs[0])
            return [outs[0]], None
        sa, sb, ga, gb = (g.integers(-8, 9, len(rows)).astype(dt) for _ in range(4))
        return Job([so._cast(rp, ot), sa, ga], [so._cast(rp, ot), sb, gb], run, want(sa, ga), want(sb, gb),
                   outs=[(len(rows), dt)])
    return build


case("csr_row_softmax-i32-f32", "sbsm_csr_row_softmax", other_stream=True)(_forward("i32", np.float32))
case("csr_row_softmax-i64-f32", "sbsm_csr_row_softmax")(_forward("i64", np.float32))
case("csr_row_softmax-i32_n64-f32", "sbsm_csr_row_softmax")(_forward("i32_n64", np.float32))
case("csr_row_softmax_backward-i32-f32", "sbsm_csr_row_softmax_backward", other_stream=True)(_backward("i32", np.float32))
case("csr_row_softmax_backward-i64-f32", "sbsm_csr_row_softmax_backward")(_backward("i64", np.float32))
case("csr_row_softmax_backward-i32_n64-f32", "sbsm_csr_row_softmax_backward")(_backward("i32_n64", np.float32))

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
