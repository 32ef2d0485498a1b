"""The stream-order contract (include/sbx.h, Conventions) for the two entry points of include/sbmt.h, on a caller's
stream that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams
fixtures) with this file's own cases and its own synchronous table, as tests/test_mm_stream_order_gpu.py has them.

sbmt_csr_transpose_plan reads back (its check of the columns; the conversions inside): it waits for the caller's stream
and its three arrays are right when it returns.  sbmt_csr_spmm_t has no read-back: it must be seen to return while the
caller's stream is still held, and Y is read out in stream order (on the caller's stream, and for one case behind an
event on a second stream).  Every decoy has the shape of the real input: the same n, m, nnz, k and row_ptr, the columns
renamed (so another plan of the same sizes), other values and another X — a premature read shows as a wrong value, never
as a fault.  The values are small integers, so every sum is exact.  k = 3 takes the groups-of-lanes form of the kernel,
k = 64 the one-group form.

tests/test_mt_abi.py (no GPU) checks that every name of capi.MT_PROTOTYPES is the target of a case here for every index
tuple and has a row in SYNCHRONOUS.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transpose_restate as tr  # noqa: E402
import test_stream_order_gpu as so  # noqa: E402
from test_stream_order_gpu import Job, ctx, delay, held_back, streams  # noqa: E402,F401  (fixtures by name)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SYNCHRONOUS = {"sbmt_csr_transpose_plan": True, "sbmt_csr_spmm_t": False}

CASES = []  # (id, entry point, builder of the Job, read-out modes)
N, M = 2000, 1500


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


@functools.lru_cache(None)
def _data():
    """2000 x 1500, 16800 entries with duplicates; (rp, col A, col B) and the two plans."""
    from sparsebase_amd import synth
    rp, col = synth.random_rect_csr(N, M, 16000, seed=51, idx_dtype=np.int64, sort_rows=True, dup_frac=0.05)
    colb = so._relabel_cols(rp, col, M, 53)
    return rp, col, colb, tr.plan(rp, col, M), tr.plan(rp, colb, M)


def _plan(tup):
    def build():
        rp, ca, cb, pa, pb = _data()
        ot, idt = so.TUPLES[tup]

        def run(ctx, bufs, outs):
            p = ctx.ops.csr_transpose_plan(bufs[0], bufs[1], M)
            return [p.col_ptr, p.row, p.perm], None
        want = lambda p: ([so._cast(p[0], ot), so._cast(p[1], idt), so._cast(p[2], ot)], None)
        return Job([so._cast(rp, ot), so._cast(ca, idt)], [so._cast(rp, ot), so._cast(cb, idt)], run, want(pa), want(pb))
    return build


def _spmm_t(tup, dt, pattern, k):
    def build():
        rp, ca, cb, pa, pb = _data()
        ot, idt = so.TUPLES[tup]
        g = np.random.default_rng(59 + k)
        xa, xb = (g.integers(-8, 9, N * k).astype(dt) for _ in range(2))
        va, vb = (None if pattern else g.integers(-1000, 1000, len(ca)).astype(dt) for _ in range(2))

        def run(ctx, bufs, outs):
            plan = ctx.ops.TransposePlan(N, M, bufs[0], bufs[1], bufs[2])
            ctx.ops.csr_spmm_t(plan, bufs[4].view(N, k), val=bufs[3], out=outs[0].view(M, k))
            return [outs[0]], None

        def want(p, v, x):  # (exact: sums far below 2^24)
            return [tr.spmm_t_wide(N, p[0], p[1], p[2], x, k, v)[0].astype(dt).reshape(-1)], None

        def arrays(p, v, x):
            return [so._cast(p[0], ot), so._cast(p[1], idt), so._cast(p[2], ot), v, x]
        return Job(arrays(pa, va, xa), arrays(pb, vb, xb), run, want(pa, va, xa), want(pb, vb, xb), outs=[(M * k, dt)])
    return build


case("csr_transpose_plan-i32", "sbmt_csr_transpose_plan", other_stream=True)(_plan("i32"))
case("csr_transpose_plan-i64", "sbmt_csr_transpose_plan")(_plan("i64"))
case("csr_transpose_plan-i32_n64", "sbmt_csr_transpose_plan")(_plan("i32_n64"))
case("csr_spmm_t-i32-f32-k3", "sbmt_csr_spmm_t", other_stream=True)(_spmm_t("i32", np.float32, False, 3))
case("csr_spmm_t-i32-f32-k64", "sbmt_csr_spmm_t")(_spmm_t("i32", np.float32, False, 64))
case("csr_spmm_t-i64-f32-k64", "sbmt_csr_spmm_t")(_spmm_t("i64", np.float32, False, 64))
case("csr_spmm_t-i64-f32-k3-pattern", "sbmt_csr_spmm_t")(_spmm_t("i64", np.float32, True, 3))
case("csr_spmm_t-i32_n64-f32-k3", "sbmt_csr_spmm_t")(_spmm_t("i32_n64", np.float32, False, 3))
case("csr_spmm_t-i32_n64-f32-k64-pattern", "sbmt_csr_spmm_t")(_spmm_t("i32_n64", np.float32, True, 64))

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
