"""The stream-order contract (include/sbx.h, Conventions) for the entry points of include/sbx_stats.h, on a caller's
stream that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams
fixtures) with this file's own cases and its own synchronous table.

Both entry points read their result back, so both wait for the handle's stream.  The decoys have the shape of the real
input: a row_ptr of the same length with other degrees for the degree statistics, the same row_ptr with renamed
columns for OffDiagBlockNNZ.

tests/test_stats_abi.py (no GPU) checks that every name of capi.STATS_PROTOTYPES is the target of a case here and has a
row in SYNCHRONOUS.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stream_order_gpu as so  # noqa: E402
from test_degree_stats_host import degree_stats, off_diag  # noqa: E402
from test_stream_order_gpu import Job, ctx, delay, held_back, streams  # noqa: E402,F401  (fixtures by name)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SYNCHRONOUS = {"sbxstat_degree_stats": True, "sbxstat_csr_off_diag_block_nnz": True}

CASES = []  # (id, entry point, builder of the Job, read-out modes)


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


def _degree_stats(tup):
    def build():
        ra, _ = so._row_ptrs()
        # the decoy: other degrees, not the same ones in another order (every statistic of a permutation is the same)
        rb = np.concatenate([[0], np.cumsum(np.diff(ra)[::-1] + np.arange(len(ra) - 1) % 3)])
        ot = so.TUPLES[tup][0]
        run = lambda ctx, bufs, outs: ([], ctx.ops.degree_stats(bufs[0], median=True, log=False))
        want = lambda r: ([], dict(degree_stats(r), sum_log=0.0))  # (the integers: exact, whatever the order of the sums)
        return Job([so._cast(ra, ot)], [so._cast(rb, ot)], run, want(ra), want(rb))
    return build


def _off_diag(tup, h, w):
    def build():
        n, rp, ca, cb = so._square()
        ca, cb = so._relabel_cols(rp, ca, n, 0), so._relabel_cols(rp, cb, n, 1)
        ot, idt = so.TUPLES[tup]
        run = lambda ctx, bufs, outs: ([], ctx.ops.csr_off_diag_block_nnz(bufs[0], bufs[1], n, h, w))
        want = lambda c: ([], off_diag(rp, c, n, n, h, w))
        return Job([so._cast(rp, ot), so._cast(ca, idt)], [so._cast(rp, ot), so._cast(cb, idt)], run, want(ca), want(cb))
    return build


for _i, _tup in enumerate(so.TUPLES):
    case(f"degree_stats-{_tup}", "sbxstat_degree_stats")(_degree_stats(_tup))
    case(f"csr_off_diag_block_nnz-{_tup}", "sbxstat_csr_off_diag_block_nnz")(_off_diag(_tup, (16, 64, 7)[_i], (16, 5, 64)[_i]))

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
