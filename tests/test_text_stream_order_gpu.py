"""The stream-order contract (include/sbx.h, Conventions) for the entry points of include/sbx_text.h, on a caller's
stream that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams
fixtures) with this file's own cases and its own synchronous table.

Every decoy has the shape of the real input AND gives a text of the same length (ids of three digits, values of four
digits and one decimal), so that a premature read shows as a wrong byte and never as a fault or another size.

tests/test_text_abi.py (no GPU) checks that every name of capi.TEXT_PROTOTYPES is the target of a case here and has a
row in SYNCHRONOUS.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stream_order_gpu as so  # noqa: E402
import text_restate as tr  # noqa: E402
from test_stream_order_gpu import Job, ctx, delay, held_back, streams  # noqa: E402,F401  (fixtures by name)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# Every formatter reads its length back, both checks their counters: all wait for the handle's stream.
SYNCHRONOUS = {
    "sbx_text_format_values": True, "sbx_text_format_coordinate": True, "sbx_text_format_dense": True,
    "sbx_coo_symmetry_check": True, "sbx_coo_undirected_unique": True,
}

CASES = []  # (id, entry point, builder of the Job, read-out modes)
ITYPES = {"i32": np.int32, "i64": np.int64}


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


def _vals(count, seed, dt):
    return (np.random.default_rng(seed).integers(1000, 10000, count) + 0.5).astype(dt)  # "1234.5"


def _ids(count, seed, dt):
    return np.random.default_rng(seed).integers(100, 999, count).astype(dt)  # (three digits with index_base 1 too)


def _text(b):
    return np.frombuffer(b, np.uint8).copy()


def _format_values(dt):
    def build():
        a, b = _vals(50000, 1, dt), _vals(50000, 2, dt)
        run = lambda ctx, bufs, outs: ([ctx.ops.text_format_values(bufs[0], precision=9)], None)
        want = lambda v: ([_text(tr.format_values(v, 9))], None)
        return Job([a], [b], run, want(a), want(b))
    return build


def _format_coordinate(tup, dt, flags):
    def build():
        n = 40000
        A = [_ids(n, 3, ITYPES[tup]), _ids(n, 4, ITYPES[tup]), _vals(n, 5, dt)]
        B = [_ids(n, 6, ITYPES[tup]), _ids(n, 7, ITYPES[tup]), _vals(n, 8, dt)]
        if flags:  # SBX_TEXT_LOWER: entry k is kept (col < row) unless k % 3 == 0, in the real input and in the decoy
            for X, seed in ((A, 31), (B, 32)):
                g = np.random.default_rng(seed)
                lo, hi = g.integers(100, 550, n).astype(ITYPES[tup]), g.integers(550, 999, n).astype(ITYPES[tup])
                drop = np.arange(n) % 3 == 0
                X[0], X[1] = np.where(drop, lo, hi), np.where(drop, hi, lo)

        def run(ctx, bufs, outs):
            return [ctx.ops.text_format_coordinate(bufs[0], bufs[1], bufs[2], index_base=1, precision=9, lower=bool(flags & 1))], None
        want = lambda X: ([_text(tr.format_coordinate(X[0], X[1], X[2], 1, 9, flags))], None)
        wa, wb = want(A), want(B)
        assert len(wa[0][0]) == len(wb[0][0])
        return Job(A, B, run, wa, wb)
    return build


def _dense(tup):
    def build():
        n, m, k = 200, 150, 9000
        def entries(seed):
            cells = np.random.default_rng(seed).choice(n * m, k, replace=False)
            return [(cells % n).astype(ITYPES[tup]), (cells // n).astype(ITYPES[tup]), _vals(k, seed + 1, np.float64)]
        A, B = entries(11), entries(13)
        run = lambda ctx, bufs, outs: ([ctx.ops.text_format_dense(n, m, bufs[0], bufs[1], bufs[2], precision=6)], None)
        want = lambda X: ([_text(tr.format_dense(n, m, X[0], X[1], X[2], 6))], None)
        return Job(A, B, run, want(A), want(B))
    return build


def _symmetry(tup, skew):
    def build():
        n, pairs = 900, 20000
        def entries(seed, broken):
            g = np.random.default_rng(seed)
            i, j = g.integers(0, n, pairs), g.integers(0, n, pairs)
            w = (g.integers(1, 50, pairs) / 4.0).astype(np.float32)
            d = g.integers(0, n, 100 + seed)  # (another diagonal count in the decoy)
            row, col = np.concatenate([i, j, d]), np.concatenate([j, i, d])
            val = np.concatenate([w, -w if skew else w, np.zeros(len(d), np.float32)])
            if broken:
                val[:7] += 1.0
            o = g.permutation(len(row))
            return [row[o].astype(ITYPES[tup]), col[o].astype(ITYPES[tup]), val[o]]
        A, B = entries(1, False), entries(2, True)
        B = [x[:len(A[0])] for x in B]  # (the same shape)
        run = lambda ctx, bufs, outs: ([], ctx.ops.coo_symmetry_check(n, bufs[0], bufs[1], bufs[2], skew=skew))
        want = lambda X: ([], tr.symmetry_check(n, X[0], X[1], X[2], skew))
        return Job(A, B, run, want(A), want(B))
    return build


def _undirected(tup, weighted):
    def build():
        nnz = 60000
        def entries(seed):
            g = np.random.default_rng(seed)
            return [g.integers(0, 700, nnz).astype(ITYPES[tup]), g.integers(0, 700, nnz).astype(ITYPES[tup]),
                    np.arange(nnz, dtype=np.float64) + seed if weighted else None]
        A, B = entries(21), entries(22)

        def run(ctx, bufs, outs):
            r, c, v = ctx.ops.coo_undirected_unique_(bufs[0], bufs[1], bufs[2])
            return [r, c, v], int(r.numel())

        def want(X):
            r, c, v = tr.undirected_unique(X[0], X[1], X[2])
            return [r, c, v], len(r)
        return Job(A, B, run, want(A), want(B), inplace=True)
    return build


case("text_format_values-f32", "sbx_text_format_values")(_format_values(np.float32))
case("text_format_values-f64", "sbx_text_format_values")(_format_values(np.float64))
for _i, _tup in enumerate(ITYPES):
    case(f"text_format_coordinate-{_tup}-all", "sbx_text_format_coordinate", other_stream=_i == 0)(
        _format_coordinate(_tup, np.float32, 0))
    case(f"text_format_coordinate-{_tup}-lower", "sbx_text_format_coordinate")(_format_coordinate(_tup, np.float64, tr.LOWER))
    case(f"text_format_dense-{_tup}", "sbx_text_format_dense")(_dense(_tup))
    case(f"coo_symmetry_check-{_tup}-{'skew' if _i else 'plain'}", "sbx_coo_symmetry_check")(_symmetry(_tup, bool(_i)))
    case(f"coo_undirected_unique-{_tup}-{'weighted' if _i else 'plain'}", "sbx_coo_undirected_unique")(_undirected(_tup, bool(_i)))

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
