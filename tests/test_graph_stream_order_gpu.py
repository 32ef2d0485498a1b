"""The stream-order contract (include/sbx.h, Conventions) for the entry points of include/sbgr.h, on a caller's stream
that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams fixtures)
with this file's own cases and its own synchronous table.

Both entry points read something back (the line, token and entry counts and the status word; the offsets of the row
range and the text's length), so both wait for the handle's stream.  Every decoy has the shape of the real input: a
graph text of the same length with the same number of lines, tokens and entries (fixed-width tokens), a CSR with the
same row offsets and other columns and values of the same printed width — a premature read shows as a wrong value,
never as a fault or another size.

tests/test_graph_abi.py (no GPU) checks that every name of capi.GRAPH_PROTOTYPES is the target of a case here and has a
row in SYNCHRONOUS.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metis_restate as mr  # noqa: E402
import test_stream_order_gpu as so  # noqa: E402
from test_stream_order_gpu import Job, ctx, delay, held_back, streams  # noqa: E402,F401  (fixtures by name)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SYNCHRONOUS = {"sbgr_metis_parse": True, "sbgr_metis_format": True}

CASES = []  # (id, entry point, builder of the Job, read-out modes)
ITYPES = {"i32": np.int32, "i64": np.int64}


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


def _tdt(dt):
    return None if dt is None else torch.from_numpy(np.zeros(0, dt)).dtype


def _parse(tup, dt):
    def build():
        n, deg = 2500, 6  # every vertex has `deg` neighbours (a circulant graph with random offsets): one text length

        def text(seed):
            g = np.random.default_rng(seed)
            offs = g.choice(np.arange(1, n // 2), deg // 2, replace=False)
            w = g.integers(1, 1 << 16, (n, deg // 2))  # weight of edge {v, v + off}: eighths, exact in float32
            lines = []
            for v in range(n):
                toks = []
                for j, o in enumerate(offs):
                    toks.append("%6d %10.3f" % ((v + o) % n + 1, w[v, j] / 8.0))
                    toks.append("%6d %10.3f" % ((v - o) % n + 1, w[(v - o) % n, j] / 8.0))
                lines.append(" ".join(g.permutation(toks)) if dt is not None else " ".join(t[:6] for t in g.permutation(toks)))
            return ("\n".join(lines) + "\n").encode()
        m, fmt = n * deg // 2, (1 if dt is not None else 0)
        ta, tb = text(1), text(2)
        assert len(ta) == len(tb)
        vtype = {None: "void", np.float32: "float", np.float64: "double"}[dt]

        def want(t):
            r = mr.parse_body(t, n, m, fmt, 1 if fmt else 0, vtype, True)
            outs = [r["row"].astype(ITYPES[tup]), r["col"].astype(ITYPES[tup]), r["val"], r["row_ptr"].astype(ITYPES[tup])]
            return outs, n

        def run(ctx, bufs, outs):
            n_dim, row, col, val, _, rp = ctx.ops.metis_parse(bufs[0], n, m, fmt, 1 if fmt else 0, True, _tdt(ITYPES[tup]),
                                                              _tdt(dt))
            return [x for x in (row, col, val, rp) if x is not None], int(n_dim)
        return Job([so._text_t(ta)], [so._text_t(tb)], run, want(ta), want(tb))
    return build


def _format(tup, dt):
    def build():
        n, deg = 6000, 3
        rp = (np.arange(n + 1) * deg).astype(ITYPES[tup])

        def graph(seed):  # columns and values of one printed width: 4 and 3 characters
            g = np.random.default_rng(seed)
            col = np.sort(g.integers(999, 5999, (n, deg)), axis=1).astype(ITYPES[tup]).ravel()
            val = None if dt is None else g.integers(100, 1000, n * deg).astype(dt)
            vw = None if dt is None else g.integers(10, 100, (n, 2)).astype(dt)
            return [rp, col, val, vw]

        def want(G):
            t = mr.format_lines(G[0], G[1], G[2], G[3], 0, n, 1, 6, dt is not None, dt is not None)
            return [np.frombuffer(t, np.uint8)], None

        def run(ctx, bufs, outs):
            return [ctx.ops.metis_format(bufs[0], bufs[1], bufs[2], bufs[3], edge_weights=dt is not None,
                                         vertex_weights=dt is not None)], None
        A, B = graph(3), graph(4)
        return Job(A, B, run, want(A), want(B))
    return build


case("metis_parse-i32-f32", "sbgr_metis_parse", other_stream=True)(_parse("i32", np.float32))
case("metis_parse-i64-void", "sbgr_metis_parse")(_parse("i64", None))
case("metis_format-i32-f64", "sbgr_metis_format", other_stream=True)(_format("i32", np.float64))
case("metis_format-i64-void", "sbgr_metis_format")(_format("i64", None))

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
