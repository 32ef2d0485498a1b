"""The stream-order contract (include/sbx.h, Conventions) for the entry points of include/sbhg.h, on a caller's stream
that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams fixtures)
with this file's own cases and its own synchronous table.

All four entry points read something back (the line, token and pin counts and the status word; the number of pins and
the range check; the offsets of the net range and the text's length), so all four wait for the handle's stream.  Every
decoy has the shape of the real input: a text of the same length with the same lines, tokens and pins (fixed-width
tokens), a CSR with the same offsets and other pins, weights of the same printed width — a premature read shows as a
wrong value, never as a fault or another size.

tests/test_hypergraph_abi.py (no GPU) checks that every name of capi.HYPERGRAPH_PROTOTYPES is the target of a case here
and has a row in SYNCHRONOUS.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patoh_restate as pr  # noqa: E402
import test_stream_order_gpu as so  # noqa: E402
from test_stream_order_gpu import Job, ctx, delay, held_back, streams  # noqa: E402,F401  (fixtures by name)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SYNCHRONOUS = {"sbhg_patoh_parse": True, "sbhg_cells_to_nets": True, "sbhg_patoh_format": True,
               "sbhg_patoh_format_weights": True}

CASES = []  # (id, entry point, builder of the Job, read-out modes)
ITYPES = {"i32": np.int32, "i64": np.int64}
NETS, DEG, CELLS = 3000, 5, 4000


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


def _tdt(dt):
    return None if dt is None else torch.from_numpy(np.zeros(0, dt)).dtype


def _pins(seed, base):
    return np.random.default_rng(seed).integers(base, CELLS + base, NETS * DEG)


def _parse(tup, dt):
    def build():
        scheme = 3 if dt is not None else 0

        def text(seed):
            g = np.random.default_rng(seed)
            pins, nw, cw = _pins(seed, 1).reshape(NETS, DEG), g.integers(1, 99999, NETS), g.integers(1, 9999, CELLS)
            lines = [(("%5d " % nw[j]) if scheme else "") + " ".join("%6d" % p for p in pins[j]) for j in range(NETS)]
            tail = " ".join("%4d" % w for w in cw) if scheme else ""
            return ("\n".join(lines) + "\n" + tail).encode()
        ta, tb = text(1), text(2)
        assert len(ta) == len(tb)

        def want(t):
            r = pr.parse_body(t, CELLS, NETS, NETS * DEG, 1, scheme, dt)
            return [r[k].astype(ITYPES[tup]) for k in ("xpin", "pin", "xnet", "net")] + [r["nw"], r["cw"]], None

        def run(ctx, bufs, outs):
            r = ctx.ops.patoh_parse(bufs[0], CELLS, NETS, NETS * DEG, 1, scheme, _tdt(ITYPES[tup]), _tdt(dt))
            return [x for x in r if x is not None], None
        return Job([so._text_t(ta)], [so._text_t(tb)], run, want(ta), want(tb))
    return build


def _transpose(tup):
    def build():
        xpin = (np.arange(NETS + 1) * DEG).astype(ITYPES[tup])

        def want(pin):
            xnet, net = pr.cells_to_nets(xpin, pin, CELLS, 0)
            return [xnet.astype(ITYPES[tup]), net.astype(ITYPES[tup])], None

        def run(ctx, bufs, outs):
            return list(ctx.ops.cells_to_nets(bufs[0], bufs[1], CELLS, 0)), None
        a, b = (_pins(s, 0).astype(ITYPES[tup]) for s in (3, 4))
        return Job([xpin, a], [xpin, b], run, want(a), want(b))
    return build


def _format(tup, dt):
    def build():
        xpin = (np.arange(NETS + 1) * DEG).astype(ITYPES[tup])

        def graph(seed):  # pins and weights of one printed width: 4 and 3 characters
            g = np.random.default_rng(seed)
            return [xpin, g.integers(1000, CELLS, NETS * DEG).astype(ITYPES[tup]),
                    None if dt is None else g.integers(100, 1000, NETS).astype(dt)]

        def want(G):
            return [np.frombuffer(pr.net_lines(G[0], G[1], G[2], 1), np.uint8)], None

        def run(ctx, bufs, outs):
            return [ctx.ops.patoh_format(bufs[0], bufs[1], bufs[2], index_delta=1, net_weights=dt is not None)], None
        A, B = graph(5), graph(6)
        return Job(A, B, run, want(A), want(B))
    return build


def _weights(dt):
    def build():
        w = lambda seed: np.random.default_rng(seed).integers(100, 1000, 20000).astype(dt)
        want = lambda a: ([np.frombuffer(pr.weight_line(a), np.uint8)], None)
        run = lambda ctx, bufs, outs: ([ctx.ops.patoh_format_weights(bufs[0])], None)
        a, b = w(7), w(8)
        return Job([a], [b], run, want(a), want(b))
    return build


case("patoh_parse-i32-f32", "sbhg_patoh_parse", other_stream=True)(_parse("i32", np.float32))
case("patoh_parse-i64-void", "sbhg_patoh_parse")(_parse("i64", None))
case("cells_to_nets-i32", "sbhg_cells_to_nets")(_transpose("i32"))
case("cells_to_nets-i64", "sbhg_cells_to_nets")(_transpose("i64"))
case("patoh_format-i32-f64", "sbhg_patoh_format")(_format("i32", np.float64))
case("patoh_format-i64-void", "sbhg_patoh_format")(_format("i64", None))
case("patoh_format_weights-f32", "sbhg_patoh_format_weights")(_weights(np.float32))
case("patoh_format_weights-i64", "sbhg_patoh_format_weights")(_weights(np.int64))

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
