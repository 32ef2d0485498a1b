"""The stream-order contract (include/sbx.h, Conventions) for the entry points of include/sbio.h, on a caller's stream
that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams fixtures)
with this file's own cases and its own synchronous table.

All three entry points read something back (the token count and the status word, nnz, the range check), so all three
wait for the handle's stream.  Every decoy has the shape of the real input: a text of the same length and token count,
a dense matrix of the same size with the same number of nonzeros elsewhere, a COO of the same length with other
positions — a premature read shows as a wrong value, never as a fault or another size.

tests/test_io_abi.py (no GPU) checks that every name of capi.IO_PROTOTYPES is the target of a case here and has a row in
SYNCHRONOUS.
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

SYNCHRONOUS = {"sbio_mtx_parse_values": True, "sbio_dense_to_coo": True, "sbio_coo_to_dense_vector": True}

CASES = []  # (id, entry point, builder of the Job, read-out modes)
ITYPES = {"i32": np.int32, "i64": np.int64}


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


def _tdt(dt):
    return torch.from_numpy(np.zeros(0, dt)).dtype


def _parse_values(dt):
    def build():
        count = 60000

        def text(seed):  # fixed-width tokens, every one exact in float32: eighths below 2^20
            k = np.random.default_rng(seed).integers(-(1 << 20), 1 << 20, count)
            return "".join("%14.3f\n" % (x / 8.0) for x in k).encode(), (k / 8.0).astype(dt)
        (ta, va), (tb, vb) = text(1), text(2)
        assert len(ta) == len(tb)
        run = lambda ctx, bufs, outs: ([ctx.ops.mtx_parse_values(bufs[0], count, _tdt(dt))], None)
        return Job([so._text_t(ta)], [so._text_t(tb)], run, ([va], None), ([vb], None))
    return build


def _dense_to_coo(tup, dt):
    def build():
        n, m, k = 333, 210, 9000

        def dense(seed):
            g = np.random.default_rng(seed)
            d = np.zeros(n * m, dt)
            cells = g.choice(n * m, k, replace=False)
            d[cells] = g.integers(1, 1000, k).astype(dt)
            return d

        def want(d):
            r, c = np.nonzero(d.reshape(m, n).T)
            return [r.astype(ITYPES[tup]), c.astype(ITYPES[tup]), d.reshape(m, n).T[r, c]], k
        A, B = dense(3), dense(4)

        def run(ctx, bufs, outs):
            r = ctx.ops.dense_to_coo(n, m, bufs[0], _tdt(ITYPES[tup]))
            return list(r), int(r[0].numel())
        return Job([A], [B], run, want(A), want(B))
    return build


def _coo_to_dense_vector(tup, dt, column):
    def build():
        length, k = 50000, 20000

        def entries(seed):
            g = np.random.default_rng(seed)
            pos = np.sort(g.choice(length, k, replace=False)).astype(ITYPES[tup])
            zero = np.zeros(k, ITYPES[tup])
            return [pos, zero, g.integers(1, 1000, k).astype(dt)] if column else [zero, pos, g.integers(1, 1000, k).astype(dt)]

        def want(X):
            out = np.zeros(length, dt)
            out[X[0] + X[1]] = X[2]
            return [out], None
        A, B = entries(5), entries(6)
        run = lambda ctx, bufs, outs: ([ctx.ops.coo_to_dense_vector(length, bufs[0], bufs[1], bufs[2])], None)
        return Job(A, B, run, want(A), want(B))
    return build


case("mtx_parse_values-f32", "sbio_mtx_parse_values", other_stream=True)(_parse_values(np.float32))
case("mtx_parse_values-f64", "sbio_mtx_parse_values")(_parse_values(np.float64))
for _i, _tup in enumerate(ITYPES):
    case(f"dense_to_coo-{_tup}", "sbio_dense_to_coo", other_stream=_i == 0)(_dense_to_coo(_tup, (np.float32, np.float64)[_i]))
    case(f"coo_to_dense_vector-{_tup}", "sbio_coo_to_dense_vector")(_coo_to_dense_vector(_tup, (np.float64, np.int32)[_i], bool(_i)))

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
