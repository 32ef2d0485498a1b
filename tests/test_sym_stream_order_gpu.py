"""The stream-order contract (include/sbx.h, Conventions) for the entry points of include/sbsym.h, on a caller's stream
that is held back: the harness of tests/test_stream_order_gpu.py (Job, held_back, the ctx / delay / streams fixtures)
with this file's own cases and its own synchronous table.

Both entry points read their counts back and wait for the handle's stream; sbsym_csr_symmetrize enqueues the kernels
that write its arrays behind that read-back, so the arrays are read out in stream order (on the caller's stream, and
for one case behind an event on a second stream).  Every decoy has the shape of the real input: the same n, nnz and
row_ptr with the columns renamed and the rows sorted again — a premature read shows as a wrong value, never as a fault
or another size of input.

tests/test_sym_abi.py (no GPU) checks that every name of capi.SYM_PROTOTYPES is the target of a case here and has a row
in SYNCHRONOUS.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symmetrize_restate as sr  # noqa: E402
import test_stream_order_gpu as so  # noqa: E402
from test_stream_order_gpu import Job, ctx, delay, held_back, streams  # noqa: E402,F401  (fixtures by name)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SYNCHRONOUS = {"sbsym_csr_missing_mirrors": True, "sbsym_csr_symmetrize": True}

CASES = []  # (id, entry point, builder of the Job, read-out modes)


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


@functools.lru_cache(None)
def _data():
    """2000 x 2000, 16000 entries with duplicates and self loops, sorted rows; (n, rp, col A, col B)."""
    from sparsebase_amd import synth
    n = 2000
    rp, col = synth.random_rect_csr(n, n, 16000, seed=41, idx_dtype=np.int64, sort_rows=True, dup_frac=0.05)
    return n, rp, col, so._relabel_cols(rp, col, n, 43)


@functools.lru_cache(None)
def _want(which, vb, no_diagonal):
    n, rp, ca, cb = _data()
    c = ca if which == "A" else cb
    return sr.symmetrize(n, rp, c, so._vals(len(c), vb, 5 if which == "A" else 6), no_diagonal)


def _missing(tup):
    def build():
        n, rp, ca, cb = _data()
        ot, idt = so.TUPLES[tup]
        run = lambda ctx, bufs, outs: ([], ctx.ops.csr_missing_mirrors(bufs[0], bufs[1]))
        return Job([so._cast(rp, ot), so._cast(ca, idt)], [so._cast(rp, ot), so._cast(cb, idt)], run,
                   ([], _want("A", 0, False)[3]), ([], _want("B", 0, False)[3]))
    return build


def _symmetrize(tup, vb, no_diagonal):
    def build():
        n, rp, ca, cb = _data()
        ot, idt = so.TUPLES[tup]
        vdt = {0: None, 4: np.float32, 8: np.float64}[vb]
        va, vbb = so._vals(len(ca), vb, 5), so._vals(len(cb), vb, 6)
        cap = 2 * len(ca)
        flags = 1 if no_diagonal else 0

        def run(ctx, bufs, outs):
            import ctypes as C
            hd = ctx.ops.handle_for(bufs[0].device)
            val, vo = (bufs[2], outs[2]) if vb else (None, None)
            k, added = C.c_int64(0), C.c_int64(0)
            hd.check(hd.lib.sbsym_csr_symmetrize(hd.h, ctx.ops._it(bufs[0], bufs[1]), ctx.ops._vt(val), n, bufs[1].numel(),
                                                 ctx.p(bufs[0]), ctx.p(bufs[1]), ctx.p(val), flags, cap, ctx.p(outs[0]),
                                                 ctx.p(outs[1]), ctx.p(vo), C.byref(k), C.byref(added)))
            return [outs[0], outs[1][:k.value]] + ([vo[:k.value]] if vb else []), (k.value, added.value)

        def want(which):
            rpo, co, vo, added = _want(which, vb, no_diagonal)
            return [so._cast(rpo, ot), so._cast(co, idt)] + ([vo] if vb else []), (len(co), added)
        A = [so._cast(rp, ot), so._cast(ca, idt)] + ([va] if vb else [])
        B = [so._cast(rp, ot), so._cast(cb, idt)] + ([vbb] if vb else [])
        return Job(A, B, run, want("A"), want("B"), outs=[(n + 1, ot), (cap, idt)] + ([(cap, vdt)] if vb else []))
    return build


case("csr_missing_mirrors-i32", "sbsym_csr_missing_mirrors")(_missing("i32"))
case("csr_missing_mirrors-i64", "sbsym_csr_missing_mirrors")(_missing("i64"))
case("csr_missing_mirrors-i32_n64", "sbsym_csr_missing_mirrors")(_missing("i32_n64"))
case("csr_symmetrize-i32-v4", "sbsym_csr_symmetrize", other_stream=True)(_symmetrize("i32", 4, False))
case("csr_symmetrize-i64-v8-nodiag", "sbsym_csr_symmetrize")(_symmetrize("i64", 8, True))
case("csr_symmetrize-i32_n64-v0", "sbsym_csr_symmetrize")(_symmetrize("i32_n64", 0, False))

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
