"""The stream-order contract of include/sbx.h, entry point by entry point, on a caller's stream.

include/sbx.h promises (Conventions; "Streams" above sbx_create): work is enqueued on the handle's stream and a caller
orders against that stream only; device outputs are complete in stream order; "synchronous" functions have their status
and `_host` results on return; the private side streams fork from and are joined back into the handle's stream before
the call returns.  Every other GPU test calls the library on the legacy null stream with inputs that were finished
long before, where a launch on the wrong stream, a read-back that waits for the wrong stream or a side stage forked in
front of the caller's producer cannot be seen.

Here every work entry point runs on a NON-BLOCKING caller stream that is HELD BACK, with DECOY inputs in its buffers
until the stream delivers the real ones (`held_back` below):

  1. the call's device buffers hold the decoy B, its outputs a sentinel (0xFF bytes), staging tensors hold A and B;
  2. warm-up on the same stream without delay: the call on A, then on B, each checked against its CPU result (two
     calls: the scratch arena grows in the first call that needs more and is consolidated — a stream synchronise and a
     hipFree — at the start of the next; torch's block pool is per stream; after both the held-back call reaches neither
     hipMalloc nor hipFree, which synchronise the device and would hide an early read);
  3. on the stream: a delay kernel and an event `d` behind it, the copies A -> buffers, `assert not d.query()` (the
     premise: the delay is pending when the call is entered; a case whose premise fails has tested nothing and FAILS),
     the call, `returned_early = not d.query()`, the download of every output into pinned memory (on the same stream,
     or for a subset behind an event on a second non-blocking stream), the clobber B -> input buffers, a synchronise;
  4. outputs and `_host` results equal R(A) bit for bit.  A mismatch is named: equal to R(B) — "inputs read before the
     stream delivered them"; sentinel left — "output not written in stream order"; else the first differing positions.

Decoys are valid inputs of the same shape (same n, m, nnz and dtypes, every id in range, symmetric where the operation
needs it, the same row_ptr wherever the operation reads col), so a premature read computes a well-defined wrong
answer: a bug shows as a wrong value, never as a fault.  Every case asserts R(A) != R(B) on the CPU.

The delay is torch.cuda._sleep, calibrated once per process with two timing events to DELAY_MS = 20 ms.  Measured on
an MI355X: see NOTES.md ("stream-order tests") for the calibration figure (cycles per millisecond) and the length the
calibrated delay then had.  The length is not a pass / fail threshold: premise (3) is.

`returned_early` gives the table of which entry points wait for the stream and which return with their work enqueued
(SYNCHRONOUS below, asserted by test_synchronous_table, printed in INTEGRATION.md).

tests/test_stream_order_table.py (no GPU) checks that every name of capi.PROTOTYPES is the target of a case here or
listed in NOT_STREAM_WORK with its reason.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from sparsebase_amd import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELAY_MS = 20.0

# (offsets, ids): SBX_I32, SBX_I64, SBX_I32_N64
TUPLES = {"i32": (np.int32, np.int32), "i64": (np.int64, np.int64), "i32_n64": (np.int64, np.int32)}
COO_TUPLES = ("i32", "i64")  # entry points without an offset array take SBX_I32_N64 as SBX_I32 (include/sbx.h)

# Entry points that enqueue no work a caller could order against, each with its reason.
NOT_STREAM_WORK = {
    "sbx_version": "a constant",
    "sbx_status_string": "a constant string",
    "sbx_device_count": "device query, no stream",
    "sbx_can_access_peer": "device query, no stream",
    "sbx_create": "handle lifetime",
    "sbx_destroy": "handle lifetime (synchronises the handle's stream and the side streams)",
    "sbx_set_stream": "selects the stream every case here runs on; drains the stream it leaves",
    "sbx_get_device": "a field of the handle",
    "sbx_reserve": "sizes the scratch arena: hipMalloc / hipFree, synchronises by design",
    "sbx_sync": "hipStreamSynchronize of the handle's stream, used by the existing RCM stream test",
    "sbx_last_error": "a field of the handle",
    "sbx_set_oom_hook": "registers a host callback",
    "sbx_profile_enable": "profiler switch: drains its own events",
    "sbx_profile_kernel_count": "a constant",
    "sbx_profile_kernel_name": "a constant string",
    "sbx_profile_query": "profiler: waits for its own events",
    "sbx_profile_query_bytes": "profiler: a host counter",
    "sbx_malloc": "hipMalloc: synchronises the device",
    "sbx_free": "hipFree: synchronises the device",
    "sbx_host_alloc": "page-locked host memory, no stream",
    "sbx_host_free": "page-locked host memory, no stream",
    "sbx_comm_create": "communicator lifetime (tests/test_sharded_gpu.py)",
    "sbx_comm_unique_id": "communicator lifetime (tests/test_sharded_gpu.py)",
    "sbx_comm_create_rccl": "communicator lifetime (tests/test_sharded_gpu.py)",
    "sbx_comm_rank": "a field of the communicator",
    "sbx_comm_destroy": "communicator lifetime (tests/test_sharded_gpu.py)",
    "sbx_permute_csr_sharded": "needs a communicator: exercised in tests/test_sharded_gpu.py",
    "sbx_coo_to_csr_sharded": "needs a communicator: exercised in tests/test_sharded_gpu.py",
    "sbx_csr_to_coo_sharded": "needs a communicator: exercised in tests/test_sharded_gpu.py",
}

# Which entry points wait for the handle's stream before they return (True) and which return with their work enqueued
# (False): `returned_early` of every case, asserted by test_synchronous_table; the table of INTEGRATION.md "Streams".
# A dict: by the part of the case's name that tells the paths apart ("": the others).
SYNCHRONOUS = {
    "sbx_memcpy_h2d": True, "sbx_memcpy_d2h": True, "sbx_memcpy_d2d": True, "sbx_memcpy_peer": True,
    "sbx_coo_is_sorted": True, "sbx_coo_sort": True, "sbx_csr_rows_sorted": True, "sbx_csr_sort_rows": True,
    # (the row test's flag is read back unless the caller vouches for sorted rows; 64-bit row ids are range-checked first)
    "sbx_coo_to_csr": {"": True, "-i32-rows_sorted": False, "-i32_n64-rows_sorted": False}, "sbx_csr_to_coo": False, "sbx_coo_to_csc": True, "sbx_csr_to_csc": True,
    "sbx_mtx_parse_coordinate": True, "sbx_text_count_tokens": True, "sbx_edge_list_parse": True,
    "sbx_csr_degrees": False, "sbx_csr_degree_distribution": False, "sbx_csr_bandwidth": True, "sbx_csr_profile": True,
    "sbx_csr_jaccard_weights": False,  # (its one read-back, the largest degree, is for nnz >= 2^31 only)
    "sbx_csr_triangle_count": True,
    "sbx_degree_reorder": True, "sbx_rcm_reorder": True, "sbx_slashburn_reorder": True, "sbx_boba_reorder": True,
    "sbx_csr_reorder_heatmap": True, "sbx_gray_row_keys": True, "sbx_gray_reorder": True,
    "sbx_inverse_permutation": False, "sbx_permute_csr": True, "sbx_permute_csr_rows": True, "sbx_permute_array": False,
    "sbx_permute_csr_rows_nnz": True, "sbx_balanced_row_splits": True,
}


# ------------------------------------------------------------------------------------------------------------ the cases
class Job:
    """One case's data.  A / B: the real and the decoy inputs (numpy arrays or None, same shapes and dtypes);
    outs: (numel, numpy dtype) of the outputs the harness allocates and fills with the sentinel;
    run(ctx, bufs, outs) -> (device outputs, host result); want_A / want_B: (list of numpy arrays, host result);
    inplace: the inputs are the outputs (no clobber); want_early: what a premature read would give, if not R(B)."""

    def __init__(self, A, B, run, want_A, want_B, outs=(), inplace=False, want_early=None):
        strip = lambda w: None if w is None else ([a for a in w[0] if a is not None], w[1])  # (a value array that is not there)
        self.A, self.B, self.run, self.want_A, self.want_B = list(A), list(B), run, strip(want_A), strip(want_B)
        self.outs, self.inplace, self.want_early = list(outs), inplace, strip(want_early)


CASES = []  # (id, entry point, builder of the Job, read-out modes)


def case(cid, entry, other_stream=False):
    def deco(build):
        CASES.append((cid, entry, build, ("same", "other") if other_stream else ("same",)))
        return build
    return deco


def _cast(a, dt):
    return None if a is None else np.ascontiguousarray(np.asarray(a).astype(dt))


def _vals(count, vb, seed):
    g = np.random.default_rng(seed)
    if vb == 0:
        return None
    return g.integers(-1000, 1000, count).astype(np.float32 if vb == 4 else np.float64)


def _row_ids(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def _relabel_cols(rp, col, m, seed, sort=True):
    """The decoy of a CSR whose operation needs no symmetry: the same row_ptr, every column renamed by one permutation
    of [0, m), the rows sorted again (or left as the renaming leaves them)."""
    q = np.random.default_rng(seed).permutation(m)
    c2 = q[np.asarray(col, np.int64)]
    if sort:
        key = np.sort(_row_ids(rp) * np.int64(m) + c2)
        c2 = key % m
    return c2


def _shuffle_rows(rp, col, seed):
    """Every row's entries in a random order (unsorted input rows)."""
    g = np.random.default_rng(seed)
    o = np.lexsort((g.random(len(col)), _row_ids(rp)))
    return np.asarray(col)[o]


def _relabel_same_degrees(rp, col, seed):
    """The decoy of a symmetric graph: P A P^T for a permutation that maps every vertex to one of the same degree —
    symmetric, rows sorted, the same row_ptr."""
    rp = np.asarray(rp, np.int64)
    n = len(rp) - 1
    deg = np.diff(rp)
    g = np.random.default_rng(seed)
    p = np.empty(n, np.int64)
    p[np.lexsort((np.arange(n), deg))] = np.lexsort((g.random(n), deg))
    rp2, col2 = synth.csr_from_edges(n, p[_row_ids(rp)], p[np.asarray(col, np.int64)], np.int64)
    assert np.array_equal(rp2, rp)
    return col2


def _second_row_ptr(rp, seed):
    """A second monotone row_ptr with the same row_ptr[n]: the degrees in another order."""
    deg = np.random.default_rng(seed).permutation(np.diff(np.asarray(rp, np.int64)))
    return np.concatenate([[0], np.cumsum(deg)])


@functools.lru_cache(None)
def _oracle():
    from orc import Oracle
    return Oracle()


@functools.lru_cache(None)
def _rect(unsorted=False):
    """6000 x 5000, 84000 entries with duplicates; (rp, col A, col B)."""
    n, m = 6000, 5000
    rp, col = synth.random_rect_csr(n, m, 80000, seed=4, idx_dtype=np.int64, sort_rows=True, dup_frac=0.05)
    colb = _relabel_cols(rp, col, m, 9)
    if unsorted:
        col, colb = _shuffle_rows(rp, col, 1), _shuffle_rows(rp, colb, 2)
    return n, m, rp, col, colb


@functools.lru_cache(None)
def _square():
    """5000 x 5000 with unsorted rows, duplicates and self loops (triangle count, slashburn take any such CSR)."""
    n = 5000
    rp, col = synth.random_rect_csr(n, n, 50000, seed=14, idx_dtype=np.int64, sort_rows=False, dup_frac=0.05)
    return n, rp, col, _relabel_cols(rp, col, n, 19, sort=False)


@functools.lru_cache(None)
def _coo(sorted_rows):
    n, m, nnz = 7000, 9000, 90000
    out = []
    for seed in (3, 33):
        row, col, _ = synth.uniform_random_coo(n, m, nnz, seed=seed, idx_dtype=np.int64, shuffled=not sorted_rows)
        out.append((row, col))
    return n, m, out[0], out[1]


def _t(a):
    return None if a is None else torch.from_numpy(a)


# ---- handle utilities: the blocking copies (capi only)
def _memcpy_case(kind):
    def build():
        g = np.random.default_rng(5)
        nwords = 1 << 18
        a, b, hsrc = (g.integers(0, 1 << 30, nwords).astype(np.int32) for _ in range(3))
        nbytes = nwords * 4
        if kind == "h2d":
            # the stream's copy A -> buffer comes first in stream order, the library's copy of the host words lands on
            # top of it; issued in front of the stream's work it would be overwritten by A
            def run(ctx, bufs, outs):
                ctx.check(ctx.lib.sbx_memcpy_h2d(ctx.h, ctx.p(bufs[0]), hsrc.ctypes.data_as(C.c_void_p), nbytes))
                return [bufs[0]], None
            return Job([a], [b], run, ([hsrc], None), ([hsrc], None), inplace=True, want_early=([a], None))
        if kind == "d2h":
            def run(ctx, bufs, outs):
                got = np.full(nwords, -1, np.int32)
                ctx.check(ctx.lib.sbx_memcpy_d2h(ctx.h, got.ctypes.data_as(C.c_void_p), ctx.p(bufs[0]), nbytes))
                return [], got.tobytes()
            return Job([a], [b], run, ([], a.tobytes()), ([], b.tobytes()))

        def run(ctx, bufs, outs):
            if kind == "d2d":
                ctx.check(ctx.lib.sbx_memcpy_d2d(ctx.h, ctx.p(outs[0]), ctx.p(bufs[0]), nbytes))
            else:  # the peer copy between two buffers of the handle's own device
                dev = torch.cuda.current_device()
                ctx.check(ctx.lib.sbx_memcpy_peer(ctx.h, ctx.p(outs[0]), dev, ctx.p(bufs[0]), dev, nbytes))
            return [outs[0]], None
        return Job([a], [b], run, ([a], None), ([b], None), outs=[(nwords, np.int32)])
    return build


for _k in ("h2d", "d2h", "d2d", "peer"):
    case(f"memcpy_{_k}", f"sbx_memcpy_{_k}", other_stream=_k == "d2d")(_memcpy_case(_k))


# ---- constructors and checks
def _coo_is_sorted(tup):
    def build():
        n, m, (ra, ca), _ = _coo(True)
        _, _, (rb, cb), _ = _coo(False)
        idt = TUPLES[tup][1]
        run = lambda ctx, bufs, outs: ([], ctx.ops.coo_is_sorted(bufs[0], bufs[1]))
        orc = _oracle()
        return Job([_cast(ra, idt), _cast(ca, idt)], [_cast(rb, idt), _cast(cb, idt)], run,
                   ([], orc.coo_is_sorted(_cast(ra, idt), _cast(ca, idt))), ([], orc.coo_is_sorted(_cast(rb, idt), _cast(cb, idt))))
    return build


def _coo_sort(tup, vb):
    def build():
        n, m, (ra, ca), (rb, cb) = _coo(False)
        idt = TUPLES[tup][1]
        A = [_cast(ra, idt), _cast(ca, idt), _vals(len(ra), vb, 1)]
        B = [_cast(rb, idt), _cast(cb, idt), _vals(len(rb), vb, 2)]

        def run(ctx, bufs, outs):
            ctx.ops.coo_sort_(n, m, bufs[0], bufs[1], bufs[2])
            return list(bufs), None
        orc = _oracle()
        return Job(A, B, run, (list(orc.coo_sort(*A)), None), (list(orc.coo_sort(*B)), None), inplace=True)
    return build


def _csr_rows_sorted(tup):
    def build():
        n, m, rp, ca, _ = _rect(True)     # unsorted: 0
        _, _, _, _, cb = _rect(False)     # sorted: 1
        ot, idt = TUPLES[tup]
        run = lambda ctx, bufs, outs: ([], ctx.ops.csr_rows_sorted(bufs[0], bufs[1]))
        orc = _oracle()
        wa, wb = orc.csr_rows_sorted(rp, ca), orc.csr_rows_sorted(rp, cb)
        return Job([_cast(rp, ot), _cast(ca, idt)], [_cast(rp, ot), _cast(cb, idt)], run, ([], wa), ([], wb))
    return build


def _csr_sort_rows(tup, vb):
    def build():
        n, m, rp, ca, cb = _rect(True)
        ot, idt = TUPLES[tup]
        va, vbb = _vals(len(ca), vb, 3), _vals(len(cb), vb, 4)

        def run(ctx, bufs, outs):
            ctx.ops.csr_sort_rows_(n, m, bufs[0], bufs[1], bufs[2])
            return [bufs[1], bufs[2]], None
        orc = _oracle()

        def want(c, v):
            wc, wv = orc.csr_sort_rows(rp, c, v)
            return [_cast(wc, idt), wv], None
        return Job([_cast(rp, ot), _cast(ca, idt), va], [_cast(rp, ot), _cast(cb, idt), vbb], run, want(ca, va), want(cb, vbb),
                   inplace=True)
    return build


for _i, _tup in enumerate(COO_TUPLES):
    case(f"coo_is_sorted-{_tup}", "sbx_coo_is_sorted")(_coo_is_sorted(_tup))
    case(f"coo_sort-{_tup}-v0", "sbx_coo_sort")(_coo_sort(_tup, 0))
    case(f"coo_sort-{_tup}-v{4 + 4 * _i}", "sbx_coo_sort", other_stream=_i == 1)(_coo_sort(_tup, 4 + 4 * _i))
for _i, _tup in enumerate(TUPLES):
    case(f"csr_rows_sorted-{_tup}", "sbx_csr_rows_sorted")(_csr_rows_sorted(_tup))
    case(f"csr_sort_rows-{_tup}-v{(0, 4, 8)[_i]}", "sbx_csr_sort_rows")(_csr_sort_rows(_tup, (0, 4, 8)[_i]))


# ---- conversions
def _coo_to_csr(tup, vb, move, rows_sorted):
    def build():
        n, m, (ra, ca), (rb, cb) = _coo(rows_sorted)
        ot, idt = TUPLES[tup]
        nnz = len(ra)
        A = [_cast(ra, idt), _cast(ca, idt), _vals(nnz, vb, 5)]
        B = [_cast(rb, idt), _cast(cb, idt), _vals(nnz, vb, 6)]
        vdt = None if vb == 0 else A[2].dtype
        outs = [(n + 1, ot)] + ([] if move else [(nnz, idt)] + ([(nnz, vdt)] if vb else []))

        def run(ctx, bufs, outs):
            o = (outs[0], None, None) if move else (outs[0], outs[1], outs[2] if vb else None)
            ctx.ops.coo_to_csr(n, m, bufs[0], bufs[1], bufs[2], move=move, rows_sorted=rows_sorted, out=o)
            return list(outs), None
        orc = _oracle()

        def want(X):
            rp, co, vo = orc.coo_to_csr(n, X[0], X[1], X[2])
            w = [_cast(rp, ot)] + ([] if move else [_cast(co, idt)] + ([vo] if vb else []))
            return w, None
        return Job(A, B, run, want(A), want(B), outs=outs)
    return build


def _csr_to_coo(tup, vb):
    def build():
        n, m, rp, ca, cb = _rect()
        ot, idt = TUPLES[tup]
        nnz = len(ca)
        va, vbb = _vals(nnz, vb, 7), _vals(nnz, vb, 8)
        outs = [(nnz, idt), (nnz, idt)] + ([(nnz, va.dtype)] if vb else [])

        def run(ctx, bufs, outs):
            ctx.ops.csr_to_coo(n, m, bufs[0], bufs[1], bufs[2], out=(outs[0], outs[1], outs[2] if vb else None))
            return list(outs), None
        orc = _oracle()

        def want(c, v):
            ro, co, vo = orc.csr_to_coo(rp, c, v)
            return [_cast(ro, idt), _cast(co, idt)] + ([vo] if vb else []), None
        return Job([_cast(rp, ot), _cast(ca, idt), va], [_cast(rp, ot), _cast(cb, idt), vbb], run, want(ca, va), want(cb, vbb),
                   outs=outs)
    return build


def _to_csc(tup, vb, from_csr):
    def build():
        ot, idt = TUPLES[tup]
        orc = _oracle()
        if from_csr:
            n, m, rp, ca, cb = _rect()
            va, vbb = _vals(len(ca), vb, 9), _vals(len(cb), vb, 10)
            A, B = [_cast(rp, ot), _cast(ca, idt), va], [_cast(rp, ot), _cast(cb, idt), vbb]
            run = lambda ctx, bufs, outs: ([x for x in ctx.ops.csr_to_csc(n, m, bufs[0], bufs[1], bufs[2]) if x is not None], None)
            want = lambda X: orc.csr_to_csc(m, rp, np.asarray(X[1], np.int64), X[2])
        else:
            n, m, (ra, ca), (rb, cb) = _coo(False)
            A = [_cast(ra, idt), _cast(ca, idt), _vals(len(ra), vb, 11)]
            B = [_cast(rb, idt), _cast(cb, idt), _vals(len(rb), vb, 12)]
            run = lambda ctx, bufs, outs: ([x for x in ctx.ops.coo_to_csc(n, m, bufs[0], bufs[1], bufs[2],
                                                                          offset_dtype=_t(np.zeros(0, ot)).dtype) if x is not None], None)
            want = lambda X: orc.coo_to_csc(n, m, np.asarray(X[0], np.int64), np.asarray(X[1], np.int64), X[2])

        def wants(X):
            cp, ro, vo = want(X)
            return [_cast(cp, ot), _cast(ro, idt)] + ([vo] if vb else []), None
        return Job(A, B, run, wants(A), wants(B))
    return build


for _i, _tup in enumerate(TUPLES):
    case(f"coo_to_csr-{_tup}-plain-v4", "sbx_coo_to_csr", other_stream=_i == 0)(_coo_to_csr(_tup, 4, False, False))
    case(f"coo_to_csr-{_tup}-move-v0", "sbx_coo_to_csr")(_coo_to_csr(_tup, 0, True, False))
    case(f"coo_to_csr-{_tup}-rows_sorted-v8", "sbx_coo_to_csr")(_coo_to_csr(_tup, 8, False, True))
    case(f"csr_to_coo-{_tup}-v{(4, 8, 0)[_i]}", "sbx_csr_to_coo")(_csr_to_coo(_tup, (4, 8, 0)[_i]))
    case(f"coo_to_csc-{_tup}-v{(8, 0, 4)[_i]}", "sbx_coo_to_csc", other_stream=_i == 2)(_to_csc(_tup, (8, 0, 4)[_i], False))
    case(f"csr_to_csc-{_tup}-v{(0, 4, 8)[_i]}", "sbx_csr_to_csc")(_to_csc(_tup, (0, 4, 8)[_i], True))


# ---- text
def _coord_text(seed, n, m, L, symmetric, weighted, zero_based=False):
    """L fixed-width lines "row col [value]": every text of one (n, m, L) has the same byte length and entry count.
    Symmetric: the first 5 entries on the diagonal, the others strictly below it; coordinates distinct."""
    g = np.random.default_rng(seed)
    if symmetric:
        key = g.choice(n * m, 3 * L, replace=False)
        r, c = key // m, key % m
        keep = np.nonzero(r > c)[0][:L]
        r, c = r[keep], c[keep].copy()
        c[:5] = r[:5]
        assert len(r) == L and len(np.unique(r * m + c)) == L
    else:
        key = g.choice(n * m, L, replace=False)
        r, c = key // m, key % m
    base = 0 if zero_based else 1
    v = g.standard_normal(L) * 10.0 ** g.integers(-20, 20, L)
    return "".join("%8d %8d%s\n" % (r[i] + base, c[i] + base, (" %24.16e" % v[i]) if weighted else "") for i in range(L)).encode()


def _text_t(b):
    return np.frombuffer(b, np.uint8).copy()


@case("text_count_tokens", "sbx_text_count_tokens")
def _count_tokens():
    a = _coord_text(1, 3000, 3000, 20000, False, True)
    b = bytearray(_coord_text(2, 3000, 3000, 20000, False, True))
    for i in range(1000):  # a blank in the middle of the mantissa: one token more
        b[i * 43 + 30] = 32
    run = lambda ctx, bufs, outs: ([], ctx.ops.text_count_tokens(bufs[0]))
    return Job([_text_t(a)], [_text_t(bytes(b))], run, ([], len(a.split())), ([], len(bytes(b).split())))


def _mtx(tup, symmetric, vb):
    def build():
        n = m = 4000
        L = 30000
        idt = TUPLES[tup][1]
        vdt = {0: None, 4: np.float32, 8: np.float64}[vb]
        ta, tb = (_coord_text(s, n, m, L, symmetric, True) for s in (3, 4))
        assert len(ta) == len(tb)

        def run(ctx, bufs, outs):
            r = ctx.ops.mtx_parse_coordinate(bufs[0], n, m, L, 3, 1 if symmetric else 0, True, False, _t(np.zeros(0, idt)).dtype,
                                             None if vdt is None else _t(np.zeros(0, vdt)).dtype)
            return [x for x in r if x is not None], int(r[0].numel())
        orc = _oracle()

        def want(t):
            r, c, v = orc.mtx_parse(t, L, 3, 1 if symmetric else 0, True, False, idt, vdt)
            return [r, c] + ([v] if vb else []), len(r)
        return Job([_text_t(ta)], [_text_t(tb)], run, want(ta), want(tb))
    return build


def _edges(tup, weighted):
    def build():
        idt = TUPLES[tup][1]
        vdt = np.float32 if weighted else None
        E, n = 25000, 3000

        def text(seed):  # distinct pairs u < v: with the reverse edges every coordinate occurs once (the sort is stable
            g = np.random.default_rng(seed)  # here, unspecified in the reference)
            key = g.choice(n * n, 3 * E, replace=False)
            u, v = key // n, key % n
            keep = np.nonzero(u < v)[0][:E]
            w = g.integers(-500, 500, E) / 8.0
            return "".join("%6d %6d%s\n" % (u[k], v[k], (" %9.3f" % w[i]) if weighted else "") for i, k in enumerate(keep)).encode()
        ta, tb = text(5), text(6)
        assert len(ta) == len(tb)

        def run(ctx, bufs, outs):
            r = ctx.ops.edge_list_parse(bufs[0], weighted=weighted, index_dtype=_t(np.zeros(0, idt)).dtype,
                                        value_dtype=None if vdt is None else torch.float32)
            return [x for x in r[2:] if x is not None], (int(r[0]), int(r[1]))
        orc = _oracle()

        def want(t):
            r = orc.edge_list_parse(t, weighted, False, False, True, False, idt, vdt)
            return [r[2], r[3]] + ([r[4]] if weighted else []), (int(r[0]), int(r[1]))
        return Job([_text_t(ta)], [_text_t(tb)], run, want(ta), want(tb))
    return build


for _i, _tup in enumerate(COO_TUPLES):
    case(f"mtx_parse-{_tup}-general-v8", "sbx_mtx_parse_coordinate", other_stream=_i == 0)(_mtx(_tup, False, 8))
    case(f"mtx_parse-{_tup}-symmetric-v4", "sbx_mtx_parse_coordinate")(_mtx(_tup, True, 4))
    case(f"edge_list_parse-{_tup}-{'weighted' if _i else 'plain'}", "sbx_edge_list_parse")(_edges(_tup, bool(_i)))


# ---- features
@functools.lru_cache(None)
def _row_ptrs():
    rp, _ = synth.rmat_symmetric(14, 8, seed=6, idx_dtype=np.int64)
    return rp, _second_row_ptr(rp, 7)


def _degrees(tup):
    def build():
        ra, rb = _row_ptrs()
        ot, idt = TUPLES[tup]
        run = lambda ctx, bufs, outs: ([ctx.ops.csr_degrees(bufs[0], id_dtype=_t(np.zeros(0, idt)).dtype)], None)
        return Job([_cast(ra, ot)], [_cast(rb, ot)], run, ([_cast(np.diff(ra), idt)], None), ([_cast(np.diff(rb), idt)], None))
    return build


def _degree_distribution(tup, fb):
    def build():
        ra, rb = _row_ptrs()
        ot = TUPLES[tup][0]
        fdt = np.float32 if fb == 4 else np.float64
        nnz = int(ra[-1])
        run = lambda ctx, bufs, outs: ([ctx.ops.csr_degree_distribution(bufs[0], nnz, dtype=_t(np.zeros(0, fdt)).dtype)], None)
        orc = _oracle()
        want = lambda r: ([orc.csr_degree_distribution(_cast(r, ot), nnz, fdt)], None)
        return Job([_cast(ra, ot)], [_cast(rb, ot)], run, want(ra), want(rb))
    return build


def _scalar_feature(tup, name):
    def build():
        n, rp, ca, cb = _square()
        ca, cb = _relabel_cols(rp, ca, n, 0), _relabel_cols(rp, cb, n, 1)  # (sorted rows)
        ot, idt = TUPLES[tup]
        run = lambda ctx, bufs, outs: ([], getattr(ctx.ops, name)(bufs[0], bufs[1]))
        orc = _oracle()
        want = lambda c: ([], getattr(orc, name)(rp, c))
        return Job([_cast(rp, ot), _cast(ca, idt)], [_cast(rp, ot), _cast(cb, idt)], run, want(ca), want(cb))
    return build


@functools.lru_cache(None)
def _jaccard_data():
    from test_jaccard_gpu import _hub_pairs
    from test_jaccard_host import jaccard_reference
    # two hubs of 40000 neighbours, adjacent to each other: beyond the LDS bin of either id width (16384 / 8192 ids):
    # the workgroup-per-edge path with its read-back
    rp, col = _hub_pairs([40000, 9000, 129, 17, 5], 60000, seed=11)
    colb = _relabel_same_degrees(rp, col, 12)
    return rp, col, colb, jaccard_reference(rp, col), jaccard_reference(rp, colb)


def _jaccard(tup, fb):
    def build():
        rp, ca, cb, wa, wb = _jaccard_data()
        ot, idt = TUPLES[tup]
        fdt = np.float32 if fb == 4 else np.float64
        run = lambda ctx, bufs, outs: ([ctx.ops.csr_jaccard_weights(bufs[0], bufs[1], dtype=_t(np.zeros(0, fdt)).dtype)], None)
        return Job([_cast(rp, ot), _cast(ca, idt)], [_cast(rp, ot), _cast(cb, idt)], run, ([wa.astype(fdt)], None),
                   ([wb.astype(fdt)], None))
    return build


def _triangles(tup, directed, exact):
    def build():
        from test_triangle_count_host import tc_exact, tc_reference
        n, rp, ca, cb = _square()
        ot, idt = TUPLES[tup]
        run = lambda ctx, bufs, outs: ([], ctx.ops.csr_triangle_count(bufs[0], bufs[1], directed=directed, exact=exact))
        f = tc_exact if exact else tc_reference
        return Job([_cast(rp, ot), _cast(ca, idt)], [_cast(rp, ot), _cast(cb, idt)], run, ([], int(f(rp, ca, directed))),
                   ([], int(f(rp, cb, directed))))
    return build


for _i, _tup in enumerate(TUPLES):
    case(f"csr_degrees-{_tup}", "sbx_csr_degrees", other_stream=_i == 0)(_degrees(_tup))
    case(f"csr_bandwidth-{_tup}", "sbx_csr_bandwidth")(_scalar_feature(_tup, "csr_bandwidth"))
    case(f"csr_profile-{_tup}", "sbx_csr_profile")(_scalar_feature(_tup, "csr_profile"))
    case(f"csr_jaccard_weights-{_tup}-f{(4, 8, 4)[_i]}", "sbx_csr_jaccard_weights", other_stream=_i == 1)(_jaccard(_tup, (4, 8, 4)[_i]))
    for _d in (False, True):
        for _e in (False, True):
            case(f"csr_triangle_count-{_tup}-{'directed' if _d else 'undirected'}-{'exact' if _e else 'reference'}",
                 "sbx_csr_triangle_count", other_stream=(_i == 2 and _d and _e))(_triangles(_tup, _d, _e))
for _tup, _fb in (("i32", 4), ("i32", 8), ("i64", 4), ("i64", 8)):
    case(f"csr_degree_distribution-{_tup}-f{_fb}", "sbx_csr_degree_distribution")(_degree_distribution(_tup, _fb))


# ---- orderings
def _degree_reorder(tup, ascending):
    def build():
        ra, rb = _row_ptrs()
        ot, idt = TUPLES[tup]
        n = len(ra) - 1

        def run(ctx, bufs, outs):
            ctx.ops.degree_reorder(bufs[0], ascending, out=outs[0])
            return [outs[0]], None
        orc = _oracle()
        want = lambda r: ([_cast(orc.degree_reorder(r, ascending), idt)], None)
        return Job([_cast(ra, ot)], [_cast(rb, ot)], run, want(ra), want(rb), outs=[(n, idt)])
    return build


@functools.lru_cache(None)
def _rcm_data(kind):
    if kind == "rmat18":  # the graph of test_rcm_on_a_callers_nonblocking_stream_the_way_a_c_caller_reads_it
        rp, col = synth.rmat_symmetric(18, 12, seed=21, idx_dtype=np.int64)
    elif kind == "rmat14":
        rp, col = synth.rmat_symmetric(14, 8, seed=3, idx_dtype=np.int64)
    else:
        # one power-law component the host searches first (it holds vertex 0) beside 300 components of 65 .. 420
        # vertices: their labelling runs on a side stream behind the search's first kernels
        from test_gpu_parity import _many_components
        r1, c1 = synth.rmat_symmetric(15, 8, seed=8, idx_dtype=np.int64)
        r2, c2 = _many_components(300, 4)
        n1 = len(r1) - 1
        src = np.concatenate([_row_ids(r1), _row_ids(np.asarray(r2, np.int64)) + n1])
        dst = np.concatenate([c1, np.asarray(c2, np.int64) + n1])
        rp, col = synth.csr_from_edges(n1 + len(r2) - 1, src, dst, np.int64)
    colb = _relabel_same_degrees(rp, col, 31)
    orc = _oracle()
    return rp, col, colb, orc.rcm_reorder(rp, col), orc.rcm_reorder(rp, colb)


def _rcm(tup, kind):
    def build():
        rp, ca, cb, wa, wb = _rcm_data(kind)
        ot, idt = TUPLES[tup]

        def run(ctx, bufs, outs):
            ctx.ops.rcm_reorder(bufs[0], bufs[1], out=outs[0])
            return [outs[0]], None
        return Job([_cast(rp, ot), _cast(ca, idt)], [_cast(rp, ot), _cast(cb, idt)], run, ([_cast(wa, idt)], None),
                   ([_cast(wb, idt)], None), outs=[(len(rp) - 1, idt)])
    return build


@functools.lru_cache(None)
def _slashburn_data(greedy):
    from test_slashburn_host import slashburn
    n, rp, ca, cb = _square()
    k = 40  # several rounds
    return rp, ca, cb, slashburn(rp, ca, k, greedy, False), slashburn(rp, cb, k, greedy, False), k


def _slashburn(tup, greedy):
    def build():
        rp, ca, cb, wa, wb, k = _slashburn_data(greedy)
        ot, idt = TUPLES[tup]

        def run(ctx, bufs, outs):
            _, st = ctx.ops.slashburn_reorder(bufs[0], bufs[1], k, greedy=greedy, out=outs[0], return_stats=True)
            return [outs[0]], st["rounds"] >= 2
        return Job([_cast(rp, ot), _cast(ca, idt)], [_cast(rp, ot), _cast(cb, idt)], run, ([_cast(wa, idt)], True),
                   ([_cast(wb, idt)], True), outs=[(len(rp) - 1, idt)])
    return build


def _boba(tup):
    def build():
        from test_boba_host import boba
        n, m, (ra, ca), (rb, cb) = _coo(False)
        idt = TUPLES[tup][1]

        def run(ctx, bufs, outs):
            ctx.ops.boba_reorder(bufs[0], bufs[1], n, m, out=outs[0])
            return [outs[0]], None
        return Job([_cast(ra, idt), _cast(ca, idt)], [_cast(rb, idt), _cast(cb, idt)], run, ([_cast(boba(ra, ca, n, m), idt)], None),
                   ([_cast(boba(rb, cb, n, m), idt)], None), outs=[(max(n, m), idt)])
    return build


def _heatmap(tup, b, double):
    def build():
        from test_reorder_heatmap_host import heatmap
        rp, ca = synth.rmat_symmetric(13, 8, seed=4, idx_dtype=np.int64)
        n = len(rp) - 1
        cb = _relabel_cols(rp, ca, n, 41)
        g = np.random.default_rng(b)
        oa, ob = (g.permutation(n), g.permutation(n)), (g.permutation(n), g.permutation(n))
        ot, idt = TUPLES[tup]
        fdt = np.float64 if double else np.float32
        run = lambda ctx, bufs, outs: ([ctx.ops.csr_reorder_heatmap(bufs[0], bufs[1], bufs[2], bufs[3], b, double=double)], None)
        want = lambda c, o: ([heatmap(rp, c, o[0], o[1], b).astype(fdt)], None)
        return Job([_cast(rp, ot), _cast(ca, idt), _cast(oa[0], idt), _cast(oa[1], idt)],
                   [_cast(rp, ot), _cast(cb, idt), _cast(ob[0], idt), _cast(ob[1], idt)], run, want(ca, oa), want(cb, ob))
    return build


@functools.lru_cache(None)
def _gray_data(kind):
    if kind == "banded":
        rp, col = synth.banded_symmetric(16384, 40, 9, 3, idx_dtype=np.int64)
        m = len(rp) - 1
        key = np.sort(_row_ids(rp) * np.int64(m) + (np.asarray(col, np.int64) + 5) % m)  # the band moved by five columns
        colb = key % m
    else:  # power law: rows of every class, a hub of 40000 entries (test_gray_row_keys_power_law_path)
        g = np.random.default_rng(1042)
        n, m = 3000, 32 * 1024
        lens = g.integers(0, 65, n)
        lens[g.integers(0, n, 400)] = g.integers(65, 1025, 400)
        lens[g.integers(0, n, 60)] = g.integers(1025, 9000, 60)
        lens[[5, 6, 7]] = (40000, 1024, 1025)
        lens = np.minimum(lens, m)
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        col = np.concatenate([np.sort(g.choice(m, int(l), replace=False)) for l in lens]).astype(np.int64)
        colb = _relabel_cols(rp, col, m, 43)
    return rp, col, colb, m


def _gray_row_keys(tup, kind):
    def build():
        rp, ca, cb, m = _gray_data(kind)
        ot, idt = TUPLES[tup]
        res, thr = 32, 10

        def run(ctx, bufs, outs):
            deg, key, counts = ctx.ops.gray_row_keys(m, bufs[0], bufs[1], res, thr)
            return [deg, key], [int(x) for x in counts]
        orc = _oracle()

        def want(c):
            deg, key, counts = orc.gray_row_keys(rp, c, m, res, thr)
            return [_cast(deg, idt), key.view(np.int64)], counts.tolist()
        return Job([_cast(rp, ot), _cast(ca, idt)], [_cast(rp, ot), _cast(cb, idt)], run, want(ca), want(cb))
    return build


def _gray_reorder(tup):
    def build():
        from test_gpu_parity import _gray_stable_model
        rp, ca = synth.rmat_symmetric(13, 8, seed=5, idx_dtype=np.int64)
        n = len(rp) - 1
        cb = _relabel_same_degrees(rp, ca, 47)
        ot, idt = TUPLES[tup]
        res, thr, grp = 32, 10, 4
        run = lambda ctx, bufs, outs: ([ctx.ops.gray_reorder(n, bufs[0], bufs[1], res, thr, grp)], None)
        orc = _oracle()

        def want(c):
            deg, key, counts = orc.gray_row_keys(rp, c, n, res, thr)
            return [_cast(_gray_stable_model(deg, key, counts, min(res, n), thr, grp)[0], idt)], None
        return Job([_cast(rp, ot), _cast(ca, idt)], [_cast(rp, ot), _cast(cb, idt)], run, want(ca), want(cb))
    return build


def _inverse_permutation(tup):
    def build():
        idt = TUPLES[tup][1]
        pa, pb = synth.random_permutation(100000, 1, idt), synth.random_permutation(100000, 2, idt)
        run = lambda ctx, bufs, outs: ([ctx.ops.inverse_permutation(bufs[0])], None)
        orc = _oracle()
        return Job([pa], [pb], run, ([orc.inverse_permutation(pa)], None), ([orc.inverse_permutation(pb)], None))
    return build


for _i, _tup in enumerate(TUPLES):
    case(f"degree_reorder-{_tup}-ascending", "sbx_degree_reorder", other_stream=_i == 0)(_degree_reorder(_tup, True))
    case(f"degree_reorder-{_tup}-descending", "sbx_degree_reorder")(_degree_reorder(_tup, False))
    case(f"rcm_reorder-{_tup}-{'rmat18' if _i == 0 else 'rmat14'}", "sbx_rcm_reorder", other_stream=_i < 2)(
        _rcm(_tup, "rmat18" if _i == 0 else "rmat14"))
    case(f"rcm_reorder-{_tup}-components", "sbx_rcm_reorder")(_rcm(_tup, "components"))
    case(f"slashburn_reorder-{_tup}-default", "sbx_slashburn_reorder", other_stream=_i == 0)(_slashburn(_tup, False))
    case(f"slashburn_reorder-{_tup}-greedy", "sbx_slashburn_reorder")(_slashburn(_tup, True))
    case(f"csr_reorder_heatmap-{_tup}-b{(32, 128, 300)[_i]}", "sbx_csr_reorder_heatmap", other_stream=_i == 1)(
        _heatmap(_tup, (32, 128, 300)[_i], _i == 1))
    case(f"gray_row_keys-{_tup}-banded", "sbx_gray_row_keys", other_stream=_i < 2)(_gray_row_keys(_tup, "banded"))
    case(f"gray_row_keys-{_tup}-power_law", "sbx_gray_row_keys")(_gray_row_keys(_tup, "power_law"))
    case(f"gray_reorder-{_tup}", "sbx_gray_reorder", other_stream=_i == 0)(_gray_reorder(_tup))
for _i, _tup in enumerate(COO_TUPLES):
    case(f"boba_reorder-{_tup}", "sbx_boba_reorder", other_stream=_i == 0)(_boba(_tup))
    case(f"inverse_permutation-{_tup}", "sbx_inverse_permutation")(_inverse_permutation(_tup))


# ---- permutes
def _pick(g, m, count):
    """`count` distinct sorted columns below m."""
    c = np.unique(g.integers(0, m, int(count * 1.4) + 8))
    if len(c) < count:
        return np.sort(g.choice(m, count, replace=False))
    return np.sort(g.permutation(c)[:count])


@functools.lru_cache(None)
def _permute_data(unsorted):
    """Tile rows (up to 128 entries), block rows of every class (129 .. 8192) and long rows (above), m = 2^18."""
    g = np.random.default_rng(41)
    m = 1 << 18
    lens = [int(x) for x in g.integers(0, 100, 2500)]
    lens += [129, 131, 255, 257, 511, 513, 1023, 1026, 2047, 2049, 4095, 4098, 8190, 8192, 700, 3001, 6002, 1, 0, 5, 300]
    lens += [8193, 12000, 70000, 16385]
    lens = [lens[i] for i in g.permutation(len(lens))]
    n = len(lens)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([_pick(g, m, l) for l in lens]).astype(np.int64)
    colb = _relabel_cols(rp, col, m, 51)
    if unsorted:
        col, colb = _shuffle_rows(rp, col, 52), _shuffle_rows(rp, colb, 53)
    orders = [(synth.random_permutation(n, s, np.int64), synth.random_permutation(m, s + 1, np.int64)) for s in (60, 70)]
    return n, m, rp, col, colb, orders


def _permute_inputs(tup, vb, mode, unsorted):
    n, m, rp, ca, cb, (oa, ob) = _permute_data(unsorted)
    ot, idt = TUPLES[tup]
    use_r, use_c = mode in ("rows", "both"), mode in ("cols", "both")
    A = [_cast(rp, ot), _cast(ca, idt), _vals(len(ca), vb, 61), _cast(oa[0], idt) if use_r else None, _cast(oa[1], idt) if use_c else None]
    B = [_cast(rp, ot), _cast(cb, idt), _vals(len(cb), vb, 62), _cast(ob[0], idt) if use_r else None, _cast(ob[1], idt) if use_c else None]
    return n, m, A, B


def _oracle_permute(X):
    orc = _oracle()
    i64 = lambda a: None if a is None else np.asarray(a, np.int64)
    return orc.permute_csr(i64(X[0]), i64(X[1]), X[2], i64(X[3]), i64(X[4]))


def _permute_csr(tup, vb, mode, unsorted):
    def build():
        n, m, A, B = _permute_inputs(tup, vb, mode, unsorted)
        ot, idt = TUPLES[tup]
        nnz = len(A[1])
        outs = [(n + 1, ot), (nnz, idt)] + ([(nnz, A[2].dtype)] if vb else [])

        def run(ctx, bufs, outs):
            ctx.ops.permute_csr(n, m, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], out=(outs[0], outs[1], outs[2] if vb else None))
            return list(outs), None

        def want(X):
            rpo, co, vo = _oracle_permute(X)
            return [_cast(rpo, ot), _cast(co, idt)] + ([vo] if vb else []), None
        return Job(A, B, run, want(A), want(B), outs=outs)
    return build


def _shard_of(whole, r0, r1, ot, idt, vb):
    a, b = int(whole[0][r0]), int(whole[0][r1])
    return [_cast(whole[0][r0:r1 + 1] - a, ot), _cast(whole[1][a:b], idt)] + ([whole[2][a:b]] if vb else []), b - a


def _permute_csr_rows(tup, vb):
    def build():
        n, m, A, B = _permute_inputs(tup, vb, "both", False)
        ot, idt = TUPLES[tup]
        r0, r1 = n // 3, 2 * n // 3

        def run(ctx, bufs, outs):
            r = ctx.ops.permute_csr_rows(n, m, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], r0, r1)
            return [x for x in r if x is not None], int(r[1].numel())
        return Job(A, B, run, _shard_of(_oracle_permute(A), r0, r1, ot, idt, vb), _shard_of(_oracle_permute(B), r0, r1, ot, idt, vb))
    return build


def _permute_csr_rows_null(tup, vb):
    """shard_nnz_host = NULL: ops always passes the pointer, so through capi on the test's own handle."""
    def build():
        from sparsebase_amd import capi
        n, m, A, B = _permute_inputs(tup, vb, "both", False)
        ot, idt = TUPLES[tup]
        nnz = len(A[1])
        r0, r1 = n // 3, 2 * n // 3
        it = {"i32": capi.SBX_I32, "i64": capi.SBX_I64, "i32_n64": capi.SBX_I32_N64}[tup]
        vt = {0: capi.V_NONE, 4: capi.V_F32, 8: capi.V_F64}[vb]
        outs = [(r1 - r0 + 1, ot), (nnz, idt)] + ([(nnz, A[2].dtype)] if vb else [])

        def run(ctx, bufs, outs):
            ctx.check(ctx.lib.sbx_permute_csr_rows(ctx.h, it, vt, n, m, nnz, ctx.p(bufs[0]), ctx.p(bufs[1]), ctx.p(bufs[2]),
                                                   ctx.p(bufs[3]), ctx.p(bufs[4]), r0, r1, ctx.p(outs[0]), ctx.p(outs[1]),
                                                   ctx.p(outs[2]) if vb else None, nnz, None))
            return list(outs), None

        def want(X):  # (the slabs have room for every entry: behind the shard's the sentinel stays)
            w, k = _shard_of(_oracle_permute(X), r0, r1, ot, idt, vb)
            pad = lambda a: np.concatenate([a, np.frombuffer(b"\xff" * ((nnz - k) * a.itemsize), a.dtype)])
            return [w[0]] + [pad(a) for a in w[1:]], None
        return Job(A, B, run, want(A), want(B), outs=outs)
    return build


def _permute_array(tup, vb):
    def build():
        idt = TUPLES[tup][1]
        n = 200000
        oa, ob = synth.random_permutation(n, 3, idt), synth.random_permutation(n, 4, idt)
        va, vbb = _vals(n, vb, 5), _vals(n, vb, 6)
        run = lambda ctx, bufs, outs: ([ctx.ops.permute_array(bufs[0], bufs[1])], None)
        orc = _oracle()
        return Job([oa, va], [ob, vbb], run, ([orc.permute_array(oa, va)], None), ([orc.permute_array(ob, vbb)], None))
    return build


def _new_row_prefix(rp, order):
    lens = np.zeros(len(rp) - 1, np.int64)
    lens[np.asarray(order, np.int64)] = np.diff(np.asarray(rp, np.int64))
    return np.concatenate([[0], np.cumsum(lens)])


def _rows_nnz(tup):
    def build():
        ra, rb = _row_ptrs()
        ot, idt = TUPLES[tup]
        n = len(ra) - 1
        oa, ob = synth.random_permutation(n, 7, idt), synth.random_permutation(n, 8, idt)
        r0, r1 = n // 4, n // 2
        run = lambda ctx, bufs, outs: ([], ctx.ops.permute_csr_rows_nnz(n, bufs[0], bufs[1], r0, r1))
        want = lambda r, o: ([], int(_new_row_prefix(r, o)[r1] - _new_row_prefix(r, o)[r0]))
        return Job([_cast(ra, ot), oa], [_cast(rb, ot), ob], run, want(ra, oa), want(rb, ob))
    return build


def _balanced_splits(tup):
    def build():
        from sparsebase_amd import sharded
        ra, rb = _row_ptrs()
        ot, idt = TUPLES[tup]
        n = len(ra) - 1
        oa, ob = synth.random_permutation(n, 9, idt), synth.random_permutation(n, 10, idt)
        run = lambda ctx, bufs, outs: ([], ctx.ops.balanced_row_splits(n, bufs[0], bufs[1], 7))
        want = lambda r, o: ([], sharded.balanced_row_ranges(torch.from_numpy(_new_row_prefix(r, o)), 7))
        return Job([_cast(ra, ot), oa], [_cast(rb, ot), ob], run, want(ra, oa), want(rb, ob))
    return build


for _i, _tup in enumerate(TUPLES):
    case(f"permute_csr-{_tup}-both-v4-sorted", "sbx_permute_csr", other_stream=True)(_permute_csr(_tup, 4, "both", False))
    case(f"permute_csr-{_tup}-rows-v0-sorted", "sbx_permute_csr")(_permute_csr(_tup, 0, "rows", False))
    case(f"permute_csr-{_tup}-cols-v8-sorted", "sbx_permute_csr")(_permute_csr(_tup, 8, "cols", False))
    case(f"permute_csr-{_tup}-both-v8-unsorted", "sbx_permute_csr")(_permute_csr(_tup, 8, "both", True))
    case(f"permute_csr-{_tup}-rows-v4-unsorted", "sbx_permute_csr")(_permute_csr(_tup, 4, "rows", True))
    case(f"permute_csr_rows-{_tup}-v{(4, 0, 8)[_i]}-shard_nnz", "sbx_permute_csr_rows")(_permute_csr_rows(_tup, (4, 0, 8)[_i]))
    case(f"permute_csr_rows-{_tup}-v{(8, 4, 0)[_i]}-null", "sbx_permute_csr_rows")(_permute_csr_rows_null(_tup, (8, 4, 0)[_i]))
    case(f"permute_csr_rows_nnz-{_tup}", "sbx_permute_csr_rows_nnz", other_stream=_i == 0)(_rows_nnz(_tup))
for _i, _tup in enumerate(COO_TUPLES):
    case(f"permute_array-{_tup}-v{4 + 4 * _i}", "sbx_permute_array")(_permute_array(_tup, 4 + 4 * _i))
    case(f"balanced_row_splits-{_tup}", "sbx_balanced_row_splits")(_balanced_splits(_tup))


# ---------------------------------------------------------------------------------------------------------- the harness
class Ctx:
    """What a case's run() gets: ops (binds its handle to torch's current stream on every call) and, for the entry points
    ops does not wrap, capi with a handle of the test's own that is set to the current stream here."""

    def __init__(self):
        from sparsebase_amd import capi, ops
        self.ops, self.capi, self.lib = ops, capi, capi.load()
        self._h = None

    @property
    def h(self):
        if self._h is None:
            self._h = C.c_void_p()
            assert self.lib.sbx_create(torch.cuda.current_device(), C.byref(self._h)) == 0
        assert self.lib.sbx_set_stream(self._h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        return self._h

    @staticmethod
    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def check(self, rc):
        assert rc == 0, self.lib.sbx_last_error(self._h).decode()

    def close(self):
        if self._h is not None:
            self.lib.sbx_sync(self._h)
            self.lib.sbx_destroy(self._h)
            self._h = None


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    c = Ctx()
    yield c
    torch.cuda.synchronize()
    c.close()


@pytest.fixture(scope="module")
def delay(ctx):
    """(cycles for DELAY_MS, cycles per millisecond, measured length in ms): torch.cuda._sleep calibrated with two
    timing events, or a chain of large kernels where torch has no _sleep."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        probe = 20_000_000
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        torch.cuda.synchronize()
        per_ms = probe / e0.elapsed_time(e1)
        amount = int(per_ms * DELAY_MS)
        fn = lambda: torch.cuda._sleep(amount)
        unit = "cycles"
    else:
        x = torch.empty(1 << 26, dtype=torch.float32, device="cuda")
        x.fill_(1.0)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(16):
            x.mul_(1.0000001)
        e1.record()
        torch.cuda.synchronize()
        per_ms = 16 / e0.elapsed_time(e1)
        amount = max(1, int(per_ms * DELAY_MS))

        def fn():
            for _ in range(amount):
                x.mul_(1.0000001)
        unit = "kernels"
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    measured = e0.elapsed_time(e1)
    print(f"\n[stream order] delay: {amount} {unit} ({per_ms:.1f} {unit} per ms), measured {measured:.2f} ms")
    return fn, per_ms, measured


@pytest.fixture(scope="module")
def streams(ctx, delay):
    """Two non-blocking streams (torch creates its streams non-blocking) for every case: the caller's and the second
    consumer's.  The runtime spreads a process's streams over a few hardware queues (four on these machines), and a
    hardware queue runs its packets in order: work that the library put on the NULL stream by mistake would sit behind
    the delay, and come out right, if the caller's stream shared the null stream's queue.  So the caller's stream is
    one that is seen NOT to hold back the null stream: a delay on the candidate, a small kernel on the null stream,
    which must finish while the delay is pending.  (Which of the handle's seven side streams share the caller's queue
    cannot be chosen; a side stage there waits behind the delay, which is what its fork event asks of it anyway.)"""
    word = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    found = []
    for _ in range(12):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            delay[0]()
            d = torch.cuda.Event()
            d.record(s)
        word.add_(1.0)  # (torch's current stream here is the null stream)
        e = torch.cuda.Event()
        e.record(torch.cuda.default_stream())
        t0 = time.perf_counter()
        while not e.query() and time.perf_counter() - t0 < 0.005:
            pass
        free = e.query() and not d.query()
        torch.cuda.synchronize()
        if free:
            found.append(s)
            if len(found) == 2:
                break
    assert len(found) == 2, "no stream found whose delay leaves the null stream running: the premise of every case"
    return found


SENTINEL = 0xFF


def _bytes_equal(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _same(got, want):
    (g_outs, g_host), (w_outs, w_host) = got, want
    return len(g_outs) == len(w_outs) and all(_bytes_equal(g, w) for g, w in zip(g_outs, w_outs)) and g_host == w_host


def _explain(got, want, early):
    """None if got == want, else what the mismatch looks like."""
    if _same(got, want):
        return None
    if _same(got, early):
        return "inputs read before the stream delivered them (the result of the decoy inputs)"
    (g_outs, g_host), (w_outs, w_host) = got, want
    notes = []
    for k, (g, w) in enumerate(zip(g_outs, w_outs)):
        if g.dtype != w.dtype or g.shape != w.shape:
            notes.append(f"output {k}: {g.dtype}{g.shape} for {w.dtype}{w.shape}")
            continue
        if g.size == 0 or _bytes_equal(g, w):
            continue
        gb = g.view(np.uint8).reshape(g.size, g.itemsize)
        wb = w.view(np.uint8).reshape(w.size, w.itemsize)
        left = np.nonzero((gb == SENTINEL).all(axis=1) & ~(wb == SENTINEL).all(axis=1))[0]
        if len(left):
            return f"output not written in stream order (output {k}: the sentinel is left at {len(left)} of {g.size} positions, first {left[:5]})"
        bad = np.nonzero((gb != wb).any(axis=1))[0]
        notes.append(f"output {k}: {len(bad)} of {g.size} differ, first at {bad[:5]}: {g[bad[:5]]} for {w[bad[:5]]}")
    if g_host != w_host:
        notes.append(f"host result {str(g_host)[:200]} for {str(w_host)[:200]}")
    return "; ".join(notes) or "outputs differ in number"


def _call(ctx, job, bufs, outs):
    dev_outs, host = job.run(ctx, bufs, outs)
    return [o for o in dev_outs if o is not None], host


OBSERVED = {}  # entry point -> {case id: returned while the delay was pending}
RESULTS = {}   # case id -> None (passed) or the failure's text


def held_back(ctx, delay_fn, streams, cid, entry, job, mode):
    dev = torch.device("cuda", torch.cuda.current_device())
    early = job.want_early or job.want_B
    assert not _same(job.want_A, early), "R(A) == R(B): the case could not tell the real inputs from the decoy"
    up = lambda xs: [None if x is None else torch.from_numpy(x).to(dev) for x in xs]
    stage_a, stage_b = up(job.A), up(job.B)
    bufs = [None if b is None else b.clone() for b in stage_b]
    outs = [torch.empty(int(numel), dtype=torch.from_numpy(np.zeros(0, dt)).dtype, device=dev) for numel, dt in job.outs]

    def load(stage):
        for b, x in zip(bufs, stage):
            if b is not None:
                b.copy_(x, non_blocking=True)

    def fill_sentinel():
        for o in outs:
            o.view(torch.uint8).fill_(SENTINEL)
    s, s2 = streams
    torch.cuda.synchronize()
    try:
        # 2. warm-up on the same stream, no delay: A, then B
        with torch.cuda.stream(s):
            shapes = None
            for name, stage, want in (("A", stage_a, job.want_A), ("B", stage_b, job.want_B)):
                load(stage)
                fill_sentinel()
                torch.cuda.synchronize()  # (the warm-up prepares, it is not the check: finished inputs, finished outputs)
                dev_outs, host = _call(ctx, job, bufs, outs)
                torch.cuda.synchronize()
                got = ([o.cpu().numpy() for o in dev_outs], host)
                if name == "A":
                    shapes = [(tuple(o.shape), o.dtype) for o in dev_outs]
                del dev_outs
                why = _explain(got, want, ([], object()))
                assert why is None, f"warm-up call on {name} (no delay) is wrong: {why}"
            load(stage_b)
            fill_sentinel()
            pinned = [torch.empty(shape, dtype=dt, pin_memory=True) for shape, dt in shapes]
            for p in pinned:
                p.view(torch.uint8).fill_(SENTINEL)
        torch.cuda.synchronize()
        # 3. the held-back call
        with torch.cuda.stream(s):
            delay_fn()
            d = torch.cuda.Event()
            d.record(s)
            load(stage_a)
            assert not d.query(), "premise: the delay had ended before the call was entered (raise DELAY_MS)"
            dev_outs, host = _call(ctx, job, bufs, outs)
            returned_early = not d.query()
            if [(tuple(o.shape), o.dtype) for o in dev_outs] != shapes:  # (a wrong result of another size)
                pinned = [torch.empty(tuple(o.shape), dtype=o.dtype, pin_memory=True) for o in dev_outs]
            if mode == "same":
                for p, o in zip(pinned, dev_outs):
                    p.copy_(o, non_blocking=True)
            else:  # a consumer on another stream orders itself behind an event recorded on the handle's stream
                ev = torch.cuda.Event()
                ev.record(s)
                s2.wait_event(ev)
                with torch.cuda.stream(s2):
                    for p, o in zip(pinned, dev_outs):
                        p.copy_(o, non_blocking=True)
            if not job.inplace:
                load(stage_b)
        s.synchronize()
        s2.synchronize()
    finally:
        torch.cuda.synchronize()
    OBSERVED.setdefault(entry, {})[f"{cid}/{mode}"] = returned_early
    return _explain(([p.numpy() for p in pinned], host), job.want_A, early)


def _report(cid, mode, entry, text):
    RESULTS[f"{cid}/{mode}"] = text
    path = os.environ.get("SBX_STREAM_ORDER_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": f"{cid}/{mode}", "entry": entry, "failure": text,
                                "returned_early": OBSERVED.get(entry, {}).get(f"{cid}/{mode}")}) + "\n")


PARAMS = [pytest.param(cid, entry, build, mode, id=f"{cid}/{mode}") for cid, entry, build, modes in CASES for mode in modes]


@pytest.mark.parametrize("cid,entry,build,mode", PARAMS)
def test_case(ctx, delay, streams, cid, entry, build, mode):
    try:
        why = held_back(ctx, delay[0], streams, cid, entry, build(), mode)
    except BaseException as e:
        _report(cid, mode, entry, f"{type(e).__name__}: {e}")
        raise
    _report(cid, mode, entry, why)
    assert why is None, f"{entry} on a held-back stream: {why}"


def test_synchronous_table():
    """Entry point by entry point: returned while the delay was pending, or waited — against SYNCHRONOUS, the table of
    INTEGRATION.md.  A function documented "Synchronous" in include/sbx.h must have waited."""
    if not OBSERVED:  # (run on its own: the table is made of what the cases of this session observed)
        return
    print("\n[stream order] entry point: waited for the stream / returned with its work enqueued")
    wrong = []
    for entry in sorted(OBSERVED):
        seen = OBSERVED[entry]
        kinds = sorted(set(seen.values()))
        print(f"  {entry:32s} {'returned early' if kinds == [True] else 'waited' if kinds == [False] else 'BOTH: ' + str(seen)}")
        for key, early in seen.items():
            want = SYNCHRONOUS[entry]
            if isinstance(want, dict):
                want = want[max((k for k in want if k in key), key=len)]
            if early != (not want):
                wrong.append((key, "returned early" if early else "waited"))
    assert not wrong, f"not as SYNCHRONOUS (and INTEGRATION.md) say: {wrong}"
    if len(RESULTS) == len(PARAMS):
        assert sorted(OBSERVED) == sorted(SYNCHRONOUS)


# ------------------------------------------------------------------------------------------- the same cases in children
def _child(select, env=None, variant=""):
    """This module's cases in a fresh process (tools/pytest_with_lib.py: pytest against the product or a variant
    library); returns {case: failure text or None}."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        report = os.path.join(tmp, "report.jsonl")
        e = dict(os.environ, SBX_STREAM_ORDER_REPORT=report, **(env or {}))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pytest_with_lib.py"), variant, os.path.abspath(__file__),
                            "-q", "-p", "no:cacheprovider", "-k", f"test_case and ({select})"],
                           cwd=ROOT, env=e, capture_output=True, text=True, timeout=1500)
        lines = [json.loads(l) for l in open(report)] if os.path.exists(report) else []
    return {l["case"]: l["failure"] for l in lines}, r


def test_permutes_without_side_streams_in_a_child():
    """SBX_PERMUTE_OVERLAP=0: tile, block-row and long-row paths and the key-distribution map back to back on the caller's
    stream — a failure of a permute case that stays here is the main stream's, one that goes away a side stream's."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    res, r = _child("permute_csr or csr_sort_rows or coo_sort", {"SBX_PERMUTE_OVERLAP": "0"})
    want = [f"{cid}/{mode}" for cid, entry, _, modes in CASES for mode in modes
            if entry in ("sbx_permute_csr", "sbx_permute_csr_rows", "sbx_permute_csr_rows_nnz", "sbx_csr_sort_rows", "sbx_coo_sort")]
    assert r.returncode == 0 and sorted(res) == sorted(want) and not any(res.values()), (res, r.stdout[-3000:], r.stderr[-2000:])


def test_rcm_without_side_streams_in_a_child():
    """SBX_RCM_OVERLAP=0 SBX_RCM_CC_OVERLAP=0 SBX_RCM_SPLIT_EXPAND=0: degree ranks, component labelling and the light rows
    of wide frontiers on the caller's stream."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    res, r = _child("rcm_reorder", {"SBX_RCM_OVERLAP": "0", "SBX_RCM_CC_OVERLAP": "0", "SBX_RCM_SPLIT_EXPAND": "0"})
    want = [f"{cid}/{mode}" for cid, entry, _, modes in CASES for mode in modes if entry == "sbx_rcm_reorder"]
    assert r.returncode == 0 and sorted(res) == sorted(want) and not any(res.values()), (res, r.stdout[-3000:], r.stderr[-2000:])


def test_the_harness_reports_a_launch_on_the_wrong_stream():
    """libsbx_stream0.so (sparsebase_amd/build.py, VARIANTS: -DSBX_DEBUG_DEGREES_STREAM0=1) launches the kernel of
    sbx_csr_degrees on the null stream instead of the handle's.  On a non-blocking caller stream that launch waits for
    nothing: every sbx_csr_degrees case must fail, as an early read of the inputs or as an output that is not written in
    stream order, and every other case must still pass."""
    from sparsebase_amd import build as hip_build
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    assert os.path.exists(hip_build.variant_path("stream0")), "libsbx_stream0.so is not built (__graft_entry__.build() builds it)"
    res, r = _child("not rmat18 and not jaccard", variant="stream0")  # (the two slowest CPU references are not needed twice)
    assert len(res) >= 100, (len(res), r.stdout[-3000:], r.stderr[-2000:])
    broken = {c: t for c, t in res.items() if c.startswith("csr_degrees-")}
    print("\n[stream order] the wrong-stream build:", broken)
    assert len(broken) == 4, broken
    for c, t in broken.items():
        assert t and ("inputs read before the stream delivered them" in t or "output not written in stream order" in t), (c, t)
    others = {c: t for c, t in res.items() if not c.startswith("csr_degrees-") and t}
    assert not others, others
