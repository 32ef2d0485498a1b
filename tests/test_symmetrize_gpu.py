"""sbsym_csr_missing_mirrors and sbsym_csr_symmetrize (include/sbsym.h) on the GPU, bit for bit against the Python
restatement tests/symmetrize_restate.py, for the three index tuples x values none, 4-byte and 8-byte.

Shapes: n = 0; n = 1 with and without its diagonal; a symmetric matrix (the copy, and the outputs left alone under
SBSYM_SKIP_IF_SYMMETRIC); a strict upper triangle; a random n = 3 000 matrix with about 8 entries per row, duplicates
and diagonals; duplicate columns whose mirror is missing; one stored ROW of 5 000 entries without mirrors in n = 6 000
and its transpose, where one row RECEIVES 5 000 entries (every kernel is a grid-stride loop of workgroups of 256 threads
with one entry per thread and step, 1 024 in the streaming comparison: the hubs are longer than twice that); an input
with more entries than the widest grid has threads, so every loop takes a second step.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symmetrize_restate as sr  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (offsets, ids): SBX_I32, SBX_I64, SBX_I32_N64
TUPLES = {"i32": (np.int32, np.int32), "i64": (np.int64, np.int64), "i32_n64": (np.int64, np.int32)}
VALUES = {"v0": None, "v4": np.float32, "v8": np.float64}
SENTINEL = 0x5A
NO_DIAGONAL, SKIP = 1, 2
HUB = 5000


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import ops
    return ops


def _csr(n, rows, cols):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    o = np.lexsort((cols, rows))
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64), cols[o]


@functools.lru_cache(None)
def _shapes():
    g = np.random.default_rng(7)
    out = {"n0": (0, np.zeros(1, np.int64), np.zeros(0, np.int64)),
           "n1": (1, np.array([0, 0]), np.zeros(0, np.int64)),
           "n1-diagonal": (1, np.array([0, 1]), np.zeros(1, np.int64)),
           "no-entries": (5, np.zeros(6, np.int64), np.zeros(0, np.int64))}
    from sparsebase_amd import synth
    rp, col = synth.random_symmetric_graph(700, avg_deg=5.0, seed=3, idx_dtype=np.int64)
    out["symmetric"] = (700, rp, col)
    r, c = np.triu_indices(90, 1)
    keep = g.random(len(r)) < 0.3
    out["upper"] = (90,) + _csr(90, r[keep], c[keep])
    n = 3000
    r, c = g.integers(0, n, 8 * n), g.integers(0, n, 8 * n)
    dup = g.random(8 * n) < 0.05
    d = g.integers(0, n, n // 3)
    out["random"] = (n,) + _csr(n, np.concatenate([r, r[dup], d, d[:50]]), np.concatenate([c, c[dup], d, d[:50]]))
    # rows with duplicate columns whose mirror is missing, next to ones whose mirror is stored once or twice
    out["duplicates"] = (6,) + _csr(6, [0, 0, 0, 1, 1, 2, 2, 4, 4, 4, 5], [2, 2, 2, 4, 4, 1, 1, 1, 5, 5, 4])
    n = 6000
    hub_cols = np.sort(g.choice(np.arange(1, n), HUB, replace=False))
    out["hub-row"] = (n,) + _csr(n, np.concatenate([np.zeros(HUB, np.int64), [7, 7, 9]]), np.concatenate([hub_cols, [7, 8, 9]]))
    out["hub-column"] = (n,) + _csr(n, np.concatenate([hub_cols, [7, 7, 9]]), np.concatenate([np.zeros(HUB, np.int64), [7, 8, 9]]))
    return out


@functools.lru_cache(None)
def _want(shape, no_diagonal):
    """(row_ptr_out, col_out, source position of every entry, added): computed once per shape, shared."""
    n, rp, col = _shapes()[shape]
    rpo, co, src, added = sr.symmetrize(n, rp, col, np.arange(len(col), dtype=np.int64), no_diagonal)
    for a in (rpo, co, src):
        a.setflags(write=False)
    return rpo, co, src, added


def _vals(count, vdt):
    return None if vdt is None else (np.random.default_rng(11).permutation(count) - count // 2).astype(vdt)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tdt(dt):
    return torch.from_numpy(np.zeros(0, dt)).dtype


def _call(ops, ot, idt, n, rp, col, val, flags=0, capacity=None, count_only=False, spare_row_ptr_word=False, handle=None):
    """One sbsym_csr_symmetrize call into sentinel-filled outputs: (status, message, row_ptr_out, col_out, val_out,
    nnz_out, added), the arrays whole, as numpy."""
    hd = handle or ops.handle_for(torch.device("cuda", torch.cuda.current_device()))
    rp_host = np.concatenate([rp, [rp[-1]]]) if spare_row_ptr_word else rp
    d_rp, d_col, d_val = _dev(rp_host.astype(ot)), _dev(col.astype(idt)), _dev(val)
    cap = max(1, 2 * len(col)) if capacity is None else capacity
    fill = lambda count, dt: torch.full((max(1, count) * np.dtype(dt).itemsize,), SENTINEL, dtype=torch.uint8,
                                        device="cuda").view(_tdt(dt))[:count]
    rpo = fill(n + 1, ot)
    co = None if count_only else fill(cap, idt)
    vo = None if (count_only or val is None) else fill(cap, val.dtype)
    k, added = C.c_int64(-1), C.c_int64(-1)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    vt = ops._vt(d_val)
    rc = hd.lib.sbsym_csr_symmetrize(hd.h, ops._it(d_rp, d_col), vt, n, len(col), p(d_rp), p(d_col), p(d_val), flags, cap,
                                     p(rpo), p(co), p(vo), C.byref(k), C.byref(added))
    msg = hd.lib.sbx_last_error(hd.h).decode() if rc else ""
    torch.cuda.synchronize()
    np_ = lambda t: None if t is None else t.cpu().numpy()
    return rc, msg, np_(rpo), np_(co), np_(vo), k.value, added.value


def _untouched(a):
    return a is None or bool((a.view(np.uint8) == SENTINEL).all())


def _check(ops, shape, tup, vkey, no_diagonal):
    n, rp, col = _shapes()[shape]
    ot, idt = TUPLES[tup]
    val = _vals(len(col), VALUES[vkey])
    w_rp, w_col, w_src, w_added = _want(shape, no_diagonal)
    rc, msg, rpo, co, vo, k, added = _call(ops, ot, idt, n, rp, col, val, NO_DIAGONAL if no_diagonal else 0)
    assert rc == 0, msg
    assert (k, added) == (len(w_col), w_added)
    assert rpo.tobytes() == w_rp.astype(ot).tobytes()
    assert co[:k].tobytes() == w_col.astype(idt).tobytes() and _untouched(co[k:])
    if val is not None:
        assert vo[:k].tobytes() == val[w_src].tobytes() and _untouched(vo[k:])
    assert ops.csr_missing_mirrors(_dev(rp.astype(ot)), _dev(col.astype(idt))) == w_added
    return rpo, co[:k], (None if vo is None else vo[:k]), added


SHAPES = ("n0", "n1", "n1-diagonal", "no-entries", "symmetric", "upper", "random", "duplicates", "hub-row", "hub-column")


@pytest.mark.parametrize("vkey", list(VALUES))
@pytest.mark.parametrize("tup", list(TUPLES))
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_restatement(ops, shape, tup, vkey):
    for no_diagonal in (False, True):
        _check(ops, shape, tup, vkey, no_diagonal)


def test_the_shapes_are_what_they_claim(ops):
    S = _shapes()
    assert _want("symmetric", False)[3] == 0
    n, rp, col = S["upper"]
    assert _want("upper", False)[3] == len(col) and len(_want("upper", False)[1]) == 2 * len(col)
    assert _want("hub-row", False)[3] == HUB + 1 and _want("hub-column", False)[3] == HUB + 1
    assert HUB > 2 * 1024
    n, rp, col = S["hub-column"]
    assert np.diff(_want("hub-column", False)[0]).max() == HUB and np.diff(rp).max() <= 3  # (no stored row is long)
    rows = np.repeat(np.arange(S["random"][0]), np.diff(S["random"][1]))
    assert (rows == S["random"][2]).sum() > 100 and _want("random", False)[3] > 20000


@pytest.mark.parametrize("tup", list(TUPLES))
def test_symmetric_input_copy_and_skip(ops, tup):
    n, rp, col = _shapes()["symmetric"]
    ot, idt = TUPLES[tup]
    val = _vals(len(col), np.float32)
    rc, msg, rpo, co, vo, k, added = _call(ops, ot, idt, n, rp, col, val)
    assert rc == 0 and (k, added) == (len(col), 0)
    assert rpo.tobytes() == rp.astype(ot).tobytes() and co[:k].tobytes() == col.astype(idt).tobytes()
    assert vo[:k].tobytes() == val.tobytes()
    rc, msg, rpo, co, vo, k, added = _call(ops, ot, idt, n, rp, col, val, SKIP)
    assert rc == 0 and (k, added) == (len(col), 0)
    assert _untouched(rpo) and _untouched(co) and _untouched(vo), "SBSYM_SKIP_IF_SYMMETRIC wrote an output"
    # the flag skips nothing where something is missing, or where a diagonal is dropped
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert (rows == col).any()
    rc, msg, rpo, co, vo, k, added = _call(ops, ot, idt, n, rp, col, val, SKIP | NO_DIAGONAL)
    w = _want("symmetric", True)
    assert rc == 0 and added == 0 and k == len(w[1]) < len(col)
    assert rpo.tobytes() == w[0].astype(ot).tobytes() and co[:k].tobytes() == w[1].astype(idt).tobytes()
    assert vo[:k].tobytes() == val[w[2]].tobytes()
    n, rp, col = _shapes()["upper"]
    rc, msg, rpo, co, vo, k, added = _call(ops, ot, idt, n, rp, col, None, SKIP)
    assert rc == 0 and added == len(col) and co[:k].tobytes() == _want("upper", False)[1].astype(idt).tobytes()


def test_duplicates_add_one_entry_with_the_first_value(ops):
    rp, col = np.array([0, 3, 3, 3]), np.array([2, 2, 2])
    val = np.array([10.0, 20.0, 30.0], np.float32)
    rc, msg, rpo, co, vo, k, added = _call(ops, np.int32, np.int32, 3, rp, col, val)
    assert rc == 0 and (k, added) == (4, 1)
    assert rpo.tolist() == [0, 3, 3, 4] and co[:4].tolist() == [2, 2, 2, 0] and vo[:4].tolist() == [10, 20, 30, 10]


def test_ops_wrappers(ops):
    n, rp, col = _shapes()["random"]
    val = _vals(len(col), np.float64)
    for nd in (False, True):
        w_rp, w_col, w_src, w_added = _want("random", nd)
        rpo, co, vo, added = ops.csr_symmetrize(_dev(rp.astype(np.int32)), _dev(col.astype(np.int32)), _dev(val), no_diagonal=nd)
        assert added == w_added and rpo.cpu().numpy().tobytes() == w_rp.astype(np.int32).tobytes()
        assert co.cpu().numpy().tobytes() == w_col.astype(np.int32).tobytes()
        assert vo.cpu().numpy().tobytes() == val[w_src].tobytes()
    rpo, co, vo, added = ops.csr_symmetrize(_dev(rp), _dev(col))
    assert vo is None and co.cpu().numpy().tobytes() == _want("random", False)[1].tobytes()


@pytest.mark.parametrize("tup", list(TUPLES))
def test_count_only_and_capacity(ops, tup):
    ot, idt = TUPLES[tup]
    for shape, nd in (("random", False), ("random", True), ("hub-column", False)):
        n, rp, col = _shapes()[shape]
        w_rp, w_col, w_src, w_added = _want(shape, nd)
        flags = NO_DIAGONAL if nd else 0
        rc, msg, rpo, co, vo, k, added = _call(ops, ot, idt, n, rp, col, None, flags, count_only=True)
        assert rc == 0 and (k, added) == (len(w_col), w_added) and rpo.tobytes() == w_rp.astype(ot).tobytes()
        val = _vals(len(col), np.float32)
        rc, msg, rpo, co, vo, k, added = _call(ops, ot, idt, n, rp, col, val, flags, capacity=len(w_col) - 1)
        assert rc == 1 and (k, added) == (len(w_col), w_added), (rc, msg)
        assert str(len(w_col)) in msg, msg
        assert _untouched(rpo) and _untouched(co) and _untouched(vo)
        rc, msg, rpo, co, vo, k, added = _call(ops, ot, idt, n, rp, col, val, flags, capacity=len(w_col))
        assert rc == 0 and co.tobytes() == w_col.astype(idt).tobytes() and vo.tobytes() == val[w_src].tobytes()


@pytest.mark.parametrize("tup", list(TUPLES))
def test_refusals(ops, tup):
    ot, idt = TUPLES[tup]
    from sparsebase_amd import capi
    n, rp, col = _shapes()["random"]
    # a row whose columns decrease
    bad = col.copy()
    i = int(np.nonzero(np.diff(rp) >= 2)[0][5])
    a, b = rp[i], rp[i + 1] - 1
    assert bad[a] != bad[b]
    bad[a], bad[b] = bad[b], bad[a]
    rc, msg, rpo, co, vo, k, added = _call(ops, ot, idt, n, rp, bad, None)
    assert rc == 1 and "decrease" in msg and _untouched(rpo) and _untouched(co)
    with pytest.raises(capi.SbxError, match="decrease"):
        ops.csr_missing_mirrors(_dev(rp.astype(ot)), _dev(bad.astype(idt)))
    # column id n (and -1): refused, never used as a row (row_ptr carries one spare trailing word)
    for where, value in ((len(col) - 1, n), (0, -1), (len(col) // 2, n)):
        bad = col.copy()
        bad[where] = value
        rc, msg, rpo, co, vo, k, added = _call(ops, ot, idt, n, rp, bad, None, spare_row_ptr_word=True)
        assert rc == 1 and "outside" in msg and _untouched(rpo) and _untouched(co), (where, value, rc, msg)
    d_rp = _dev(np.concatenate([rp, [rp[-1]]]).astype(ot))
    with pytest.raises(capi.SbxError, match="outside"):
        ops.csr_missing_mirrors(d_rp[:n + 1], _dev(bad.astype(idt)))
    # the handle works on
    _check(ops, "duplicates", tup, "v4", False)


def test_argument_refusals(ops):
    n, rp, col = _shapes()["duplicates"]
    rc, msg, *_ = _call(ops, np.int32, np.int32, n, rp, col, None, flags=4)
    assert rc == 1 and "flag" in msg
    hd = ops.handle_for(torch.device("cuda", torch.cuda.current_device()))
    out = C.c_int64(0)
    d_rp, d_col = _dev(rp.astype(np.int32)), _dev(col.astype(np.int32))
    p = lambda t: C.c_void_p(t.data_ptr())
    assert hd.lib.sbsym_csr_missing_mirrors(hd.h, 0, n, len(col), p(d_rp), None, C.byref(out)) == 1
    assert hd.lib.sbsym_csr_missing_mirrors(hd.h, 7, n, len(col), p(d_rp), p(d_col), C.byref(out)) == 1
    assert hd.lib.sbsym_csr_missing_mirrors(hd.h, 1, (1 << 31) - 1, 1, p(d_rp), p(d_col), C.byref(out)) == 5
    assert "2^31" in hd.lib.sbx_last_error(hd.h).decode()
    assert hd.lib.sbsym_csr_missing_mirrors(hd.h, 1, 10, 1 << 31, p(d_rp), p(d_col), C.byref(out)) == 5
    assert str(1 << 31) in hd.lib.sbx_last_error(hd.h).decode()


def test_same_bits_from_two_calls_and_two_handles(ops):
    n, rp, col = _shapes()["random"]
    val = _vals(len(col), np.float32)
    first = _call(ops, np.int32, np.int32, n, rp, col, val)
    again = _call(ops, np.int32, np.int32, n, rp, col, val)
    other = ops.Handle(torch.cuda.current_device())
    other.bind_stream()
    third = _call(ops, np.int32, np.int32, n, rp, col, val, handle=other)
    torch.cuda.synchronize()
    other.check(other.lib.sbx_destroy(other.h))
    for got in (again, third):
        assert got[0] == 0 and got[5:] == first[5:]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[2:5], first[2:5]))


def test_more_entries_than_the_widest_grid_has_threads(ops):
    """Every nonzero-parallel kernel caps its grid at 32 workgroups of 256 threads per compute unit: with more entries
    than that every grid-stride loop takes a second step (checked on the device's own count of compute units)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 1 << 17
    per_row = (cus * 32 * 256) // n + 2
    g = np.random.default_rng(5)
    rows = np.repeat(np.arange(n, dtype=np.int64), per_row)
    step = np.tile(1 + 2 * np.arange(per_row, dtype=np.int64), n) + g.integers(0, 2, len(rows))  # distinct inside a row
    cols = (rows + step) % n  # a band: cheap to state with numpy
    key = np.unique(rows * n + cols)
    rows, cols = key // n, key % n
    assert len(rows) > cus * 32 * 256
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    rpo, co, _, added = ops.csr_symmetrize(_dev(rp.astype(np.int32)), _dev(cols.astype(np.int32)))
    both = np.unique(np.concatenate([key, cols * n + rows]))
    assert added == len(both) - len(key)
    assert np.array_equal(co.cpu().numpy(), (both % n).astype(np.int32))
    assert np.array_equal(rpo.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(both // n, minlength=n))]).astype(np.int32))
