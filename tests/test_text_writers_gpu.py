"""GPU tests of the text-output ABI (include/sbx_text.h) against the Python restatement of its rules
(tests/text_restate.py), the literal transcription of the reference's writers and the bytes recorded from the real
reference (tests/golden/text_writers.npz)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_restate as tr  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = (1, 6, 9, 17)
# name -> (numpy dtype of the values, dtype the tensor is handed over as, unsigned)
VTYPES = {"none": (None, None, False), "i32": (np.int32, np.int32, False), "u32": (np.uint32, np.int32, True),
          "f32": (np.float32, np.float32, False), "i64": (np.int64, np.int64, False), "u64": (np.uint64, np.int64, True),
          "f64": (np.float64, np.float64, False)}
ITYPES = {"i32": np.int32, "i64": np.int64}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import ops
    return ops


def dev(a, as_dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if as_dtype is not None and a.dtype != as_dtype:
        a = a.view(as_dtype)
    return torch.from_numpy(a.copy()).cuda()


def text_of(t):
    return t.cpu().numpy().tobytes()


def values(vname, count, seed):
    """Values of every kind the type has: extremes, zeros, for the floating types random bit patterns (subnormals, inf
    and NaN of both signs), short decimals, ties, and magnitudes a matrix has."""
    dt = VTYPES[vname][0]
    if dt is None:
        return None
    g = np.random.default_rng(seed)
    if np.issubdtype(dt, np.integer):
        info = np.iinfo(dt)
        v = g.integers(info.min, info.max, count, dtype=dt, endpoint=True)
        small = g.integers(max(info.min, -1000), 1000, count).astype(dt)
        v = np.where(g.random(count) < 0.5, v, small)
        v[:4] = np.array([info.min, info.max, 0, 1], dt)[:len(v[:4])]
        return v
    bits = np.uint32 if dt == np.float32 else np.uint64
    raw = g.integers(0, np.iinfo(bits).max, count, dtype=bits, endpoint=True).view(dt)
    short = (g.integers(-2000000, 2000000, count) / 10.0 ** g.integers(0, 9, count)).astype(dt)
    ties = (g.integers(1, 10 ** 6, count) + g.choice([0.5, 0.25, 0.125, 0.375], count)).astype(dt)
    wide = (g.random(count) * 10.0 ** g.integers(-12, 12, count)).astype(dt)
    pick = g.integers(0, 4, count)
    v = np.where(pick == 0, raw, np.where(pick == 1, short, np.where(pick == 2, ties, wide))).astype(dt)
    fixed = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 0.5, 2.5, 1000005.0, 999999.5, np.finfo(dt).max, np.finfo(dt).tiny,
             np.finfo(dt).smallest_subnormal, 1e-5, 1e-4, 123456.5, 1e16, 1e17]
    v[:len(fixed)] = np.array(fixed, dt)[:len(v[:len(fixed)])]
    return v


def coo(iname, n, m, nnz, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, n, nnz).astype(ITYPES[iname]), g.integers(0, m, nnz).astype(ITYPES[iname])


# ------------------------------------------------------------------------------------------------------ the formatters
@pytest.mark.parametrize("vname", [v for v in VTYPES if v != "none"])
def test_format_values(ops, vname):
    _, as_dt, unsigned = VTYPES[vname]
    v = values(vname, 20000, 1)
    for p in PRECISIONS:
        got = text_of(ops.text_format_values(dev(v, as_dt), precision=p, unsigned=unsigned))
        assert got == tr.format_values(v, p), (vname, p)


@pytest.mark.parametrize("vname", list(VTYPES))
@pytest.mark.parametrize("iname", list(ITYPES))
def test_format_coordinate(ops, iname, vname):
    _, as_dt, unsigned = VTYPES[vname]
    row, col = coo(iname, 40, 50, 3000, 2)
    if iname == "i64":  # ids beyond 32 bits
        row[:50] += 1 << 40
        col[25:75] += 1 << 50
    v = values(vname, len(row), 3)
    dr, dc, dv = dev(row), dev(col), dev(v, as_dt)
    for p, flags, base in itertools.product(PRECISIONS, range(8), (0, 1)):
        got = text_of(ops.text_format_coordinate(dr, dc, dv, index_base=base, precision=p, lower=bool(flags & 1),
                                                 no_diagonal=bool(flags & 2), pattern=bool(flags & 4), unsigned=unsigned))
        assert got == tr.format_coordinate(row, col, v, base, p, flags), (iname, vname, p, flags, base)


def _raw(ops, t):
    from sparsebase_amd import capi
    hd = ops.handle_for(t.device)
    return hd, capi


def test_protocol_sizing_capacity_and_sentinels(ops):
    row, col = coo("i32", 300, 300, 5000, 4)
    v = values("f64", len(row), 5)
    want = tr.format_coordinate(row, col, v, 1, 17, 0)
    dr, dc, dv = dev(row), dev(col), dev(v)
    hd, capi = _raw(ops, dr)
    call = lambda out, cap, nb: hd.lib.sbx_text_format_coordinate(hd.h, capi.SBX_I32, capi.V_F64, len(row), dr.data_ptr(),
                                                                  dc.data_ptr(), dv.data_ptr(), 1, 17, 0, out, cap, C.byref(nb))
    nb = C.c_int64(-1)
    assert call(None, 0, nb) == 0 and nb.value == len(want)  # the sizing call
    for shift in (0, 1, 7, 15):  # (every alignment of the output against the 16-byte words it is stored in)
        buf = torch.full((len(want) + 96,), 0xA5, dtype=torch.uint8, device="cuda")
        # one byte short: refused, nothing written
        nb = C.c_int64(-1)
        assert call(C.c_void_p(buf.data_ptr() + 16 + shift), len(want) - 1, nb) == 1 and nb.value == len(want)
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all())
        assert call(C.c_void_p(buf.data_ptr() + 16 + shift), len(want), nb) == 0 and nb.value == len(want)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert got[16 + shift:16 + shift + len(want)].tobytes() == want
        assert (got[:16 + shift] == 0xA5).all() and (got[16 + shift + len(want):] == 0xA5).all()
    # precision outside 1..17, an unknown flag
    for bad_p in (0, 18, -1):
        assert hd.lib.sbx_text_format_coordinate(hd.h, capi.SBX_I32, capi.V_F64, len(row), dr.data_ptr(), dc.data_ptr(),
                                                 dv.data_ptr(), 1, bad_p, 0, None, 0, C.byref(nb)) == 1
        assert hd.lib.sbx_text_format_values(hd.h, capi.V_F64, len(row), dv.data_ptr(), bad_p, None, 0, C.byref(nb)) == 1
        assert hd.lib.sbx_text_format_dense(hd.h, capi.SBX_I32, capi.V_F64, 300, 300, 0, None, None, None, bad_p, None, 0,
                                            C.byref(nb)) == 1
    assert hd.lib.sbx_text_format_coordinate(hd.h, capi.SBX_I32, capi.V_F64, len(row), dr.data_ptr(), dc.data_ptr(),
                                             dv.data_ptr(), 1, 6, 8, None, 0, C.byref(nb)) == 1


def test_no_entries(ops):
    e32, ef = torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.float32, device="cuda")
    assert ops.text_format_coordinate(e32, e32, ef).numel() == 0
    assert ops.text_format_values(ef).numel() == 0
    assert ops.coo_symmetry_check(5, e32, e32, ef) == (True, 0, 0)
    r, c, v = ops.coo_undirected_unique_(e32.clone(), e32.clone(), ef.clone())
    assert r.numel() == 0 and c.numel() == 0 and v.numel() == 0
    assert text_of(ops.text_format_dense(2, 3, e32, e32, ef)) == b"0\n" * 6
    assert ops.text_format_dense(0, 3, e32, e32, ef).numel() == 0
    # entries, but none kept
    one = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    two = torch.tensor([3, 4], dtype=torch.int32, device="cuda")
    assert ops.text_format_coordinate(one, two, lower=True).numel() == 0


@pytest.mark.parametrize("vname", ["none", "f32", "i64"])
def test_sub_ranges_concatenate_to_the_whole(ops, vname):
    _, as_dt, unsigned = VTYPES[vname]
    row, col = coo("i32", 1000, 1000, 7001, 6)
    v = values(vname, len(row), 7)
    dr, dc, dv = dev(row), dev(col), dev(v, as_dt)
    whole = text_of(ops.text_format_coordinate(dr, dc, dv, lower=True, precision=9, unsigned=unsigned))
    assert whole == tr.format_coordinate(row, col, v, 1, 9, tr.LOWER)
    for chunk in (1, 7, 256, 1000, 7001):
        parts = [text_of(ops.text_format_coordinate(dr[a:a + chunk], dc[a:a + chunk], None if dv is None else dv[a:a + chunk],
                                                    lower=True, precision=9, unsigned=unsigned))
                 for a in range(0, len(row), chunk)]
        assert b"".join(parts) == whole, chunk


# ------------------------------------------------------------------------------------------------------ symmetry check
def _symmetric_case(g, n, pairs, vname, skew):
    """A matrix that IS (skew-)symmetric: mirrored pairs, a few duplicated, a diagonal."""
    dt = VTYPES[vname][0]
    i, j = g.integers(0, n, pairs), g.integers(0, n, pairs)
    off = i != j
    i, j = i[off], j[off]
    if dt is None:
        w = None
    elif np.issubdtype(dt, np.integer):
        w = g.integers(-50, 50, len(i)).astype(dt)
    else:
        w = (g.integers(-50, 50, len(i)) / 4.0).astype(dt)
    row, col = np.concatenate([i, j]), np.concatenate([j, i])
    val = None if w is None else np.concatenate([w, (np.zeros_like(w) - w) if skew else w])  # (integers wrap)
    d = g.integers(0, n, 10)
    row, col = np.concatenate([row, d]), np.concatenate([col, d])
    if val is not None:
        val = np.concatenate([val, np.zeros(10, dt) if skew else g.integers(0, 3, 10).astype(dt)])
    return row, col, val


def _literal(n, row, col, val, skew):
    """The reference's double loop (tests/text_restate.py: ref_mtx_write_coo): (all matched, the message)."""
    _, msg = tr.ref_mtx_write_coo(n, n, row, col, val, void_type=val is None, field="pattern" if val is None else "real",
                                  symmetry="skew-symmetric" if skew else "symmetric")
    return msg != "Matrix is not symmetric!", msg


@pytest.mark.parametrize("vname", ["none", "i32", "u32", "f32", "i64", "f64"])
@pytest.mark.parametrize("iname", list(ITYPES))
def test_symmetry_check_against_the_literal_loop(ops, iname, vname):
    dt, as_dt, unsigned = VTYPES[vname]
    g = np.random.default_rng(11)
    n = 60
    seen = set()
    for trial in range(40):
        skew = bool(trial & 8)
        row, col, val = _symmetric_case(g, n, 150, vname, skew)
        kind = trial % 8
        if kind == 2 and val is not None:      # a mirror with another value
            k = int(g.integers(0, len(row) - 10))
            val[k:k + 1] += dt(3)
        elif kind == 3:                        # a missing mirror
            keep = np.ones(len(row), bool)
            keep[int(g.integers(0, len(row) - 10))] = False
            row, col, val = row[keep], col[keep], None if val is None else val[keep]
        elif kind == 4 and val is not None and np.issubdtype(dt, np.floating):  # -0 against +0, NaN
            val[0], val[(len(val) - 10) // 2] = dt(0.0), dt(-0.0)  # (an entry and its mirror)
            if trial & 16:
                val[1] = dt(np.nan)
        elif kind == 5 and val is not None:    # duplicates with another value next to the matching ones, both ways
            w7 = (val[:3] + dt(7)).astype(dt)
            row, col = np.concatenate([row, row[:3], col[:3]]), np.concatenate([col, col[:3], row[:3]])
            val = np.concatenate([val, w7, (np.zeros_like(w7) - w7) if skew else w7])
        elif kind == 6 and val is not None:    # a non-zero diagonal
            val[-1] = dt(5)
        if kind != 7:                          # (kind 7: the entries stay in input order; the others are shuffled or sorted)
            o = g.permutation(len(row)) if trial % 3 else np.lexsort((col, row))
            row, col, val = row[o], col[o], None if val is None else val[o]
        row, col = row.astype(ITYPES[iname]), col.astype(ITYPES[iname])
        got = ops.coo_symmetry_check(n, dev(row), dev(col), dev(val, as_dt), skew=skew, unsigned=unsigned)
        want = tr.symmetry_check(n, row, col, val, skew)
        assert got == want, (trial, got, want)
        matched, msg = _literal(n, row, col, val, skew)
        assert got[0] == matched, (trial, msg)
        if matched and skew:
            assert (got[2] > 0) == (msg == "Skew-symmetric matrix with non-zero diagonal values!")
        seen.add((got[0], skew))
    assert len(seen) == (3 if vname == "none" else 4)  # matched and unmatched, plain and skew (a pattern is never skew)
    # an id outside [0, n): refused
    row[0] = n
    with pytest.raises(Exception, match="outside"):
        ops.coo_symmetry_check(n, dev(row), dev(col))


def test_symmetry_check_leaves_the_arrays_alone(ops):
    g = np.random.default_rng(12)
    row, col, val = _symmetric_case(g, 500, 4000, "f32", False)
    o = g.permutation(len(row))
    row, col, val = row[o].astype(np.int32), col[o].astype(np.int32), val[o]
    dr, dc, dv = dev(row), dev(col), dev(val)
    assert ops.coo_symmetry_check(500, dr, dc, dv)[0]
    assert np.array_equal(dr.cpu().numpy(), row) and np.array_equal(dc.cpu().numpy(), col)
    assert dv.cpu().numpy().tobytes() == val.tobytes()


# --------------------------------------------------------------------------------------------------- undirected unique
@pytest.mark.parametrize("vname", ["none", "f32", "i64", "f64"])
@pytest.mark.parametrize("iname", list(ITYPES))
def test_undirected_unique(ops, iname, vname):
    _, as_dt, _ = VTYPES[vname]
    for n, nnz, seed in ((30, 2000, 1), (5000, 20000, 2), (3, 1, 3)):
        row, col = coo(iname, n, n, nnz, seed)
        if iname == "i64" and n == 5000:
            row[::7] += 1 << 31  # (beyond 32 bits; row and column bits together fit sbx_coo_sort's 64-bit key)
        val = values(vname, nnz, seed + 10)
        if val is not None and val.dtype.kind == "f":
            val = np.arange(nnz).astype(val.dtype)  # (distinct: which duplicate survives shows)
        r, c, v = ops.coo_undirected_unique_(dev(row), dev(col), dev(val, as_dt))
        wr, wc, wv = tr.undirected_unique(row, col, val)
        assert np.array_equal(r.cpu().numpy(), wr) and np.array_equal(c.cpu().numpy(), wc)
        if val is not None:
            assert v.cpu().numpy().tobytes() == wv.tobytes()
    bad = dev(np.array([1, -2, 3], ITYPES[iname]))
    with pytest.raises(Exception, match="negative"):
        ops.coo_undirected_unique_(bad, dev(np.array([1, 2, 3], ITYPES[iname])))


# --------------------------------------------------------------------------------------------------------------- dense
@pytest.mark.parametrize("vname", list(VTYPES))
@pytest.mark.parametrize("iname", list(ITYPES))
def test_format_dense(ops, iname, vname):
    _, as_dt, unsigned = VTYPES[vname]
    n, m = 37, 53
    g = np.random.default_rng(21)
    cells = g.choice(n * m, 600, replace=False)  # (no duplicates, any order)
    row, col = (cells % n).astype(ITYPES[iname]), (cells // n).astype(ITYPES[iname])
    v = values(vname, len(row), 22)
    for p in PRECISIONS:
        got = text_of(ops.text_format_dense(n, m, dev(row), dev(col), dev(v, as_dt), precision=p, unsigned=unsigned))
        assert got == tr.format_dense(n, m, row, col, v, p), (p,)
    row2, col2 = np.append(row, row[5]), np.append(col, col[5])  # a coordinate stored twice
    with pytest.raises(Exception, match="twice"):
        ops.text_format_dense(n, m, dev(row2), dev(col2), dev(None if v is None else np.append(v, v[0]), as_dt),
                              unsigned=unsigned)
    row2[-1] = n  # outside the matrix
    with pytest.raises(Exception, match="outside"):
        ops.text_format_dense(n, m, dev(row2), dev(col2))
    from sparsebase_amd import capi
    with pytest.raises(capi.SbxError) as e:
        ops.text_format_dense(1 << 16, 1 << 15, dev(row), dev(col))
    assert e.value.status == 5


# ---------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("vname,precision", [("f32", 9), ("f64", 17)])
def test_round_trip_through_the_parser_is_bit_identical(ops, vname, precision):
    dt = VTYPES[vname][0]
    g = np.random.default_rng(31)
    nnz = 200000
    bits = np.uint32 if dt == np.float32 else np.uint64
    v = g.integers(0, np.iinfo(bits).max, nnz, dtype=bits, endpoint=True).view(dt).copy()
    v[~np.isfinite(v)] = dt(1.5)  # (the parser refuses inf / nan by design)
    v[:nnz // 2] = (g.random(nnz // 2) * 10.0 ** g.integers(-8, 8, nnz // 2)).astype(dt)
    row, col = coo("i32", 5000, 7000, nnz, 32)
    text = ops.text_format_coordinate(dev(row), dev(col), dev(v), precision=precision)
    r, c, w = ops.mtx_parse_coordinate(text, 5000, 7000, nnz, 3, value_dtype=torch.float32 if dt == np.float32 else torch.float64)
    assert np.array_equal(r.cpu().numpy(), row) and np.array_equal(c.cpu().numpy(), col)
    assert w.cpu().numpy().tobytes() == v.tobytes()


# ---------------------------------------------------------------------------------------------- the recorded reference
def test_golden_cases_through_the_abi(ops):
    """What the reference's own writers wrote (tools/make_text_writers_golden.py), composed here the way the host layer
    composes a file: the checks through sbx_coo_symmetry_check, the lines through the formatters."""
    import json
    z = np.load(os.path.join(ROOT, "tests", "golden", "text_writers.npz"))
    cases = json.loads(z["cases"].tobytes().decode())
    assert len(cases) >= 20
    ran = 0
    for k, case in enumerate(cases):
        want = z[f"file_{k}"].tobytes()
        if case["message"]:
            continue  # (the refusals are the host layer's: tests/test_text_writers_host.py, test_text_writers_hostlayer.py)
        val = z[f"val_{k}"] if f"val_{k}" in z.files else None
        dval = dev(val)
        if case["kind"] == "array":
            text = text_of(ops.text_format_values(dval))
            head = f"%%MatrixMarket {case['object']} {case['format']} {case['field']} {case['symmetry']}\n1 {len(val)}\n".encode()
        else:
            row, col = z[f"row_{k}"], z[f"col_{k}"]
            dr, dc = dev(row), dev(col)
            if case["kind"] == "edges":
                if not case["directed"]:
                    dr, dc, dval = ops.coo_undirected_unique_(dr, dc, dval)
                text, head = text_of(ops.text_format_coordinate(dr, dc, dval, index_base=0)), b""
            else:
                n, m = case["n"], case["m"]
                sym, size_nnz = case["symmetry"], len(row)
                head = f"%%MatrixMarket {case['object']} {case['format']} {case['field']} {sym}\n".encode()
                if sym != "general":
                    ok, diag, diag_nz = ops.coo_symmetry_check(n, dr, dc, dval, skew=sym == "skew-symmetric")
                    assert ok and not (sym == "skew-symmetric" and diag_nz)
                    size_nnz = len(row) - (len(row) - diag) // 2 - (diag if sym == "skew-symmetric" else 0)
                if case["format"] == "array":
                    head += f"{n} {m}\n".encode()
                    text = text_of(ops.text_format_dense(n, m, dr, dc, dval))
                else:
                    head += f"{n} {m} {size_nnz}\n".encode()
                    text = text_of(ops.text_format_coordinate(dr, dc, dval, lower=sym != "general",
                                                              no_diagonal=sym == "skew-symmetric",
                                                              pattern=case["field"] == "pattern"))
        assert head + text == want, case
        ran += 1
    assert ran >= 12


# ------------------------------------------------------------------------------------------------ more than 2^31 bytes
def test_a_text_of_more_than_two_to_the_31_bytes(ops):
    nnz = 130_000_000
    gen = torch.Generator(device="cuda")
    gen.manual_seed(41)
    row = torch.randint(0, 30_000_000, (nnz,), dtype=torch.int32, device="cuda", generator=gen)
    col = torch.randint(0, 30_000_000, (nnz,), dtype=torch.int32, device="cuda", generator=gen)

    def digits(x):  # of x + 1 (index_base 1)
        d = torch.ones_like(x, dtype=torch.int64)
        for k in range(1, 9):
            d += (x + 1 >= 10 ** k)
        return d
    line = digits(row) + digits(col) + 2
    ends = torch.cumsum(line, 0)
    total = int(ends[-1])
    assert total > 1 << 31
    text = ops.text_format_coordinate(row, col)  # pattern only
    assert text.numel() == total
    MB = 1 << 20

    def check(lo_entry, hi_entry):
        start = int(ends[lo_entry - 1]) if lo_entry else 0
        want = tr.format_coordinate(row[lo_entry:hi_entry].cpu().numpy(), col[lo_entry:hi_entry].cpu().numpy())
        assert len(want) >= MB
        assert text[start:start + len(want)].cpu().numpy().tobytes() == want
    per_mb = MB // 12 + 1  # (a line has at least 4 and at most 18 bytes; 12 and more on average here)
    check(0, 2 * per_mb)
    check(nnz - 2 * per_mb, nnz)
    mid = int(torch.searchsorted(ends, torch.tensor([1 << 31], device="cuda"))[0])
    lo = mid - per_mb
    assert int(ends[lo]) < (1 << 31) - MB // 2 and int(ends[mid + per_mb]) > (1 << 31) + MB // 2
    check(lo, mid + per_mb)
