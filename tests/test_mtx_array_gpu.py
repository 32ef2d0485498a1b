"""GPU tests of the dense side of the Matrix Market path (include/sbio.h, ops.mtx_parse_values / dense_to_coo /
coo_to_dense_vector):

  (a) sbio_dense_to_coo against np.nonzero, over shapes that straddle every edge of its 64 x 64 tiles, four densities,
      all six value types (with -0.0 among the floats: it must vanish), both id widths, count mode and the capacity check;
  (b) sbio_mtx_parse_values against the restatement's coordinate parser (oracle/: strtof / strtod / integer results) on
      the same tokens written as "1 1 <token>" entries, bit for bit, for every value type; texts longer than four
      4096-byte tiles with several values per line, tabs, CRLF and runs of blanks; its refusals;
  (c) both together against the real reference's MTXReader::ReadCOO on array files (the reference reports the
      dimensions swapped: include/sparsebase/io/mtx_reader.h);
  (d) sbio_coo_to_dense_vector: 1 x N and N x 1, an empty COO, the last of a duplicate position, a position == len;
  (e) round trips with the library's own writers (ops.text_format_dense / text_format_values).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mtxgen  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BAD_ARG, UNSUPPORTED = 1, 5
# (name, numpy dtype of the values, numpy dtype torch holds them in)
VALUE_TYPES = [("i32", np.int32, np.int32), ("u32", np.uint32, np.int32), ("f32", np.float32, np.float32),
               ("i64", np.int64, np.int64), ("u64", np.uint64, np.int64), ("f64", np.float64, np.float64)]
SHAPES = [(1, 1), (1, 257), (257, 1), (64, 64), (63, 65), (65, 63), (130, 67), (300, 3), (3, 300)]
DENSITIES = [0.0, 0.05, 0.5, 1.0]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: buffers of bytes objects are read-only)


def _vt(name):
    from sparsebase_amd import capi
    return {"i32": capi.V_I32, "u32": capi.V_U32, "f32": capi.V_F32, "i64": capi.V_I64, "u64": capi.V_U64, "f64": capi.V_F64}[name]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import ops
    return ops.handle_for(torch.device("cuda", torch.cuda.current_device()))


def _raw_dense_to_coo(hd, vt_name, it, n, m, dense_t, capacity, fill=True):
    """The C entry point itself (ops.dense_to_coo has no unsigned types and no capacity): (status, nnz, row, col, val)."""
    from sparsebase_amd import capi
    hd.bind_stream()
    idt = torch.int64 if it == capi.SBX_I64 else torch.int32
    row = torch.full((max(1, capacity),), -7, dtype=idt, device="cuda") if fill else None
    col = torch.full((max(1, capacity),), -7, dtype=idt, device="cuda") if fill else None
    val = torch.zeros(max(1, capacity), dtype=dense_t.dtype, device="cuda") if fill else None
    nnz = C.c_int64(-1)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = hd.lib.sbio_dense_to_coo(hd.h, it, _vt(vt_name), n, m, p(dense_t), capacity, p(row), p(col), p(val), C.byref(nnz))
    torch.cuda.synchronize()
    return rc, nnz.value, row, col, val


def _dense(n, m, density, name, vdt, seed):
    """Column-major cells; the floats get -0.0 at a tenth of the empty cells."""
    g = np.random.default_rng(seed)
    cells = n * m
    keep = g.random(cells) < density if 0.0 < density < 1.0 else np.full(cells, density >= 1.0)
    if vdt in (np.float32, np.float64):
        v = (g.standard_normal(cells) * 10.0 ** g.integers(-10, 10, cells)).astype(vdt)
        v[v == 0] = 1
        v[~keep] = 0
        v[~keep & (g.random(cells) < 0.1)] = -0.0
        if keep.any():
            v[np.nonzero(keep)[0][0]] = np.nan  # (nan != 0: kept)
    else:
        info = np.iinfo(vdt)
        v = g.integers(info.min, info.max, cells, dtype=vdt, endpoint=True)
        v[v == 0] = 1
        v[~keep] = 0
    return v


def _expect(n, m, v, idt):
    mat = v.reshape(m, n).T
    with np.errstate(invalid="ignore"):
        r, c = np.nonzero(mat != 0)
    return r.astype(idt), c.astype(idt), mat[r, c]


@pytest.mark.parametrize("name,vdt,tdt", VALUE_TYPES, ids=[v[0] for v in VALUE_TYPES])
@pytest.mark.parametrize("it_name", ["i32", "i64"])
def test_dense_to_coo_against_numpy(lib, name, vdt, tdt, it_name):
    from sparsebase_amd import capi
    it, idt = (capi.SBX_I32, np.int32) if it_name == "i32" else (capi.SBX_I64, np.int64)
    for si, (n, m) in enumerate(SHAPES):
        for di, density in enumerate(DENSITIES):
            v = _dense(n, m, density, name, vdt, 100 * si + di)
            d = _dev(v.view(tdt))
            wr, wc, wv = _expect(n, m, v, idt)
            rc, counted, *_ = _raw_dense_to_coo(lib, name, it, n, m, d, 0, fill=False)
            assert rc == 0 and counted == len(wr), (n, m, density, rc, counted, len(wr))
            rc, nnz, row, col, val = _raw_dense_to_coo(lib, name, it, n, m, d, len(wr))
            assert rc == 0 and nnz == len(wr), (n, m, density, lib.lib.sbx_last_error(lib.h))
            assert np.array_equal(row[:nnz].cpu().numpy(), wr) and np.array_equal(col[:nnz].cpu().numpy(), wc), (n, m, density)
            assert val[:nnz].cpu().numpy().tobytes() == wv.tobytes(), (n, m, density)
            if nnz:
                rc, left, row, col, val = _raw_dense_to_coo(lib, name, it, n, m, d, nnz - 1)
                assert rc == BAD_ARG, (n, m, density)
                assert nnz == 1 or bool((row == -7).all()), "a refused call wrote its outputs"


def test_dense_to_coo_through_ops_and_its_argument_checks(lib):
    from sparsebase_amd import capi, ops
    n, m = 130, 67
    v = _dense(n, m, 0.3, "f64", np.float64, 7)
    wr, wc, wv = _expect(n, m, v, np.int64)
    r, c, x = ops.dense_to_coo(n, m, _dev(v), torch.int64)
    assert r.dtype == torch.int64 and np.array_equal(r.cpu().numpy(), wr) and np.array_equal(c.cpu().numpy(), wc)
    assert x.cpu().numpy().tobytes() == wv.tobytes()
    assert ops.coo_is_sorted(r, c)
    r, c, x = ops.dense_to_coo(5, 4, _dev(np.zeros(20, np.float32)))
    assert r.numel() == 0 and c.numel() == 0 and x.numel() == 0
    d = _dev(np.ones(4, np.float32))
    nnz = C.c_int64(0)
    assert lib.lib.sbio_dense_to_coo(lib.h, capi.SBX_I32, capi.V_NONE, 2, 2, C.c_void_p(d.data_ptr()), 0, None, None, None,
                                     C.byref(nnz)) == BAD_ARG
    assert lib.lib.sbio_dense_to_coo(lib.h, capi.SBX_I32, capi.V_F32, 1 << 16, 1 << 15, C.c_void_p(d.data_ptr()), 0, None, None,
                                     None, C.byref(nnz)) == UNSUPPORTED  # (2^31 cells: refused before anything is read)
    # SBX_I32_N64 is SBX_I32 here
    rc, k, row, col, val = _raw_dense_to_coo(lib, "f32", capi.SBX_I32_N64, 2, 2, d, 4)
    assert rc == 0 and k == 4 and row.dtype == torch.int32 and row.cpu().tolist() == [0, 0, 1, 1] and col.cpu().tolist() == [0, 1, 0, 1]


# ------------------------------------------------------------------------------------------------ (b) parse_values
def _tokens(field, count, seed):
    """The value tokens of mtxgen.random_mtx (its generators, messy: 'E', '+'), without the coordinates."""
    toks = []
    while len(toks) < count:
        _, body, _, _, L = mtxgen.random_mtx(seed + len(toks), field, "general", n=200, nnz=4000, messy=True)
        toks += [line.split()[2] for line in body.splitlines() if line.strip()]
    return toks[:count]


def _array_text(toks, seed):
    """Several values per line, tabs, CRLF, runs of blanks."""
    g = np.random.default_rng(seed)
    seps = [" ", "\n", "\t", "\r\n", "   ", " \t ", "\n\n", "  \n"]
    return "".join(t + seps[int(g.integers(len(seps)))] for t in toks)


@functools.lru_cache(None)
def _parse_case(name):
    """(tokens, array text, what the restatement's coordinate parser returns for "1 1 <token>" entries)."""
    from orc import Oracle
    vdt = dict((v[0], v[1]) for v in VALUE_TYPES)[name]
    toks = _tokens("integer" if name[0] in "iu" else "real", 3000, {"i32": 1, "u32": 2, "f32": 3, "i64": 4, "u64": 5, "f64": 6}[name] * 10000)
    if name[0] == "u":
        toks = [t.lstrip("-") for t in toks]
    if name in ("i64", "u64"):  # beyond 32 bits too
        toks[5:5] = ["9223372036854775807", "4294967296", "1234567890123"]
        if name == "i64":
            toks[9:9] = ["-9223372036854775808", "-4294967297"]
        toks = toks[:3000]
    coord = "".join(f"1 1 {t}\n" for t in toks)
    _, _, want = Oracle().mtx_parse(coord.encode(), len(toks), 3, 0, True, False, np.int32, vdt)
    assert len(want) == len(toks)
    text = _array_text(toks, len(name)).encode()
    assert len(text) >= 4 * 4096
    return toks, text, want


@pytest.mark.parametrize("name,vdt,tdt", VALUE_TYPES, ids=[v[0] for v in VALUE_TYPES])
def test_parse_values_against_the_restatement(lib, name, vdt, tdt):
    from sparsebase_amd import capi
    toks, text, want = _parse_case(name)
    t = _dev(np.frombuffer(text, np.uint8))
    out = torch.zeros(len(toks), dtype=torch.from_numpy(np.zeros(0, tdt)).dtype, device="cuda")

    def call(text_t, count):
        lib.bind_stream()
        rc = lib.lib.sbio_mtx_parse_values(lib.h, _vt(name), C.c_void_p(text_t.data_ptr()), text_t.numel(), count,
                                           C.c_void_p(out.data_ptr()))
        torch.cuda.synchronize()
        return rc
    assert call(t, len(toks)) == 0, lib.lib.sbx_last_error(lib.h)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    # trailing tokens are ignored, garbage among them
    out.zero_()
    more = _dev(np.frombuffer(text + b" 17 nonsense 0x10\n", np.uint8))
    assert call(more, len(toks)) == 0
    assert out.cpu().numpy().tobytes() == want.tobytes()
    # a prefix: the first count tokens
    out.zero_()
    assert call(t, 1000) == 0
    assert out[:1000].cpu().numpy().tobytes() == want[:1000].tobytes() and not bool(out[1000:].any())
    # one token short
    assert call(t, len(toks) + 1) == BAD_ARG
    assert call(t, 0) == 0


@pytest.mark.parametrize("name,vdt,tdt", VALUE_TYPES, ids=[v[0] for v in VALUE_TYPES])
def test_parse_values_refusals(lib, name, vdt, tdt):
    from sparsebase_amd import capi, ops

    def status(text, count, vt=None):
        t = _dev(np.frombuffer(text, np.uint8))
        out = torch.zeros(max(1, count), dtype=torch.from_numpy(np.zeros(0, tdt)).dtype, device="cuda")
        lib.bind_stream()
        rc = lib.lib.sbio_mtx_parse_values(lib.h, _vt(name) if vt is None else vt, C.c_void_p(t.data_ptr()), t.numel(), count,
                                           C.c_void_p(out.data_ptr()))
        torch.cuda.synchronize()
        return rc
    assert status(b"1 2 3\n", 3) == 0
    assert status(b"1 2 3\n", 4) == BAD_ARG
    assert status(b"1 nan 3\n", 3) == BAD_ARG
    assert status(b"1 2 3\n", 3, capi.V_NONE) == BAD_ARG
    assert status(b"1 1.5 3\n", 3) == (BAD_ARG if name[0] in "iu" else 0)
    assert status(b"1 1.5 3\n", 1) == 0  # (behind the first `count` tokens: not looked at)
    digits = b"1." + b"1" * 40
    assert status(b"3 " + digits + b"\n", 2) == (BAD_ARG if name[0] in "iu" else UNSUPPORTED)
    if name == "f32":
        with pytest.raises(capi.SbxError):
            ops.mtx_parse_values(_dev(np.frombuffer(b"1 2\n", np.uint8)), 3, torch.float32)


# ------------------------------------------------------------------------------------------- (c) the real reference
REF_TUPLES = [("int-int", np.int32, np.int32), ("int-float", np.int32, np.float32), ("int-double", np.int32, np.float64),
              ("longlong-double", np.int64, np.float64)]


@pytest.mark.parametrize("tname,idt,vdt", REF_TUPLES, ids=[t[0] for t in REF_TUPLES])
@pytest.mark.parametrize("M,N", [(70, 70), (131, 40), (5, 200), (1, 90), (90, 1)])
def test_array_file_against_the_real_reference(ref, tmp_path, tname, idt, vdt, M, N):
    from sparsebase_amd import ops
    g = np.random.default_rng(M * 1000 + N)
    integer = vdt == np.int32
    toks = _tokens("integer" if integer else "real", M * N, 77 + M)
    for k in np.nonzero(g.random(M * N) < 0.4)[0]:
        toks[k] = ("0", "0.0", "-0", "0e5")[int(g.integers(4))] if not integer else "0"
    head = f"%%MatrixMarket matrix array {'integer' if integer else 'real'} general\n% a comment\n{M} {N}\n"
    body = "".join(t + ("\n", " ", "\t", "  \n")[int(g.integers(4))] for t in toks[:-1]) + toks[-1] + "\n"
    path = tmp_path / "array.mtx"
    path.write_text(head + body)
    ref_rows, ref_cols, rr, rc_, rv = ref.mtx_read(path, index_dtype=idt, value_dtype=vdt)
    tdt = torch.from_numpy(np.zeros(0, vdt)).dtype
    dense = ops.mtx_parse_values(_dev(np.frombuffer(body.encode(), np.uint8)), M * N, tdt)
    row, col, val = ops.dense_to_coo(M, N, dense, torch.from_numpy(np.zeros(0, idt)).dtype)
    # the reference constructs COO(N, M, ...): its dimensions come back swapped (the documented divergence)
    assert (ref_rows, ref_cols) == (N, M)
    assert len(rr) == row.numel() and len(rr) > 0
    assert np.array_equal(row.cpu().numpy(), rr) and np.array_equal(col.cpu().numpy(), rc_)
    assert val.cpu().numpy().tobytes() == rv.tobytes()


# ------------------------------------------------------------------------------------------- (d) coo_to_dense_vector
@pytest.mark.parametrize("idt", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("name,vdt,tdt", VALUE_TYPES, ids=[v[0] for v in VALUE_TYPES])
def test_coo_to_dense_vector(lib, idt, name, vdt, tdt):
    from sparsebase_amd import capi, ops
    g = np.random.default_rng(9)
    length, k = 1000, 300
    pos = np.sort(g.choice(length, k, replace=False)).astype(idt)
    pos[100] = pos[99]                   # a position stored twice, and
    pos[200] = pos[201] = pos[199]       # three times: the last of the run wins
    vals = g.integers(1, 1 << 30, k).astype(vdt)
    want = np.zeros(length, vdt)
    for p, x in zip(pos, vals):
        want[p] = x
    zero = np.zeros(k, idt)
    for row, col in ((zero, pos), (pos, zero)):  # 1 x N, N x 1
        out = ops.coo_to_dense_vector(length, _dev(row), _dev(col), _dev(vals.view(tdt)))
        assert out.cpu().numpy().tobytes() == want.tobytes()
    # an empty COO: zeros
    e = _dev(np.zeros(0, idt))
    out = ops.coo_to_dense_vector(17, e, e, _dev(np.zeros(0, tdt)))
    assert out.numel() == 17 and not bool(out.any())
    assert ops.coo_to_dense_vector(0, e, e, _dev(np.zeros(0, tdt))).numel() == 0
    # a position equal to len, a negative one
    for bad in (length, -1):
        p2 = pos.copy()
        p2[-1] = bad
        with pytest.raises(capi.SbxError) as err:
            ops.coo_to_dense_vector(length, _dev(zero), _dev(np.sort(p2) if bad < 0 else p2), _dev(vals.view(tdt)))
        assert err.value.status == BAD_ARG
    out = torch.zeros(4, dtype=torch.float32, device="cuda")
    lib.bind_stream()
    assert lib.lib.sbio_coo_to_dense_vector(lib.h, capi.SBX_I32, capi.V_NONE, 4, 0, None, None, None, C.c_void_p(out.data_ptr())) == BAD_ARG


# ------------------------------------------------------------------------------------------------ (e) round trips
@pytest.mark.parametrize("vdt,precision", [(np.float32, 9), (np.float64, 17)], ids=["f32", "f64"])
@pytest.mark.parametrize("idt", [np.int32, np.int64], ids=["i32", "i64"])
def test_round_trip_with_the_librarys_writers(lib, vdt, precision, idt):
    from sparsebase_amd import ops
    g = np.random.default_rng(precision)
    n, m, k = 150, 97, 4000
    cells = np.sort(g.choice(n * m, k, replace=False))
    row, col = (cells // m).astype(idt), (cells % m).astype(idt)  # (row, col) order
    val = (g.standard_normal(k) * 10.0 ** g.integers(-30, 30, k)).astype(vdt)
    val[::50] = 0   # stored zeros: written as "0", gone after the round trip
    val[25::50] = -0.0
    tdt = torch.from_numpy(np.zeros(0, vdt)).dtype
    text = ops.text_format_dense(n, m, _dev(row), _dev(col), _dev(val), precision=precision)
    dense = ops.mtx_parse_values(text, n * m, tdt)
    r, c, v = ops.dense_to_coo(n, m, dense, torch.from_numpy(np.zeros(0, idt)).dtype)
    keep = val != 0
    assert np.array_equal(r.cpu().numpy(), row[keep]) and np.array_equal(c.cpu().numpy(), col[keep])
    assert v.cpu().numpy().tobytes() == val[keep].tobytes()
    # values: the identity, zeros and signs of zeros included
    back = ops.mtx_parse_values(ops.text_format_values(_dev(val), precision=precision), k, tdt)
    assert back.cpu().numpy().tobytes() == val.tobytes()
