"""GPU tests of include/sbgr.h through sparsebase_amd.ops, all bit-exact: every case recorded from the real reference
(tests/golden/metis_graph.npz) with both index widths; texts built around the tokenizer's 4096-byte tile; a hub line;
degenerate files; every refusal; the formatter's protocol; a random graph of about 1 MB against the restatement
(tests/metis_restate.py, itself checked against the recording by tests/test_metis_host.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metis_restate as mr  # noqa: E402
from test_metis_host import CASES, GOLD, READ, REFUSALS, WRITE  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 4096
NPDT = {"void": None, "int": np.int32, "float": np.float32, "double": np.float64}
WIDTHS = [pytest.param(np.int32, np.int32, id="i32"), pytest.param(np.int64, np.int64, id="i64"),
          pytest.param(np.int32, np.int64, id="i32n64")]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import ops
    return ops


def _tdt(dt):
    return None if dt is None else torch.from_numpy(np.zeros(0, dt)).dtype


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _text(b, shift=0):
    """The bytes on the device; shift = 1 puts them at an address that is 1 modulo 16."""
    t = torch.from_numpy(np.frombuffer(b"\0" * shift + bytes(b), np.uint8).copy()).cuda()
    t = t[shift:]
    assert t.data_ptr() % 16 == shift % 16
    return t


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_parse(ops, body, n, m, fmt, ncon, vtype, zero, idt=np.int32, odt=np.int32, shift=0, want=None):
    want = mr.parse_body(body, n, m, fmt, ncon, vtype, zero) if want is None else want
    n_dim, row, col, val, vw, rp = ops.metis_parse(_text(body, shift), n, m, fmt, ncon, zero, _tdt(idt), _tdt(NPDT[vtype]),
                                                   _tdt(odt))
    assert n_dim == want["n_dim"]
    assert _bits(row.cpu().numpy(), want["row"].astype(idt)) and _bits(col.cpu().numpy(), want["col"].astype(idt))
    assert (val is None) == (want["val"] is None) and (val is None or _bits(val.cpu().numpy(), want["val"]))
    assert (vw is None) == (want["vwgt"] is None) and (vw is None or _bits(vw.cpu().numpy(), want["vwgt"]))
    assert _bits(rp.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(want["row"], minlength=n_dim))]).astype(odt))
    return want


# ------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("idt,odt", WIDTHS)
@pytest.mark.parametrize("name", sorted({CASES[k]["name"] for k in READ}))
def test_golden_reader_cases(ops, name, idt, odt):
    for k in (k for k in READ if CASES[k]["name"] == name):
        c = CASES[k]
        data = bytes(GOLD[f"in_{k}"])
        n, m, fmt, ncon, off = mr.parse_header(data)
        want = dict(n_dim=c["n_dim"], row=GOLD[f"row_{k}"], col=GOLD[f"col_{k}"],
                    val=GOLD[f"val_{k}"] if f"val_{k}" in GOLD else None, vwgt=GOLD[f"vw_{k}"] if f"vw_{k}" in GOLD else None)
        _check_parse(ops, data[off:], n, m, fmt, ncon, c["vtype"], c["zero"], idt, odt, want=want)


@pytest.mark.parametrize("idt,odt", WIDTHS)
def test_golden_writer_cases(ops, idt, odt):
    from sparsebase_amd import metis
    for k in WRITE:
        c = CASES[k]
        row, col = GOLD[f"row_{k}"], GOLD[f"col_{k}"]
        typed = c["vtype"] != "void"
        ew, vw = typed and c["ew"], typed and c["vw"]
        val = GOLD[f"val_{k}"] if f"val_{k}" in GOLD else None
        vwa = GOLD[f"vw_{k}"] if (vw and f"vw_{k}" in GOLD) else None
        rp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=c["n_dim"]))]).astype(odt)
        body = ops.metis_format(_dev(rp), _dev(col.astype(idt)), _dev(val), _dev(vwa), 0 if c["zero"] else 1, c["n_dim"],
                                1 if c["zero"] else 0, 6, ew, vw)
        head = metis.header_line(c["n_dim"], len(row), typed, ew, vw, c["zero"], c["ncon"] if vw else 0)
        assert head + bytes(body.cpu().numpy()) == bytes(GOLD[f"file_{k}"]), (k, c)


# ------------------------------------------------------------------------------------------- around the 4096-byte tile
def _tile_body():
    """About 2.5 tiles of an edge- and vertex-weighted graph with a comment line, rich in '%', behind every fifth line."""
    g = np.random.default_rng(5)
    n = 150
    adj = [[] for _ in range(n)]
    w = {}
    for i in range(n):
        for j in g.choice(n, 3, replace=False):
            j = int(j)
            if j != i and j + 1 not in adj[i]:
                adj[i].append(j + 1)
                adj[j].append(i + 1)
                w[(min(i, j), max(i, j))] = "%d.%d" % (g.integers(0, 999), g.integers(0, 99))
    lines = []
    for i in range(n):
        toks = [str(int(g.integers(1, 9999)))]
        for j in adj[i]:
            toks += [str(j), w[(min(i, j - 1), max(i, j - 1))]]
        lines.append(" ".join(toks).encode())
        if i % 5 == 4:
            lines.append(b"%% comment %%%% 1 2 3 %%%%%%%% x")
    return n, sum(len(a) for a in adj) // 2, b"\n".join(lines) + b"\n"


def _is_comment_at(text, p):
    start = text.rfind(b"\n", 0, p) + 1
    return text[start:start + 1] == b"%"


SPACE = b" \t\r\n"
TILE_CONDITIONS = {
    # a line and a token straddle byte 4096
    "token_straddles": lambda t: t[TILE - 1] not in SPACE and t[TILE] not in SPACE and not _is_comment_at(t, TILE),
    # a comment line straddles byte 8192, and a '%' in the middle of it sits at the tile's first byte
    "comment_straddles": lambda t: _is_comment_at(t, 2 * TILE) and t[2 * TILE - 1] != 10 and t[2 * TILE] == 37,
    # a '%' at a tile's first byte as a line start
    "percent_starts_tile": lambda t: t[TILE - 1] == 10 and t[TILE] == 37,
    # a vertex line starts exactly at byte 4096
    "line_starts_tile": lambda t: t[TILE - 1] == 10 and t[TILE] not in b"%\n",
}


@pytest.fixture(scope="module")
def tile_body():
    return _tile_body()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("cond", sorted(TILE_CONDITIONS))
def test_tile_boundaries(ops, tile_body, cond, shift):
    n, m, body = tile_body
    assert 2 * TILE < len(body) < 3 * TILE
    texts = (b"%" + b"-" * pad + b"\n" + body for pad in range(400))
    text = next(t for t in texts if TILE_CONDITIONS[cond](t))
    for vtype in ("double", "void"):
        _check_parse(ops, text, n, m, 11, 1, vtype, True, shift=shift)


def test_hub_line_and_row_sort(ops):
    """One line holds 20 000 of about 20 400 entries, its neighbours in descending order: the work is per token, and the
    one row out of order sends every row through the row sort."""
    g = np.random.default_rng(6)
    n = 20001
    adj = {i: [] for i in range(1, n + 1)}
    adj[1] = list(range(n, 1, -1))  # (a file need not be symmetric: the count alone is checked)
    for _ in range(200):
        a, b = (int(x) for x in g.integers(2, n + 1, 2))
        if a != b and b not in adj[a]:
            adj[a].append(b)
            adj[b].append(a)
    entries = sum(len(a) for a in adj.values())
    assert entries % 2 == 0 and 20300 <= entries <= 20400
    body = b"".join((" ".join("%d %d" % (j, (i * j) % 97) for j in adj[i]) + "\n").encode() for i in range(1, n + 1))
    for idt in (np.int32, np.int64):
        want = _check_parse(ops, body, n, entries // 2, 1, 1, "int", True, idt, idt)
    assert want["nnz"] == entries and np.bincount(want["row"])[0] == 20000


def test_degenerate_files(ops):
    for body, n in ((b"\n" * 5000, 5000), (b"\n" * 10 + b"% c\n\r\n \t \n", 40), (b"", 5), (b"% only\n", 0), (b"", 0)):
        for zero in (True, False):
            for vtype, fmt, ncon in (("void", 0, 0), ("float", 11, 2)):
                want = _check_parse(ops, body, n, 0, fmt, ncon, vtype, zero)
                assert want["nnz"] == 0 and len(want["row"]) == 0


def test_duplicate_neighbours_keep_file_order(ops):
    want = _check_parse(ops, b"2 7 2 3 2 5\n1 3 1 7 1 5\n", 2, 3, 1, 1, "int", True)
    assert want["val"].tolist() == [7, 3, 5, 3, 7, 5]
    want = _check_parse(ops, b"5 2\n6 1\n", 3, 1, 10, 1, "int", False)  # fewer lines than n: the rest of the weights is zero
    assert want["vwgt"].tolist() == [[0], [5], [6], [0]]


# ------------------------------------------------------------------------------------------- refusals
def _raw_parse(ops, body, n, m, fmt, ncon, vtype, zero, capacity, bytes_override=None, it=0):
    """The entry point itself, on outputs of `capacity` + 16 words filled with a sentinel.  Returns (status, outputs)."""
    from sparsebase_amd import capi
    text = _text(body if body else b" ")
    hd = ops.handle_for(text.device)
    dt = NPDT[vtype]
    n_dim = n + (0 if zero else 1)
    mk = lambda count, tdt: torch.full(((count + 16) * torch.empty(0, dtype=tdt).element_size(),), 0x5A, dtype=torch.uint8,
                                       device="cuda").view(tdt)
    row, col, rp = mk(capacity, torch.int32), mk(capacity, torch.int32), mk(n_dim + 1, torch.int32)
    val = None if dt is None else mk(capacity, _tdt(dt))
    vw = None if dt is None else mk(n_dim * max(ncon, 1), _tdt(dt))
    dims = (C.c_int64 * 2)()
    vt = capi.V_NONE if dt is None else ops._VT[_tdt(dt)]
    rc = hd.lib.sbgr_metis_parse(hd.h, it, vt, ops._p(text), len(body) if bytes_override is None else bytes_override, n, m, fmt,
                                 ncon, capi.GR_ZERO_INDEX if zero else 0, capacity, ops._p(row), ops._p(col), ops._p(val),
                                 ops._p(vw), ops._p(rp), dims)
    torch.cuda.synchronize()
    msg = hd.lib.sbx_last_error(hd.h).decode()
    return rc, msg, dict(row=row, col=col, val=val, rp=rp, vw=vw), dims


def _tail_intact(t, used):
    return t is None or bool((t[used:].view(torch.uint8) == 0x5A).all())


@pytest.mark.parametrize("body,n,m,fmt,ncon,vtype,zero,status", REFUSALS)
def test_refusals(ops, body, n, m, fmt, ncon, vtype, zero, status):
    nnz = 2 * m
    rc, msg, outs, dims = _raw_parse(ops, body, n, m, fmt, ncon, vtype, zero, nnz + 3)
    assert rc == status and msg and "sbgr_metis_parse" in msg
    assert all(_tail_intact(outs[k], nnz) for k in ("row", "col", "val"))
    n_dim = n + (0 if zero else 1)
    assert _tail_intact(outs["vw"], n_dim * ncon)  # (vwgt_out: n_dim x ncon values at the most)
    assert _tail_intact(outs["rp"], 0)             # (a refused call writes no row offset at all)
    assert dims[0] == 0 and dims[1] == 0


def test_refusals_name_their_counts_and_limits(ops):
    rc, msg, outs, _ = _raw_parse(ops, b"2 3\n1\n", 3, 3, 0, 0, "void", True, 6)
    assert rc == mr.BAD_ARG and "3 neighbours" in msg and "needs 6" in msg
    assert all(_tail_intact(outs[k], 0) for k in ("row", "col"))  # (refused before anything is written)
    # what is malformed is named: an id, a weight, or both (and a malformed id is not reported as one out of range)
    for text, what in ((b"2x 5\n1 5\n", "neighbour id token"), (b"2 0x10\n1 5\n", "weight token"),
                       (b"2x 0x10\n1 5\n", "neighbour id and weight tokens")):
        for zero in (True, False):
            rc, msg, _, _ = _raw_parse(ops, text, 3, 1, 1, 1, "int", zero, 2)
            assert rc == mr.BAD_ARG and msg == "sbgr_metis_parse: malformed " + what, msg
    rc, msg, outs, _ = _raw_parse(ops, b"2\n1\n", 2, 1, 0, 0, "void", True, 1)  # capacity one short
    assert rc == mr.BAD_ARG and "capacity" in msg and all(_tail_intact(outs[k], 0) for k in ("row", "col"))
    rc, msg, _, _ = _raw_parse(ops, b"2\n1\n", 2, 1, 0, 0, "void", True, 2, bytes_override=1 << 32)
    assert rc == mr.UNSUPPORTED and "4 GiB" in msg
    rc, msg, outs, dims = _raw_parse(ops, b"2\n1\n", 2, 1, 0, 0, "void", True, 5)  # (the same call, accepted)
    assert rc == 0 and dims[0] == 2 and dims[1] == 2 and outs["row"][:2].tolist() == [0, 1] and outs["col"][:2].tolist() == [1, 0]
    assert all(_tail_intact(outs[k], 2) for k in ("row", "col")) and outs["rp"][:3].tolist() == [0, 1, 2]
    assert _tail_intact(outs["rp"], 3)


# ------------------------------------------------------------------------------------------- the formatter
def _random_csr(seed, n, avg, dt, idt=np.int32, ncon=2):
    g = np.random.default_rng(seed)
    deg = g.poisson(avg, n)
    deg[g.integers(0, n, n // 10)] = 0
    rp = np.concatenate([[0], np.cumsum(deg)])
    col = np.concatenate([np.sort(g.choice(n, d, replace=False)) for d in deg] + [np.zeros(0, np.int64)]).astype(idt)
    if dt is None:
        return rp.astype(idt), col, None, None
    if dt == np.int32:
        return rp.astype(idt), col, g.integers(-9999, 9999, len(col)).astype(dt), g.integers(0, 99, (n, ncon)).astype(dt)
    val = (g.standard_normal(len(col)) * 10.0 ** g.integers(-8, 9, len(col))).astype(dt)
    return rp.astype(idt), col, val, g.random((n, ncon)).astype(dt)


@pytest.mark.parametrize("vtype", ["void", "int", "float", "double"])
def test_formatter_protocol(ops, vtype):
    from sparsebase_amd import capi
    dt = NPDT[vtype]
    n = 3000
    rp, col, val, vw = _random_csr(8, n, 4.0, dt)
    ew = vwf = dt is not None
    want = mr.format_lines(rp, col, val, vw, 0, n, 1, 6, ew, vwf)
    drp, dcol, dval, dvw = _dev(rp), _dev(col), _dev(val), _dev(vw)
    whole = ops.metis_format(drp, dcol, dval, dvw, edge_weights=ew, vertex_weights=vwf)
    assert bytes(whole.cpu().numpy()) == want
    # row chunks concatenate to the whole (chunk ends inside and between tiles of 256 items, empty chunks too)
    cuts = [0, 1, 1, 255, 256, 257, 1500, 2999, 3000]
    parts = [ops.metis_format(drp, dcol, dval, dvw, a, b, edge_weights=ew, vertex_weights=vwf) for a, b in zip(cuts, cuts[1:])]
    assert b"".join(bytes(p.cpu().numpy()) for p in parts) == want
    assert bytes(parts[-1].cpu().numpy()) == mr.format_lines(rp, col, val, vw, 2999, 3000, 1, 6, ew, vwf)
    # the sizing call, a capacity one byte short, a guard byte behind the length
    hd = ops.handle_for(drp.device)
    vt = capi.V_NONE if dt is None else ops._VT[_tdt(dt)]
    flags = (capi.GR_EDGE_WEIGHTS | capi.GR_VERTEX_WEIGHTS) if ew else 0
    call = lambda out, cap, nb: hd.lib.sbgr_metis_format(hd.h, 0, vt, 0, n, ops._p(drp), ops._p(dcol), ops._p(dval), ops._p(dvw),
                                                         2 if ew else 0, 1, 6, flags, out, cap, C.byref(nb))
    nb = C.c_int64(-1)
    assert call(None, 0, nb) == 0 and nb.value == len(want)
    for off in (0, 1):  # (an aligned and an unaligned text_out)
        buf = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[16 + off:]
        assert call(ops._p(out), len(want) - 1, nb) == mr.BAD_ARG and nb.value == len(want)
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all()), "a refused call wrote"
        assert call(ops._p(out), len(want), nb) == 0 and nb.value == len(want)
        got = buf.cpu().numpy()
        assert bytes(got[16 + off:16 + off + len(want)]) == want
        assert (got[:16 + off] == 0xA5).all() and (got[16 + off + len(want):] == 0xA5).all()


def test_formatter_refusals(ops):
    rp, col, val, vw = _random_csr(9, 50, 3.0, np.float32)
    drp, dcol, dval, dvw = _dev(rp), _dev(col), _dev(val), _dev(vw)
    from sparsebase_amd import capi
    with pytest.raises(capi.SbxError) as e:
        ops.metis_format(drp, dcol, None, dvw, edge_weights=True)
    assert e.value.status == mr.BAD_ARG
    with pytest.raises(capi.SbxError) as e:
        ops.metis_format(drp, dcol, None, None, vertex_weights=True)
    assert e.value.status == mr.BAD_ARG
    with pytest.raises(capi.SbxError) as e:
        ops.metis_format(drp, dcol, dval, dvw, precision=18, edge_weights=True)
    assert e.value.status == mr.BAD_ARG
    assert bytes(ops.metis_format(drp, dcol, row_begin=7, row_end=7).cpu().numpy()) == b""
    assert bytes(ops.metis_format(_dev(np.zeros(4, np.int32)), dcol[:0]).cpu().numpy()) == b"\n\n\n"


@pytest.mark.parametrize("vtype,precision", [("float", 9), ("double", 17)])
@pytest.mark.parametrize("idt,odt", WIDTHS)
def test_format_then_parse_reproduces_the_arrays(ops, vtype, precision, idt, odt):
    dt = NPDT[vtype]
    g = np.random.default_rng(10)
    n = 700
    pairs = np.unique(np.sort(g.integers(0, n, (2500, 2)), axis=1), axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    w = (g.standard_normal(len(pairs)) * 10.0 ** g.integers(-20, 20, len(pairs))).astype(dt)
    row = np.concatenate([pairs[:, 0], pairs[:, 1]])
    col = np.concatenate([pairs[:, 1], pairs[:, 0]])
    o = np.lexsort((col, row))
    row, col, val = row[o], col[o], np.concatenate([w, w])[o]
    rp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(odt)
    vw = g.random((n, 3)).astype(dt)
    text = ops.metis_format(_dev(rp), _dev(col.astype(idt)), _dev(val), _dev(vw), precision=precision, edge_weights=True,
                            vertex_weights=True)
    n_dim, r2, c2, v2, vw2, rp2 = ops.metis_parse(text, n, len(pairs), 11, 3, True, _tdt(idt), _tdt(dt), _tdt(odt))
    assert n_dim == n and _bits(r2.cpu().numpy(), row.astype(idt)) and _bits(c2.cpu().numpy(), col.astype(idt))
    assert _bits(v2.cpu().numpy(), val) and _bits(vw2.cpu().numpy(), vw) and _bits(rp2.cpu().numpy(), rp)


def test_one_megabyte_graph_against_the_restatement(ops):
    g = np.random.default_rng(12)
    n = 30000
    pairs = np.unique(np.sort(g.integers(0, n, (60000, 2)), axis=1), axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    w = g.integers(1, 10 ** 6, len(pairs))
    adj = [[] for _ in range(n)]
    for (a, b), x in zip(pairs.tolist(), w.tolist()):
        adj[a].append("%d %d.%03d" % (b + 1, x // 1000, x % 1000))
        adj[b].append("%d %d.%03d" % (a + 1, x // 1000, x % 1000))
    body = "".join(("%% vertex %d follows\n" % (i + 1) if i % 1000 == 0 else "") + "  ".join(t) + "\n"
                   for i, t in enumerate(adj)).encode()
    assert 1_000_000 < len(body) < 2_500_000
    want = _check_parse(ops, body, n, len(pairs), 1, 1, "double", False)
    # and back: the lines of rows 1 .. n of the 1-based graph, which this parser reads to the same arrays again
    text = ops.metis_format(_dev(want["row_ptr"].astype(np.int32)), _dev(want["col"].astype(np.int32)), _dev(want["val"]),
                            None, 1, n + 1, 0, 9, True, False)
    assert bytes(text.cpu().numpy()) == mr.format_lines(want["row_ptr"], want["col"], want["val"], None, 1, n + 1, 0, 9, True)
    _check_parse(ops, bytes(text.cpu().numpy()), n, len(pairs), 1, 1, "double", False, want=want)
