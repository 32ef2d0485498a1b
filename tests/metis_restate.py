"""CPU restatement of the METIS graph reader and writer (test infrastructure, no GPU, no library): the rules of
include/sbgr.h and of the host layer's header handling, in plain Python.  tests/test_metis_host.py checks it against
every case recorded from the real reference (tests/golden/metis_graph.npz); tests/test_metis_gpu.py takes it as the
expected value where no recording exists.

    read_graph(data, vtype, zero_index)          -> dict(n_dim, ncon, row, col, val, vwgt)   (MetisGraphReader::ReadGraph)
    parse_body(body, n, m, fmt, ncon, ...)       -> the same for the bytes behind the header  (sbgr_metis_parse)
    format_lines(row_ptr, col, ...)              -> the vertex lines                          (sbgr_metis_format)
    write_graph(n_dim, row, col, ...)            -> the whole file                            (MetisGraphWriter::WriteGraph)

A refusal is a Refusal carrying the sbx_status the ABI returns (BAD_ARG 1, UNSUPPORTED 5); HeaderError is what the host
layer throws as a ReaderException before the device is asked.
"""
import re
from decimal import Decimal
from fractions import Fraction

import numpy as np

BAD_ARG, UNSUPPORTED = 1, 5
DTYPES = {"void": None, "int": np.int32, "float": np.float32, "double": np.float64}
_INT = re.compile(rb"[+-]?[0-9]+\Z")
_DEC = re.compile(rb"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?\Z")


class Refusal(Exception):
    def __init__(self, status, msg):
        super().__init__(msg)
        self.status = status


class HeaderError(Exception):
    pass


def fmt(v, precision=6):
    """One value as `ostream << v` prints it."""
    if isinstance(v, (np.floating, float)):
        x = float(v)
        if x != x:
            return "-nan" if np.signbit(v) else "nan"
        return "%.*g" % (precision, x)
    return str(int(v))


def _f32(tok):
    """The float nearest to the decimal, ties to even: what strtof gives (float(tok) rounds twice)."""
    f = np.float32(float(tok))
    if not np.isfinite(f):
        return f
    x = Fraction(Decimal(tok.decode()))
    best = f
    for c in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
        if not np.isfinite(c):
            continue
        dc, db = abs(Fraction(float(c)) - x), abs(Fraction(float(best)) - x)
        if dc < db or (dc == db and int(c.view(np.uint32)) % 2 == 0 and int(best.view(np.uint32)) % 2 == 1):
            best = c
    return best


def parse_value(tok, dtype):
    if dtype == np.int32:
        if not _INT.match(tok) or not -2 ** 31 <= int(tok) < 2 ** 31:
            raise Refusal(BAD_ARG, f"malformed weight token {tok!r}")
        return np.int32(int(tok))
    if not _DEC.match(tok):
        raise Refusal(BAD_ARG, f"malformed weight token {tok!r}")
    return _f32(tok) if dtype == np.float32 else np.float64(float(tok))


def parse_header(data):
    """(n, m, fmt, ncon, body_offset) of the first line whose first byte is not '%'."""
    pos = 0
    while pos < len(data):
        end = data.find(b"\n", pos)
        line, nxt = (data[pos:], len(data)) if end < 0 else (data[pos:end], end + 1)
        if not line:
            raise HeaderError("an empty line before the header line")
        if line[:1] != b"%":
            vals = []
            for t in line.split()[:4]:
                m = re.match(rb"[+-]?[0-9]+", t)
                if not m:
                    break
                vals.append(int(m.group(0)))
                if m.end() != len(t):
                    break
            if len(vals) < 2 or vals[0] < 0 or vals[1] < 0:
                raise HeaderError("the header line does not give n and m")
            n, m_ = vals[0], vals[1]
            f = vals[2] if len(vals) > 2 else 0
            ncon = vals[3] if len(vals) > 3 else 0
            if f in (1, 11) and ncon == 0:
                ncon = 1
            if f not in (0, 1, 10, 11):
                raise HeaderError(f"FMT {f} is not supported")
            if ncon < 0:
                raise HeaderError("NCON is negative")
            return n, m_, f, ncon, nxt
        pos = nxt
    raise HeaderError("no header line")


def parse_body(body, n, m, fmt_, ncon, vtype, zero_index):
    """The rules of sbgr_metis_parse.  Returns dict(n_dim, nnz, row, col, val, vwgt, row_ptr); val / vwgt None where
    the ABI writes none."""
    if fmt_ not in (0, 1, 10, 11):
        raise Refusal(UNSUPPORTED, f"FMT {fmt_}")
    if len(body) >= 2 ** 32:
        raise Refusal(UNSUPPORTED, "text of 4 GiB and more")
    dtype = DTYPES[vtype]
    base = 0 if zero_index else 1
    n_dim, nnz = n + base, 2 * m
    ew, vw = fmt_ in (1, 11), fmt_ >= 10 and ncon > 0
    nvw = ncon if vw else 0
    lines = body.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # (a '\n' that ends the text starts no line)
    rows, cols, vals = [], [], []
    vwgt = np.zeros((n_dim, ncon), dtype) if (vw and dtype is not None) else None
    counts = np.zeros(n_dim, np.int64)
    vertex = base - 1
    parsed = []
    for line in lines:
        if line[:1] == b"%":
            continue
        vertex += 1
        toks = [t for t in re.split(rb"[ \t\r\v\f]+", line) if t]
        parsed.append((vertex, toks))
    if len(parsed) > n:
        raise Refusal(BAD_ARG, f"{len(parsed)} vertex lines, n is {n}")
    found = 0
    for vertex, toks in parsed:
        k = max(len(toks) - nvw, 0)
        if ew and k % 2:
            raise Refusal(BAD_ARG, "a neighbour without a weight")
        found += k // 2 if ew else k
    if found != nnz:
        raise Refusal(BAD_ARG, f"the lines hold {found} neighbours, m = {m} needs {nnz}")
    for vertex, toks in parsed:
        for j, t in enumerate(toks[:nvw]):
            if vwgt is not None:
                vwgt[vertex, j] = parse_value(t, dtype)
        rest = toks[nvw:]
        step = 2 if ew else 1
        for i in range(0, len(rest), step):
            if not _INT.match(rest[i]):
                raise Refusal(BAD_ARG, f"malformed neighbour token {rest[i]!r}")
            c = int(rest[i]) - (1 if zero_index else 0)
            if not 0 <= c < n_dim:
                raise Refusal(BAD_ARG, f"neighbour id {int(rest[i])} out of range")
            rows.append(vertex)
            cols.append(c)
            if ew and dtype is not None:
                vals.append(parse_value(rest[i + 1], dtype))
            counts[vertex] += 1
    row, col = np.array(rows, np.int64), np.array(cols, np.int64)
    order = np.lexsort((col, row))  # stable: equal (row, col) keep their file order
    val = np.array(vals, dtype)[order] if (ew and dtype is not None) else None
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return dict(n_dim=n_dim, nnz=nnz, row=row[order], col=col[order], val=val, vwgt=vwgt, row_ptr=row_ptr)


def read_graph(data, vtype, zero_index):
    """MetisGraphReader::ReadGraph: the Graph's n_dim, ncon_, COO arrays and vertex weights."""
    n, m, f, ncon, off = parse_header(data)
    out = parse_body(data[off:], n, m, f, ncon, vtype, zero_index)
    out["ncon"] = 0 if vtype == "void" else ncon  # (Graph::ncon_ is the derived NCON even where no weights are read)
    return out


def format_lines(row_ptr, col, val=None, vwgt=None, row_begin=0, row_end=None, index_base=1, precision=6,
                 edge_weights=False, vertex_weights=False):
    """The rules of sbgr_metis_format."""
    row_end = len(row_ptr) - 1 if row_end is None else row_end
    if edge_weights and val is None:
        raise Refusal(BAD_ARG, "edge weights without values")
    if vertex_weights and vwgt is None and val is None:
        raise Refusal(BAD_ARG, "vertex weights without a value type")
    ncon = 0 if vwgt is None else vwgt.shape[1]
    out = []
    for r in range(row_begin, row_end):
        s = ""
        if vertex_weights:
            s += "".join(fmt(vwgt[r, j], precision) + " " for j in range(ncon)) + "  "
        a, b = int(row_ptr[r]), int(row_ptr[r + 1])
        for e in range(a, b):
            s += " " + str(int(col[e]) + index_base)
            if edge_weights:
                s += " " + fmt(val[e], precision) + ("" if e + 1 == b else " ")
            if e + 1 != b:
                s += " "
        out.append(s + "\n")
    return "".join(out).encode()


def header_line(dim0, nnz, typed, edge_weighted, vertex_weighted, zero_indexed, ncon):
    s = f" {dim0 - (0 if zero_indexed else 1)} {nnz // 2}"
    if typed:
        s += " " + ("1" if (edge_weighted and not vertex_weighted) else "11" if edge_weighted else "10")
        if vertex_weighted and ncon > 0:
            s += f" {ncon}"
    return (s + "\n").encode()


def write_graph(n_dim, row, col, val, vwgt, ncon, vtype, edge_weighted, vertex_weighted, zero_indexed, precision=6):
    """MetisGraphWriter::WriteGraph of a Graph whose connectivity is the COO (row, col, val), sorted by (row, col)."""
    typed = vtype != "void"
    if typed and edge_weighted and val is None:
        raise Refusal(BAD_ARG, "edgeWeighted without values")           # the host layer's WriterException
    if typed and vertex_weighted and vwgt is None:
        raise Refusal(BAD_ARG, "vertexWeighted without vertex weights")  # likewise
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(row, np.int64), minlength=n_dim))])
    ew, vw = typed and edge_weighted, typed and vertex_weighted
    if vw and vwgt is not None and vwgt.shape[1] != ncon:
        vwgt = vwgt[:, :ncon]
    return header_line(n_dim, len(row), typed, ew, vw, zero_indexed, ncon if vw else 0) + format_lines(
        row_ptr, col, val if ew else None, vwgt if vw else None, 0 if zero_indexed else 1, n_dim,
        1 if zero_indexed else 0, precision, ew, vw)
