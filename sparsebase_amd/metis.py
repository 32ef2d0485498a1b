"""The header line of a METIS graph file, on the host: what MetisGraphReader::ReadGraph reads before its line loop
(io/metis_graph_reader.cc:26-39) and what MetisGraphWriter::WriteGraph writes before its own (io/metis_graph_writer.cc:
35-64).  The lines behind the header are the device's work: ops.metis_parse / ops.metis_format (include/sbgr.h)."""
import re


class MetisHeaderError(ValueError):
    pass


def _stream_int(tok):
    """`iss >> int` on one whitespace-separated token: the longest prefix that is a decimal integer, None if there is none
    (the extraction fails and every later one of the line with it)."""
    m = re.match(rb"[+-]?[0-9]+", tok)
    return None if m is None else int(m.group(0))


def parse_header(data):
    """data: the file's bytes.  Returns (n, m, fmt, ncon, body_offset): the header line is the first line whose first
    byte is not '%'; `n m [FMT [NCON]]` are read as ints (`011` is 11); fmt 1 / 11 without NCON has ncon 1; body_offset
    is the offset of the byte behind the header line's '\\n'.  n is the file's vertex count, m its edge count: the reader
    has n_dim = n + (0 if convert_to_zero_index else 1) rows and 2 * m entries.
    Where the reference reads garbage this raises: no header line, an empty line in front of it (the reference indexes an
    empty string), n or m missing or negative, FMT outside {0, 1, 10, 11}."""
    pos = 0
    while pos < len(data):
        end = data.find(b"\n", pos)
        stop = len(data) if end < 0 else end
        line = data[pos:stop]
        nxt = len(data) if end < 0 else end + 1
        if len(line) == 0:
            raise MetisHeaderError("an empty line before the header line")
        if line[:1] != b"%":
            toks = line.split()
            vals = []
            for t in toks[:4]:
                v = _stream_int(t)
                if v is None:
                    break
                vals.append(v)
                if len(t) != len(re.match(rb"[+-]?[0-9]+", t).group(0)):
                    break  # (the rest of the token stays in the stream and fails the next extraction)
            if len(vals) < 2 or vals[0] < 0 or vals[1] < 0:
                raise MetisHeaderError(f"the header line {bytes(line)!r} does not give n and m")
            n, m = vals[0], vals[1]
            fmt = vals[2] if len(vals) > 2 else 0
            ncon = vals[3] if len(vals) > 3 else 0
            if fmt in (1, 11) and ncon == 0:
                ncon = 1
            if fmt not in (0, 1, 10, 11):
                raise MetisHeaderError(f"FMT {fmt} (vertex sizes) is not supported: 0, 1, 10 or 11")
            if ncon < 0:
                raise MetisHeaderError(f"NCON {ncon} is negative")
            return n, m, fmt, ncon, nxt
        pos = nxt
    raise MetisHeaderError("no header line")


def header_line(dim0, nnz, typed, edge_weighted=False, vertex_weighted=False, zero_indexed=True, ncon=0):
    """The writer's header line, with its '\\n': " n m" for a graph without a value type (typed=False); otherwise
    " n m FMT[ NCON]" with FMT 1 / 11 / 10 under the reference's rule (a typed graph with neither flag writes 10) and
    NCON = ncon when vertex-weighted and ncon > 0.  n = dim0 - (0 if zero_indexed else 1), m = nnz // 2."""
    n = dim0 - (0 if zero_indexed else 1)
    s = f" {n} {nnz // 2}"
    if typed:
        fmt = "1" if (edge_weighted and not vertex_weighted) else "11" if edge_weighted else "10"
        s += " " + fmt
        if vertex_weighted and ncon > 0:
            s += f" {ncon}"
    return (s + "\n").encode()
