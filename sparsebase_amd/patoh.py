"""The header line of a PaToH hypergraph file, on the host: what PatohReader's constructor reads before ReadHyperGraph's
line loop (io/patoh_reader.cc:11-43) and what PatohWriter::WriteHyperGraph writes before its own (io/patoh_writer.cc).  The
lines behind the header are the device's work: ops.patoh_parse / ops.patoh_format / ops.patoh_format_weights
(include/sbhg.h)."""
import re


class PatohHeaderError(ValueError):
    pass


def _stoi(tok, what):
    """std::stoi on one whitespace-separated token: the longest prefix that is a decimal integer; it throws if there is
    none (a missing token is the empty string, on which it throws as well)."""
    m = re.match(rb"[+-]?[0-9]+", tok)
    if m is None:
        raise PatohHeaderError(f"the header line does not give {what}")
    return int(m.group(0))


def parse_header(data):
    """data: the file's bytes.  Returns (base, cells, nets, pins, scheme, constraints, body_offset).  Leading lines that
    begin with '%' are skipped (the reference peeks at the first byte of each); the next line is the header
    `base cells nets pins [scheme [constraints]]`, every token read with stoi; scheme defaults to 0 (bit 0: the cells are
    weighted, bit 1: the nets are), constraints to 1.  body_offset is the offset of the byte behind the header line's '\\n'.
    Where the reference throws or reads garbage this raises: no header line, one of the four counts missing or negative,
    base outside {0, 1}, scheme outside 0..3."""
    pos = 0
    while pos < len(data) and data[pos:pos + 1] == b"%":
        end = data.find(b"\n", pos)
        pos = len(data) if end < 0 else end + 1
    if pos >= len(data):
        raise PatohHeaderError("no header line")
    end = data.find(b"\n", pos)
    stop = len(data) if end < 0 else end
    toks = data[pos:stop].split()
    names = ("the base", "the number of cells", "the number of nets", "the number of pins")
    base, cells, nets, pins = (_stoi(toks[i] if i < len(toks) else b"", names[i]) for i in range(4))
    scheme = _stoi(toks[4], "the scheme") if len(toks) > 4 else 0
    constraints = _stoi(toks[5], "the constraints") if len(toks) > 5 else 1
    if base not in (0, 1):
        raise PatohHeaderError(f"base {base}: 0 or 1")
    if cells < 0 or nets < 0 or pins < 0:
        raise PatohHeaderError("a negative count in the header line")
    if not 0 <= scheme <= 3:
        raise PatohHeaderError(f"scheme {scheme}: 0..3")
    return base, cells, nets, pins, scheme, constraints, (len(data) if end < 0 else end + 1)


def header_line(index_base, cells, nets, pins, nets_weighted=False, cells_weighted=False, constraints=1):
    """The writer's header line, with its '\\n': "base cells nets pins", then " scheme" when something is weighted, then
    " constraints" for schemes 1 and 2 when it is not 1 — and never for scheme 3, as the reference writes it."""
    scheme = (1 if cells_weighted else 0) | (2 if nets_weighted else 0)
    s = f"{index_base} {cells} {nets} {pins}"
    if scheme:
        s += f" {scheme}"
    if scheme in (1, 2) and constraints != 1:
        s += f" {constraints}"
    return (s + "\n").encode()
