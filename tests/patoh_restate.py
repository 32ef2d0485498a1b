"""The PaToH reader and writer restated in numpy: what the reference's PatohReader::ReadHyperGraph holds after reading a
file for which it is defined, and what the library's PatohWriter writes (which is the reference's PatohWriter wherever that
one writes at all).  tests/test_patoh_host.py checks both against tests/golden/patoh.npz, recorded from the reference;
tests/test_patoh_gpu.py checks the device against this file where the golden cases end."""
import json
import os
import re

import numpy as np

from sparsebase_amd import patoh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patoh.npz")
DTYPES = {"void": None, "int": np.int32, "float": np.float32, "double": np.float64}


def load_golden():
    """The cases of tests/golden/patoh.npz (tools/make_patoh_golden.py) with their arrays unpacked: `in` / `file` as bytes,
    xpin / pin / xnet / net as int64 arrays, nw / cw in the case's value type."""
    z = np.load(GOLDEN)
    ints, text = z["ints"], z["text"]
    cases = json.loads(bytes(z["cases"]).decode())
    for c in cases:
        for key in ("in", "file"):
            if key in c:
                c[key] = bytes(text[c[key][0]:c[key][0] + c[key][1]])
        for key in ("xpin", "pin", "xnet", "net", "nw", "cw"):
            if key in c:
                arr = ints[c[key][0]:c[key][0] + c[key][1]]
                c[key] = arr.astype(DTYPES[c["vtype"]]) if key in ("nw", "cw") else arr
    return cases


class Refused(ValueError):
    """A file on which the reference has undefined behaviour (the library refuses it)."""


def _int(tok):
    if re.fullmatch(rb"[+-]?[0-9]+", tok) is None:
        raise Refused(f"malformed token {tok!r}")
    return int(tok)


def body_lines(body):
    """getline over the body: (line, at_eof) pairs; at_eof is what fin.eof() says behind the getline that read the line."""
    if not body:
        return []
    parts = body.split(b"\n")
    ends_nl = body.endswith(b"\n")
    if ends_nl:
        parts.pop()
    return [(p, (not ends_nl) and i == len(parts) - 1) for i, p in enumerate(parts)]


def cells_to_nets(xpin, pin, cells, base):
    """xnet, net: row c lists, in ascending pin position, the net (+ base) of every pin equal to c + base."""
    xpin, pin = np.asarray(xpin, np.int64), np.asarray(pin, np.int64)
    order = np.argsort(pin - base, kind="stable")
    net = np.searchsorted(xpin, order, side="right") - 1 + base
    xnet = np.zeros(cells + 1, np.int64)
    np.cumsum(np.bincount(pin - base, minlength=cells), out=xnet[1:])
    return xnet, net


def parse_body(body, cells, nets, pins, base, scheme, dtype=None):
    """The lines behind the header -> dict(xpin, pin, xnet, net, nw, cw) (nw, cw None with dtype None).  Raises Refused
    where the library refuses."""
    xpin, pin, nw, cw = [0], [], [], []
    for line, eof in body_lines(body):
        if line[:1] == b"%":
            continue
        toks = line.split()
        if (scheme & 1) and eof:
            cw = [_int(t) for t in toks] if dtype is not None else [0] * len(toks)
            continue
        if scheme & 2:
            if not toks:
                raise Refused("a net line without a weight")
            nw.append(_int(toks[0]) if dtype is not None else 1)
            toks = toks[1:]
        pin.extend(_int(t) for t in toks)
        xpin.append(len(pin))
    if len(xpin) - 1 != nets:
        raise Refused(f"{len(xpin) - 1} net lines, nets = {nets}")
    if len(pin) != pins:
        raise Refused(f"{len(pin)} pins, pins = {pins}")
    if len(cw) > cells:
        raise Refused(f"{len(cw)} cell weights, cells = {cells}")
    pin = np.array(pin, np.int64)
    if len(pin) and (pin.min() < base or pin.max() >= cells + base):
        raise Refused("a pin out of range")
    xnet, net = cells_to_nets(xpin, pin, cells, base)
    out = dict(xpin=np.array(xpin, np.int64), pin=pin, xnet=xnet, net=net, nw=None, cw=None)
    if dtype is not None:
        out["nw"] = np.array(nw + [1] * (nets - len(nw)), np.int64).astype(dtype)
        out["cw"] = np.array(cw + [1] * (cells - len(cw)), np.int64).astype(dtype)
    return out


def read(data, dtype=None):
    """A whole file -> the dict of parse_body plus base, cells, nets, pins, scheme, constraints."""
    base, cells, nets, pins, scheme, constraints, off = patoh.parse_header(data)
    out = parse_body(data[off:], cells, nets, pins, base, scheme, dtype)
    out.update(base=base, cells=cells, nets=nets, pins=pins, scheme=scheme, constraints=constraints)
    return out


def net_lines(xpin, pin, nw=None, delta=0, net_begin=0, net_end=None, last_newline=True, value_text=None):
    """The lines of nets [net_begin, net_end) as sbhg_patoh_format writes them; value_text(v) -> bytes prints a weight."""
    net_end = len(xpin) - 1 if net_end is None else net_end
    value_text = value_text or (lambda v: b"%d" % int(v))
    out = []
    for j in range(net_begin, net_end):
        toks = [value_text(nw[j])] if nw is not None else []
        toks += [b"%d" % (int(p) + delta) for p in pin[xpin[j]:xpin[j + 1]]]
        out.append(b" ".join(toks))
    text = b"".join(l + b"\n" for l in out)
    if not last_newline and out:
        text = text[:-1]
    return text


def weight_line(w, begin=0, end=None, value_text=None):
    end = len(w) if end is None else end
    value_text = value_text or (lambda v: b"%d" % int(v))
    return b"".join((b" " if i else b"") + value_text(w[i]) for i in range(begin, end))


def write(hg, zero_indexed, net_weighted, cell_weighted, value_text=None):
    """The file PatohWriter(filename, zero_indexed, net_weighted, cell_weighted) writes for hg = dict(base, cells, nets,
    constraints, xpin, pin, nw, cw).  Ids are written as stored + (0 if zero_indexed else 1) - base.  No '\\n' behind the
    file's last line — unless that line is an empty net, which would otherwise be lost."""
    idx = 0 if zero_indexed else 1
    xpin, pin = hg["xpin"], hg["pin"]
    nets = len(xpin) - 1
    text = patoh.header_line(idx, hg["cells"], nets, len(pin), net_weighted, cell_weighted, hg["constraints"])
    last_empty = nets > 0 and xpin[nets] == xpin[nets - 1] and not net_weighted
    text += net_lines(xpin, pin, hg["nw"] if net_weighted else None, idx - hg["base"],
                      last_newline=cell_weighted or last_empty, value_text=value_text)
    if cell_weighted:
        text += weight_line(hg["cw"], value_text=value_text)
    return text
