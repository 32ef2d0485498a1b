"""GPU tests of include/sbhg.h through sparsebase_amd.ops, all bit-exact: every case recorded from the real reference
(tests/golden/patoh.npz) with the three index tuples; texts built around the tokenizer's 4096-byte tile; a net and a cell
of 20 000 pins; the transpose at its degenerate sizes and on both sides of the switch between its sorts; every refusal
with canaries; the formatters' protocol; format -> parse; a random hypergraph of about 1 MB against the restatement
(tests/patoh_restate.py, itself checked against the recording by tests/test_patoh_host.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import patoh_restate as pr  # noqa: E402
from test_patoh_host import READ, WRITE  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 4096
COUNT_SORT_MAX = 1 << 20  # sbx_countsort.h: MAX_PAIRS, where sbhg_cells_to_nets switches to the one-sweep radix sort
WIDTHS = [pytest.param(np.int32, np.int32, id="i32"), pytest.param(np.int64, np.int64, id="i64"),
          pytest.param(np.int32, np.int64, id="i32n64")]
CANARY = 0x5A


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


def _check_parse(ops, body, cells, nets, pins, base, scheme, vdt, idt=np.int32, odt=np.int32, shift=0, want=None):
    want = pr.parse_body(body, cells, nets, pins, base, scheme, vdt) if want is None else want
    xpin, pin, xnet, net, nw, cw = ops.patoh_parse(_text(body, shift), cells, nets, pins, base, scheme, _tdt(idt), _tdt(vdt),
                                                   _tdt(odt))
    for got, key, dt in ((xpin, "xpin", odt), (pin, "pin", idt), (xnet, "xnet", odt), (net, "net", idt)):
        assert _bits(got.cpu().numpy(), np.asarray(want[key]).astype(dt)), key
    for got, key in ((nw, "nw"), (cw, "cw")):
        assert (got is None) == (vdt is None)
        if got is not None:
            assert _bits(got.cpu().numpy(), want[key]), key
    return want


# ------------------------------------------------------------------------------------------- the recorded cases
@pytest.mark.parametrize("idt,odt", WIDTHS)
@pytest.mark.parametrize("name", sorted({c["name"] for c in READ}))
def test_golden_reader_cases(ops, name, idt, odt):
    from sparsebase_amd import patoh
    for c in (c for c in READ if c["name"] == name):
        base, cells, nets, pins, scheme, constraints, off = patoh.parse_header(c["in"])
        assert (nets, pins, cells, base, constraints) == (c["n"], c["m"], c["cells"], c["base"], c["constraints"])
        vdt = pr.DTYPES[c["vtype"]]
        want = {k: c.get(k) for k in ("xpin", "pin", "xnet", "net", "nw", "cw")}
        _check_parse(ops, c["in"][off:], cells, nets, pins, base, scheme, vdt, idt, odt, want=want)


def _dev_write(ops, hg, zero, ew, vw, idt=np.int32, odt=np.int32, chunk=None, precision=6):
    """A whole file as the host layer's PatohWriter assembles it: header, the net lines (in chunks of `chunk` nets), the
    cell-weight line."""
    from sparsebase_amd import patoh
    idx = 0 if zero else 1
    xpin, pin = _dev(np.asarray(hg["xpin"]).astype(odt)), _dev(np.asarray(hg["pin"]).astype(idt))
    nets = len(hg["xpin"]) - 1
    nw = _dev(hg["nw"]) if ew else None
    out = patoh.header_line(idx, hg["cells"], nets, len(hg["pin"]), ew, vw, hg["constraints"])
    last_empty = nets > 0 and hg["xpin"][nets] == hg["xpin"][nets - 1] and not ew
    chunk = chunk or max(1, nets)
    for b in range(0, nets, chunk):
        e = min(nets, b + chunk)
        out += bytes(ops.patoh_format(xpin, pin, nw, b, e, idx - hg["base"], precision, ew,
                                      last_newline=(e < nets) or vw or last_empty).cpu().numpy())
    if vw:
        out += bytes(ops.patoh_format_weights(_dev(hg["cw"]), precision=precision).cpu().numpy())
    return out


@pytest.mark.parametrize("idt,odt", WIDTHS)
def test_golden_writer_cases(ops, idt, odt):
    for c in WRITE:
        before = {k: c[k].copy() for k in ("xpin", "pin", "nw", "cw")}
        assert _dev_write(ops, c, c["zero"], c["ew"], c["vw"], idt, odt, chunk=3) == c["file"], c
        assert all(_bits(c[k], v) for k, v in before.items())


# ------------------------------------------------------------------------------------------- around the 4096-byte tile
def _tile_file(kind):
    """A net- and cell-weighted body (scheme 3, base 1) in which `kind` happens at byte 4096: filler nets, a comment line
    that pads to the byte wanted, the line in question, more nets, the cell-weight line."""
    g = np.random.default_rng(7)
    cells = 2600 if kind == "cw_three_tiles" else 40
    lines, pins, nets = [], 0, 0

    def net(k, weight=None, first=None):
        nonlocal pins, nets
        ps = [int(x) for x in g.integers(1, cells + 1, k)]
        if first is not None:
            ps[0] = first
        pins += k
        nets += 1
        return ("%d " % (int(g.integers(1, 999)) if weight is None else weight) + " ".join(map(str, ps))).encode()
    for _ in range(60):
        lines.append(net(int(g.integers(1, 6))))
        if nets % 7 == 0:
            lines.append(b"% 1 2 3 % a comment")
    head = b"\n".join(lines) + b"\n"
    # where the line in question has to start so that `kind` falls on byte 4096
    start = {"token_straddles": TILE - 3, "line_starts": TILE, "comment_starts": TILE, "weight_straddles": TILE - 3}.get(kind)
    tail_nets = [net(int(g.integers(1, 6))) for _ in range(25)]
    if kind == "cw_three_tiles":  # the cell-weight line starts at a tile's first byte and is longer than two tiles
        body = head + b"\n".join(tail_nets) + b"\n"
        body += b"%" + b"x" * ((-(len(body) + 2)) % TILE) + b"\n"
        assert len(body) % TILE == 0
        line = " ".join("%3d" % w for w in g.integers(1, 999, cells)).encode()
        assert len(line) > 2 * TILE
        return body + line, cells, nets, pins
    pad = start - len(head) - 2
    assert pad >= 0
    body = head + b"%" + b"x" * pad + b"\n"
    assert len(body) == start
    if kind == "token_straddles":
        body += net(3, weight=7, first=40) + b"\n"  # "7 40 ..": the pin 40 lies on bytes 4095 and 4096
    elif kind == "line_starts":
        body += net(4) + b"\n"
    elif kind == "comment_starts":
        body += b"% 5 6 7 at the start of a tile\n"
    elif kind == "weight_straddles":
        body += net(2, weight=987654) + b"\n"
    body += b"\n".join(tail_nets) + b"\n"
    body += " ".join(str(int(x)) for x in g.integers(1, 999, cells)).encode()
    return body, cells, nets, pins


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("kind", ["token_straddles", "line_starts", "comment_starts", "cw_three_tiles", "weight_straddles"])
def test_around_the_tile(ops, kind, shift):
    body, cells, nets, pins = _tile_file(kind)
    if kind == "token_straddles":  # a token with bytes on both sides of 4096
        assert body[TILE - 2:TILE + 2] == b" 40 "
    if kind == "weight_straddles":
        assert body[TILE - 3:TILE + 3] == b"987654"
    if kind in ("line_starts", "comment_starts"):
        assert body[TILE - 1:TILE] == b"\n" and (body[TILE:TILE + 1] == b"%") == (kind == "comment_starts")
    for vdt in (np.int32, np.float64, None):
        _check_parse(ops, body, cells, nets, pins, 1, 3, vdt, shift=shift)


# ------------------------------------------------------------------------------------------- long lines, long rows
def test_one_net_of_20000_pins_and_one_cell_in_20000_nets(ops):
    g = np.random.default_rng(8)
    cells = 300
    big = " ".join(str(int(x)) for x in g.integers(0, cells, 20000))
    small = [" ".join(str(int(x)) for x in g.integers(0, cells, 3)) for _ in range(50)]
    body = ("\n".join(small[:20] + [big] + small[20:]) + "\n").encode()
    _check_parse(ops, body, cells, 51, 20150, 0, 0, None)
    # cell 7 in every one of 20 000 nets: a row of the transpose longer than a workgroup's share
    lines = ["%d 7 %d" % (int(g.integers(1, 9)), int(g.integers(0, cells))) for _ in range(20000)]
    body = ("\n".join(lines) + "\n" + " ".join(["3"] * cells)).encode()
    want = _check_parse(ops, body, cells, 20000, 40000, 0, 3, np.int32)
    assert want["xnet"][8] - want["xnet"][7] >= 20000


# ------------------------------------------------------------------------------------------- the transpose alone
def _check_transpose(ops, xpin, pin, cells, base, idt=np.int32, odt=np.int32):
    xnet, net = ops.cells_to_nets(_dev(np.asarray(xpin).astype(odt)), _dev(np.asarray(pin).astype(idt)), cells, base)
    wx, wn = pr.cells_to_nets(xpin, pin, cells, base)
    assert _bits(xnet.cpu().numpy(), wx.astype(odt)) and _bits(net.cpu().numpy(), wn.astype(idt))


def _random_csr(g, nets, pins, cells, base):
    xpin = np.concatenate([[0], np.sort(g.integers(0, pins + 1, nets - 1)), [pins]]).astype(np.int64)
    return xpin, g.integers(base, cells + base, pins)


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("pins", [0, 1, 63, 64, 65, 5000])
def test_cells_to_nets_small(ops, pins, base):
    g = np.random.default_rng(pins + base)
    for idt, odt in ((np.int32, np.int32), (np.int64, np.int64), (np.int32, np.int64)):
        xpin, pin = _random_csr(g, 9, pins, 17, base)
        _check_transpose(ops, xpin, pin, 17, base, idt, odt)


@pytest.mark.parametrize("pins", [COUNT_SORT_MAX, COUNT_SORT_MAX + 1])
def test_cells_to_nets_on_both_sides_of_the_sort_switch(ops, pins):
    g = np.random.default_rng(pins & 0xFF)
    xpin, pin = _random_csr(g, 70001, pins, 33333, 1)
    _check_transpose(ops, xpin, pin, 33333, 1)


@pytest.mark.parametrize("base", [0, 1])
def test_cells_to_nets_degenerate_rows(ops, base):
    g = np.random.default_rng(9)
    xpin, _ = _random_csr(g, 40, 3000, 50, base)
    _check_transpose(ops, xpin, np.full(3000, 12 + base), 50, base)            # all pins in one cell
    _check_transpose(ops, xpin, np.full(3000, 49 + base), 50, base)            # every cell empty but the last
    _check_transpose(ops, xpin, np.full(3000, base), 1, base)                  # one cell: no bit to sort by
    _check_transpose(ops, np.zeros(1, np.int64), np.zeros(0, np.int64), 5, base)  # no net at all


def test_cells_to_nets_refusals(ops):
    from sparsebase_amd import capi
    xpin = _dev(np.array([0, 2, 4], np.int32))
    for pin, base in (([0, 1, 2, 5], 0), ([0, 1, 2, 3], 1), ([1, 2, 3, 6], 1)):
        with pytest.raises(capi.SbxError) as e:
            ops.cells_to_nets(xpin, _dev(np.array(pin, np.int32)), 5, base)
        assert e.value.status == 1 and "a pin outside" in str(e.value)
    with pytest.raises(capi.SbxError) as e:
        ops.cells_to_nets(_dev(np.array([0, 3, 2], np.int32)), _dev(np.zeros(3, np.int32)), 5, 0)
    assert e.value.status == 1 and "descends" in str(e.value)


# ------------------------------------------------------------------------------------------- refusals
def _raw_parse(ops, body, cells, nets, pins, base, scheme, vdt=np.int32, capacity=None, extra=8):
    """The entry point itself over outputs filled with a canary: (status, message, outputs as numpy, counts)."""
    t = _text(body)
    hd = ops.handle_for(t.device)
    cap = max(0, pins) + extra if capacity is None else capacity
    mk = lambda n, dt: torch.full(((max(0, n) + extra) * np.dtype(dt).itemsize,), CANARY, dtype=torch.uint8,
                                  device=t.device).view(_tdt(dt))
    outs = dict(xpin=mk(nets + 1, np.int32), pin=mk(pins, np.int32), xnet=mk(cells + 1, np.int32), net=mk(pins, np.int32),
                nw=mk(nets, vdt or np.int32), cw=mk(cells, vdt or np.int32))
    vt = 0 if vdt is None else ops._VT[_tdt(vdt)]
    counts = (C.c_int64 * 3)()
    p = lambda k: C.c_void_p(outs[k].data_ptr())
    rc = hd.lib.sbhg_patoh_parse(hd.h, 0, vt, C.c_void_p(t.data_ptr()), t.numel(), cells, nets, pins, base, scheme, cap,
                                 p("xpin"), p("pin"), p("xnet"), p("net"), p("nw"), p("cw"), counts)
    torch.cuda.synchronize()
    msg = hd.lib.sbx_last_error(hd.h).decode()
    return rc, msg, {k: v.cpu().numpy().view(np.uint8) for k, v in outs.items()}, list(counts)


def _untouched(outs, cells, nets, pins, vb=4):
    """A refused call: nothing in the offset arrays, nothing behind the stated extents of the others."""
    assert (outs["xpin"] == CANARY).all() and (outs["xnet"] == CANARY).all()
    for key, n, b in (("pin", pins, 4), ("net", pins, 4), ("nw", nets, vb), ("cw", cells, vb)):
        assert (outs[key][max(0, n) * b:] == CANARY).all(), key


REFUSED = [  # (id, body, cells, nets, pins, base, scheme, status, what the message names)
    ("more_net_lines", b"1 2\n3 4\n1 4\n", 4, 2, 6, 1, 0, 1, ("3 net lines", "nets is 2")),
    ("fewer_net_lines", b"1 2\n3 4\n", 4, 3, 4, 1, 0, 1, ("2 net lines", "nets is 3")),
    ("weighted_file_ends_in_newline", b"1 2\n3 4\n7 7 7 7\n", 4, 2, 4, 1, 1, 1, ("3 net lines", "nets is 2", "newline")),
    ("more_pins", b"1 2 3\n3 4\n", 4, 2, 4, 1, 0, 1, ("hold 5 pins", "pins is 4")),
    ("fewer_pins", b"1 2\n3 4\n", 4, 2, 5, 1, 0, 1, ("hold 4 pins", "pins is 5")),
    ("more_cell_weights", b"1 2\n3 4\n7 7 7 7 7", 4, 2, 4, 1, 1, 1, ("5 cell weights", "cells is 4")),
    ("pin_below_base", b"1 2\n0 4\n", 4, 2, 4, 1, 0, 1, ("a pin outside [1, 4]",)),
    ("pin_above", b"1 2\n3 4\n", 4, 2, 4, 0, 0, 1, ("a pin outside [0, 3]",)),
    ("malformed_pin", b"1 2\n3 4x\n", 4, 2, 4, 1, 0, 1, ("malformed pin token",)),
    ("float_pin", b"1 2\n3 4.0\n", 4, 2, 4, 1, 0, 1, ("malformed pin token",)),
    ("malformed_weight", b"1.5 1 2\n2 3 4\n", 4, 2, 4, 1, 2, 1, ("malformed weight token",)),
    ("malformed_cell_weight", b"1 2\n3 4\n7 7 x 7", 4, 2, 4, 1, 1, 1, ("malformed weight token",)),
    ("weighted_net_without_tokens", b"5 1 2\n\n5 3 4\n", 4, 3, 4, 1, 2, 1, ("no weight",)),
    ("base_2", b"1 2\n", 4, 1, 2, 2, 0, 1, ("base",)),
    ("scheme_4", b"1 2\n", 4, 1, 2, 1, 4, 1, ("scheme",)),
    ("negative_cells", b"1 2\n", -1, 1, 2, 1, 0, 1, ("negative",)),
    ("cells_2_31", b"1 2\n", 1 << 31, 1, 2, 1, 0, 5, ("2^31",)),
]


@pytest.mark.parametrize("cid,body,cells,nets,pins,base,scheme,status,names", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals(ops, cid, body, cells, nets, pins, base, scheme, status, names):
    if cells < 100:
        rc, msg, outs, counts = _raw_parse(ops, body, cells, nets, pins, base, scheme)
        _untouched(outs, max(0, cells), nets, pins)
    else:  # (2^31 cells: outputs of that size are never touched, and never allocated here)
        t = _text(body)
        hd = ops.handle_for(t.device)
        counts = (C.c_int64 * 3)()
        one = torch.zeros(16, dtype=torch.int32, device=t.device)
        p = C.c_void_p(one.data_ptr())
        rc = hd.lib.sbhg_patoh_parse(hd.h, 0, 0, C.c_void_p(t.data_ptr()), t.numel(), cells, nets, pins, base, scheme, 16, p, p,
                                     None, None, None, None, counts)
        msg = hd.lib.sbx_last_error(hd.h).decode()
        assert (one.cpu().numpy() == 0).all()
    assert rc == status, (rc, msg)
    for name in names:
        assert name in msg, msg
    if cid not in ("base_2", "scheme_4", "negative_cells", "cells_2_31"):  # (the restatement refuses the same files)
        with pytest.raises(pr.Refused):
            pr.parse_body(body, cells, nets, pins, base, scheme, np.int32)


def test_capacity_and_pair_refusals(ops):
    rc, msg, outs, _ = _raw_parse(ops, b"1 2\n3 4\n", 4, 2, 4, 1, 0, capacity=3)
    assert rc == 1 and "capacity" in msg
    _untouched(outs, 4, 2, 0)
    t = _text(b"1 2\n")
    hd = ops.handle_for(t.device)
    a = torch.zeros(8, dtype=torch.int32, device=t.device)
    p = C.c_void_p(a.data_ptr())
    counts = (C.c_int64 * 3)()
    rc = hd.lib.sbhg_patoh_parse(hd.h, 0, 0, C.c_void_p(t.data_ptr()), 4, 4, 1, 2, 1, 0, 8, p, p, p, None, None, None, counts)
    assert rc == 1 and "pair" in hd.lib.sbx_last_error(hd.h).decode()
    rc = hd.lib.sbhg_patoh_parse(hd.h, 0, 0, C.c_void_p(t.data_ptr()), 1 << 32, 4, 1, 2, 1, 0, 8, p, p, None, None, None, None,
                                 counts)
    assert rc == 5 and "4 GiB" in hd.lib.sbx_last_error(hd.h).decode()


def test_accepted_edges(ops):
    """What is defined and must not be refused: fewer cell weights (the rest stay 1), a weighted file that ends in '\\n'
    with exactly `nets` lines (cell weights stay 1), weights skipped unparsed without a value type, counts on success."""
    want = _check_parse(ops, b"1 2\n3 4\n7 8", 4, 2, 4, 1, 1, np.float32)
    assert want["cw"].tolist() == [7, 8, 1, 1]
    want = _check_parse(ops, b"1 2\n3 4\n", 4, 2, 4, 1, 1, np.int64)
    assert want["cw"].tolist() == [1, 1, 1, 1] and want["nw"].tolist() == [1, 1]
    _check_parse(ops, b"x.5 1 2\n?? 3 4\n1 2 zz 4", 4, 2, 4, 1, 3, None)
    rc, msg, outs, counts = _raw_parse(ops, b"9 1 2\n8 3 4 1\n% c\n5 6 7", 4, 2, 5, 1, 3)
    assert rc == 0 and counts == [2, 5, 3]
    assert (outs["pin"][5 * 4:] == CANARY).all() and (outs["net"][5 * 4:] == CANARY).all()
    assert (outs["nw"][2 * 4:] == CANARY).all() and (outs["cw"][4 * 4:] == CANARY).all()
    assert (outs["xpin"][3 * 4:] == CANARY).all() and (outs["xnet"][5 * 4:] == CANARY).all()
    assert outs["cw"][:16].view(np.int32).tolist() == [5, 6, 7, 1]


# ------------------------------------------------------------------------------------------- the formatters' protocol
def _g(v, precision=6):
    return ("%.*g" % (precision, float(v))).encode()


VALUE_CASES = [pytest.param(None, None, id="none"), pytest.param(np.int32, None, id="int"),
               pytest.param(np.float32, _g, id="float"), pytest.param(np.float64, _g, id="double")]


def _protocol(ops, call, want):
    """sizing, short capacity (nothing written), the exact capacity (canary behind the length)."""
    hd = ops.handle_for(torch.device("cuda", torch.cuda.current_device()))
    nb = C.c_int64(-1)
    assert call(hd, None, 0, nb) == 0 and nb.value == len(want)
    buf = torch.full((len(want) + 16,), CANARY, dtype=torch.uint8, device="cuda")
    if len(want):
        assert call(hd, C.c_void_p(buf.data_ptr()), len(want) - 1, nb) == 1
        assert "text_out holds" in hd.lib.sbx_last_error(hd.h).decode() and str(len(want)) in hd.lib.sbx_last_error(hd.h).decode()
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == CANARY).all()
    assert call(hd, C.c_void_p(buf.data_ptr()), len(want), nb) == 0 and nb.value == len(want)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert bytes(got[:len(want)]) == want and (got[len(want):] == CANARY).all()


@pytest.mark.parametrize("vdt,vtext", VALUE_CASES)
def test_format_protocol(ops, vdt, vtext):
    g = np.random.default_rng(10)
    nets, cells = 700, 5000
    deg = g.integers(0, 9, nets)
    deg[[0, 350, nets - 1]] = 0
    xpin = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    pin = g.integers(0, cells, xpin[-1]).astype(np.int32)
    nw = None if vdt is None else (g.integers(-999, 99999, nets) / (1 if vdt == np.int32 else 8.0)).astype(vdt)
    if nw is not None and vdt != np.int32:
        nw[:4] = np.array([0.1, 1e-5, 123456.7, 3.0], vdt)
    dx, dp, dw = _dev(xpin), _dev(pin), _dev(nw)
    vt = 0 if vdt is None else ops._VT[_tdt(vdt)]
    for weighted in ((False, True) if vdt is not None else (False,)):
        flags = 1 if weighted else 0
        want = pr.net_lines(xpin, pin, nw if weighted else None, 1, value_text=vtext)
        _protocol(ops, lambda hd, out, cap, nb: hd.lib.sbhg_patoh_format(
            hd.h, 0, vt, 0, nets, C.c_void_p(dx.data_ptr()), C.c_void_p(dp.data_ptr()),
            None if dw is None else C.c_void_p(dw.data_ptr()), 1, 6, flags, out, cap, C.byref(nb)), want)
        # ranges concatenate; SBHG_NO_LAST_NEWLINE drops the range's last '\n' only
        cuts = [0, 1, 200, 351, 699, nets]
        parts = [bytes(ops.patoh_format(dx, dp, dw, a, b, 1, 6, weighted).cpu().numpy()) for a, b in zip(cuts, cuts[1:])]
        assert b"".join(parts) == want
        assert bytes(ops.patoh_format(dx, dp, dw, 0, nets, 1, 6, weighted, last_newline=False).cpu().numpy()) == want[:-1]
        assert bytes(ops.patoh_format(dx, dp, dw, 5, 5, 1, 6, weighted).cpu().numpy()) == b""
    if vdt is not None:
        wantw = pr.weight_line(nw, value_text=vtext)
        _protocol(ops, lambda hd, out, cap, nb: hd.lib.sbhg_patoh_format_weights(
            hd.h, vt, 0, nets, C.c_void_p(dw.data_ptr()), 6, out, cap, C.byref(nb)), wantw)
        cuts = [0, 1, 256, 257, nets]
        parts = [bytes(ops.patoh_format_weights(dw, a, b).cpu().numpy()) for a, b in zip(cuts, cuts[1:])]
        assert b"".join(parts) == wantw and not wantw.endswith(b" ") and b"\n" not in wantw
    assert _bits(dx.cpu().numpy(), xpin) and _bits(dp.cpu().numpy(), pin)  # the inputs are never modified


def test_format_refusals(ops):
    from sparsebase_amd import capi
    xpin, pin = _dev(np.array([0, 2, 3], np.int32)), _dev(np.array([0, 1, 2], np.int32))
    hd = ops.handle_for(xpin.device)
    nb = C.c_int64(0)
    px, pp = C.c_void_p(xpin.data_ptr()), C.c_void_p(pin.data_ptr())
    w = _dev(np.array([1, 2], np.int32))
    pw = C.c_void_p(w.data_ptr())
    fmt = hd.lib.sbhg_patoh_format
    assert fmt(hd.h, 0, capi.V_I32, 0, 2, px, pp, None, 0, 6, capi.HG_NET_WEIGHTS, None, 0, C.byref(nb)) == 1
    assert fmt(hd.h, 0, capi.V_NONE, 0, 2, px, pp, pw, 0, 6, capi.HG_NET_WEIGHTS, None, 0, C.byref(nb)) == 1
    assert "SBHG_NET_WEIGHTS needs values" in hd.lib.sbx_last_error(hd.h).decode()
    assert fmt(hd.h, 0, capi.V_NONE, 0, 2, px, pp, None, 0, 6, 4, None, 0, C.byref(nb)) == 1
    assert "unknown flag" in hd.lib.sbx_last_error(hd.h).decode()
    assert fmt(hd.h, 0, capi.V_NONE, 0, 2, px, pp, None, 0, 6, 0, None, 0, C.byref(nb)) == 0 and nb.value == 6
    bad = _dev(np.array([0, 3, 2], np.int32))
    assert fmt(hd.h, 0, capi.V_NONE, 0, 2, C.c_void_p(bad.data_ptr()), pp, None, 0, 6, 0, None, 0, C.byref(nb)) == 1
    fw = hd.lib.sbhg_patoh_format_weights
    assert fw(hd.h, capi.V_NONE, 0, 2, pw, 6, None, 0, C.byref(nb)) == 1
    assert fw(hd.h, capi.V_I32, 0, 1 << 32, pw, 6, None, 0, C.byref(nb)) == 5
    assert "2^32" in hd.lib.sbx_last_error(hd.h).decode()


# ------------------------------------------------------------------------------------------- format -> parse
@pytest.mark.parametrize("idt,odt", WIDTHS)
@pytest.mark.parametrize("vdt", [None, np.int32, np.float32, np.float64], ids=["none", "int", "float", "double"])
def test_format_then_parse(ops, vdt, idt, odt):
    from sparsebase_amd import patoh
    g = np.random.default_rng(11)
    nets, cells = 900, 333
    deg = g.integers(0, 7, nets)
    deg[[0, 1, 400, nets - 1]] = 0  # empty nets first, in the middle and last
    xpin = np.concatenate([[0], np.cumsum(deg)])
    for base, zero in ((0, True), (0, False), (1, True), (1, False)):
        pin = g.integers(base, cells + base, xpin[-1])
        hg = dict(base=base, cells=cells, constraints=1, xpin=xpin, pin=pin,
                  nw=None if vdt is None else g.integers(1, 9999, nets).astype(vdt),
                  cw=None if vdt is None else g.integers(-99, 9999, cells).astype(vdt))
        for ew, vw in (((False, False), (True, False), (False, True), (True, True)) if vdt is not None else ((False, False),)):
            data = _dev_write(ops, hg, zero, ew, vw, idt, odt, chunk=250)
            assert data == pr.write(hg, zero, ew, vw)
            fbase, fcells, fnets, fpins, scheme, _, off = patoh.parse_header(data)
            assert (fbase, fcells, fnets, fpins, scheme) == (0 if zero else 1, cells, nets, len(pin), ew * 2 + vw)
            delta = fbase - base
            want = dict(xpin=xpin, pin=pin + delta, nw=hg["nw"] if ew else (None if vdt is None else np.ones(nets, vdt)),
                        cw=hg["cw"] if vw else (None if vdt is None else np.ones(cells, vdt)))
            want["xnet"], want["net"] = pr.cells_to_nets(xpin, pin + delta, cells, fbase)
            _check_parse(ops, data[off:], cells, nets, len(pin), fbase, scheme, vdt, idt, odt, want=want)


def test_a_non_integral_weight_prints_and_is_refused(ops):
    from sparsebase_amd import capi
    xpin, pin = _dev(np.array([0, 2, 3], np.int32)), _dev(np.array([0, 1, 2], np.int32))
    body = bytes(ops.patoh_format(xpin, pin, _dev(np.array([3.0, 2.5], np.float32)), net_weights=True).cpu().numpy())
    assert body == b"3 0 1\n2.5 2\n"
    with pytest.raises(capi.SbxError) as e:
        ops.patoh_parse(_text(body), 3, 2, 3, 0, 2, value_dtype=torch.float32)
    assert e.value.status == 1 and "malformed weight token" in str(e.value)


# ------------------------------------------------------------------------------------------- about 1 MB
def test_random_hypergraph_of_a_megabyte(ops):
    g = np.random.default_rng(12)
    nets, cells = 30000, 20011
    deg = g.integers(0, 11, nets)
    xpin = np.concatenate([[0], np.cumsum(deg)])
    pin = g.integers(1, cells + 1, xpin[-1])
    nw, cw = g.integers(1, 99999, nets), g.integers(1, 999, cells)
    body = pr.net_lines(xpin, pin, nw) + pr.weight_line(cw)
    body = body.replace(b"\n", b"\n% a comment 1 2 3\n", 50)
    assert 0.9e6 < len(body) < 1.5e6
    ref = pr.parse_body(body, cells, nets, len(pin), 1, 3, np.int64)  # (once: the restatement walks the text in Python)
    assert _bits(ref["pin"], pin) and _bits(ref["nw"], nw) and _bits(ref["cw"], cw)
    for vdt, idt, odt in ((np.float64, np.int32, np.int32), (np.int32, np.int64, np.int64), (None, np.int32, np.int64)):
        want = dict(ref, nw=None if vdt is None else nw.astype(vdt), cw=None if vdt is None else cw.astype(vdt))
        _check_parse(ops, body, cells, nets, len(pin), 1, 3, vdt, idt, odt, want=want)
