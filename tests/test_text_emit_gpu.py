"""GPU tests of the emit back end every text formatter shares (sbx_text_emit.h: k_tx_lengths / k_tx_write), once per job:
values, coordinate lines, METIS rows, PaToH nets, PaToH cell weights.  Every job gets 257 items — two workgroups of 256, so
the second one's text starts at an address whose low four bits depend on the first one's total — and writes at text_out + k
for k in {0, 1, 15} between 32 sentinel bytes on either side.  The text is compared with the Python restatements."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metis_restate as mr  # noqa: E402
import patoh_restate as pr  # noqa: E402
import text_restate as tr  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ITEMS = 257
SENTINEL = 0xA5
GUARD = 32
JOBS = ("values", "coordinate", "metis", "patoh_nets", "patoh_weights")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def jobs():
    """name -> (call(hd, out, cap, nb) -> status, the text the restatement gives); the device arrays stay alive in the
    closures."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import capi
    g = np.random.default_rng(257)
    out = {}
    # values: doubles of every length at precision 17
    v = (g.standard_normal(ITEMS) * 10.0 ** g.integers(-9, 10, ITEMS)).astype(np.float64)
    v[:4] = [0.0, 0.5, -1e-5, 123456789.0]
    dv = _dev(v)
    out["values"] = (lambda hd, o, cap, nb: hd.lib.sbx_text_format_values(hd.h, capi.V_F64, ITEMS, _p(dv), 17, o, cap, C.byref(nb)),
                     tr.format_values(v, 17))
    # coordinate lines: 64-bit ids of 1 to 13 digits, float values
    row = (g.integers(0, 10, ITEMS) ** g.integers(1, 14, ITEMS)).astype(np.int64)
    col = (g.integers(0, 10, ITEMS) ** g.integers(1, 14, ITEMS)).astype(np.int64)
    w = (g.standard_normal(ITEMS) * 10.0 ** g.integers(-5, 6, ITEMS)).astype(np.float32)
    dr, dc, dw = _dev(row), _dev(col), _dev(w)
    out["coordinate"] = (lambda hd, o, cap, nb: hd.lib.sbx_text_format_coordinate(
        hd.h, capi.SBX_I64, capi.V_F32, ITEMS, _p(dr), _p(dc), _p(dw), 1, 9, 0, o, cap, C.byref(nb)),
        tr.format_coordinate(row, col, w, 1, 9, 0))
    # METIS: 30 rows with 2 vertex weights each are 90 items, the last '\n' is one, 166 entries (some rows empty)
    n, ncon = 30, 2
    deg = g.multinomial(ITEMS - n * (1 + ncon) - 1, np.ones(n - 4) / (n - 4))
    deg = np.insert(deg, [0, 7, 7, len(deg)], 0)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    assert len(deg) == n and rp[-1] + n * (1 + ncon) + 1 == ITEMS
    mcol = g.integers(0, 100000, rp[-1]).astype(np.int32)
    mval = (g.standard_normal(rp[-1]) * 10.0 ** g.integers(-6, 7, rp[-1])).astype(np.float32)
    mvw = g.random((n, ncon)).astype(np.float32)
    drp, dmc, dmv, dvw = _dev(rp), _dev(mcol), _dev(mval), _dev(mvw)
    out["metis"] = (lambda hd, o, cap, nb: hd.lib.sbgr_metis_format(
        hd.h, capi.SBX_I32, capi.V_F32, 0, n, _p(drp), _p(dmc), _p(dmv), _p(dvw), ncon, 1, 9,
        capi.GR_EDGE_WEIGHTS | capi.GR_VERTEX_WEIGHTS, o, cap, C.byref(nb)),
        mr.format_lines(rp, mcol, mval, mvw, 0, n, 1, 9, True, True))
    # PaToH nets: 50 heads and 207 pins, integer net weights
    nets = 50
    pdeg = g.multinomial(ITEMS - nets, np.ones(nets - 2) / (nets - 2))
    pdeg = np.insert(pdeg, [0, len(pdeg)], 0)
    xpin = np.concatenate([[0], np.cumsum(pdeg)]).astype(np.int32)
    assert xpin[-1] + nets == ITEMS
    pin = (g.integers(0, 10, xpin[-1]) ** g.integers(1, 10, xpin[-1])).astype(np.int32)
    nw = g.integers(-999, 99999, nets).astype(np.int32)
    dx, dp, dnw = _dev(xpin), _dev(pin), _dev(nw)
    out["patoh_nets"] = (lambda hd, o, cap, nb: hd.lib.sbhg_patoh_format(
        hd.h, capi.SBX_I32, capi.V_I32, 0, nets, _p(dx), _p(dp), _p(dnw), 1, 6, 1, o, cap, C.byref(nb)),
        pr.net_lines(xpin, pin, nw, 1))
    # PaToH cell weights: one line of 257 integers
    cw = (g.integers(0, 10, ITEMS) ** g.integers(1, 10, ITEMS)).astype(np.int32)
    dcw = _dev(cw)
    out["patoh_weights"] = (lambda hd, o, cap, nb: hd.lib.sbhg_patoh_format_weights(
        hd.h, capi.V_I32, 0, ITEMS, _p(dcw), 6, o, cap, C.byref(nb)), pr.weight_line(cw))
    return out


@pytest.mark.parametrize("k", [0, 1, 15])
@pytest.mark.parametrize("job", JOBS)
def test_two_workgroups_at_every_alignment(jobs, job, k):
    from sparsebase_amd import ops
    call, want = jobs[job]
    hd = ops.handle_for(torch.device("cuda", torch.cuda.current_device()))
    nb = C.c_int64(-1)
    assert call(hd, None, 0, nb) == 0 and nb.value == len(want), hd.lib.sbx_last_error(hd.h)  # the sizing call
    buf = torch.full((GUARD + k + len(want) + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    nb = C.c_int64(-1)
    assert call(hd, C.c_void_p(buf.data_ptr() + GUARD + k), len(want), nb) == 0 and nb.value == len(want)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[GUARD + k:GUARD + k + len(want)].tobytes() == want
    assert (got[:GUARD + k] == SENTINEL).all() and (got[GUARD + k + len(want):] == SENTINEL).all()
