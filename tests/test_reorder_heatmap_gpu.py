"""reorder::ReorderHeatmap on the MI355X (sbx_csr_reorder_heatmap / ops.csr_reorder_heatmap / the C++ host layer): the
device's heatmap equals the recorded outputs of the real reference and the restatement in test_reorder_heatmap_host.py
bit for bit, for every index tuple and FeatureType, on both sides of the LDS / global-counter boundary, and on a
matrix with a cell of more than 2^24 entries."""
import os

import numpy as np
import pytest
import torch

from sparsebase_amd import capi, ops, synth
from test_boba_host import random_messy_coo
from test_host_layer import built, run  # noqa: F401  (the host programs' fixture and runner)
from test_reorder_heatmap_host import (NO_ORDER_TRUE, RC_ORDER_TRUE, C_REORDER, COL3, R_REORDER, RP3, csr_of,
                                       golden_heatmaps, heatmap, orders_for)

pytestmark = pytest.mark.gpu

# index tuples: (row_ptr dtype, id dtype) -> SBX_I32, SBX_I64, SBX_I32_N64
TUPLES = {"i32": (torch.int32, torch.int32), "i64": (torch.int64, torch.int64), "i32_n64": (torch.int64, torch.int32)}


def _t(a, dt):
    return torch.as_tensor(np.asarray(a, np.int64)).to(dt).cuda()


def _gpu(rp, col, orr, orc, b, m, tup="i32", double=False):
    rd, idt = TUPLES[tup]
    out = ops.csr_reorder_heatmap(_t(rp, rd), _t(col, idt), _t(orr, idt), _t(orc, idt), b, m=m, double=double)
    return out.cpu().numpy()


def _same(got, want):
    """Bit-identical, NaNs included (a double output holds the float widened)."""
    want = np.asarray(want, np.float32)
    if got.dtype == np.float64:
        assert np.array_equal(got.astype(np.float32).astype(np.float64), got, equal_nan=True)
        got = got.astype(np.float32)
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _check(rp, col, orr, orc, b, m, tups=tuple(TUPLES)):
    want = heatmap(rp, col, orr, orc, b, m)
    for tup in tups:
        for double in (False, True):
            assert _same(_gpu(rp, col, orr, orc, b, m, tup, double), want), (tup, double, b)


def test_reference_known_answers():
    for tup in TUPLES:
        assert _gpu(RP3, COL3, [0, 1, 2], [0, 1, 2], 3, 3, tup).tolist() == NO_ORDER_TRUE
        assert _gpu(RP3, COL3, R_REORDER, C_REORDER, 3, 3, tup, True).tolist() == RC_ORDER_TRUE


def test_recorded_reference_outputs():
    count = 0
    for name, oname, rp, col, m, orr, orc, b, want in golden_heatmaps():
        for tup in TUPLES:
            for double in (False, True):
                assert _same(_gpu(rp, col, orr, orc, b, m, tup, double), want), (name, oname, b, tup, double)
        count += 1
    assert count >= 150


def test_random_messy_matrices():
    g = np.random.default_rng(20261020)
    for trial in range(120):
        n = int(g.integers(1, 400))
        m = int(g.integers(1, 400))
        row, col = random_messy_coo(g, n, n, int(g.integers(0, 8 * n)))
        rp, col = csr_of(row, col % m, n)
        for oname, orr, orc in orders_for(rp, col, n, m, seed=trial):
            b = int(g.integers(1, min(n, m) + 1))
            _check(rp, col, orr, orc, b, m, tups=(list(TUPLES)[trial % 3],))


@pytest.mark.parametrize("b", [1, 2, 3, 32, 33, 128, 129, 300])
def test_both_sides_of_the_lds_boundary(b):
    # b <= 32: the small LDS grid; b <= 128: the 64 KiB one; b >= 129: 64-bit global counters
    rp, col = synth.rmat_symmetric(13, 8, seed=4)
    n = len(rp) - 1
    g = np.random.default_rng(b)
    for oname, orr, orc in orders_for(rp, col, n, n, seed=b):
        _check(rp, col, orr, orc, b, n)
    orr = g.integers(0, 2 * n, n)  # positions past the last block clamp into it
    _check(rp, col, orr, g.permutation(n), b, n, tups=("i64",))


def test_rectangular_and_rmat_coos():
    rp, col = synth.rmat_symmetric(18, 8, seed=12)
    n = len(rp) - 1
    for oname, orr, orc in orders_for(rp, col, n, n, seed=1):
        for b in (3, 64, 1000):
            _check(rp, col, orr, orc, b, n)
    for n, m in [(5000, 300), (300, 5000)]:
        g = np.random.default_rng(n)
        row = g.integers(0, n, 60000)
        rp, col = csr_of(row, g.integers(0, m, 60000), n)
        for oname, orr, orc in orders_for(rp, col, n, m, seed=2):
            for b in (1, 7, 100, min(n, m)):
                _check(rp, col, orr, orc, b, m)


def test_empty_matrix_is_nan():
    for tup in TUPLES:
        for double in (False, True):
            got = _gpu([0, 0, 0, 0], [], [0, 1, 2], [0, 1], 2, 2, tup, double)
            assert got.shape == (4,) and np.isnan(got).all()


def test_cell_of_more_than_2_24_entries():
    rp_d, col_d = synth.rmat_symmetric_torch(22, seed=1)
    n = rp_d.numel() - 1
    ident = torch.arange(n, dtype=torch.int32, device="cuda")
    got = ops.csr_reorder_heatmap(rp_d, col_d, ident, ident, 3).cpu().numpy()
    rp = rp_d.cpu().numpy().astype(np.int64)
    col = col_d.cpu().numpy().astype(np.int64)
    bsize = n // 3
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cnt = np.bincount(np.minimum(rows // bsize, 2) * 3 + np.minimum(col // bsize, 2), minlength=9)
    assert cnt.max() > (1 << 24)
    want = cnt.astype(np.float32) / np.float32(rp[n])
    assert _same(got, want)
    got64 = ops.csr_reorder_heatmap(rp_d.to(torch.int64), col_d, ident, ident, 3, double=True).cpu().numpy()
    assert _same(got64, want)


def test_bad_arguments():
    rp, col = _t(RP3, torch.int32), _t(COL3, torch.int32)
    ident = _t([0, 1, 2], torch.int32)
    for b in (0, -2, 4):
        with pytest.raises(capi.SbxError) as e:
            ops.csr_reorder_heatmap(rp, col, ident, ident, b)
        assert e.value.status == 1
    with pytest.raises(capi.SbxError) as e:  # b > m
        ops.csr_reorder_heatmap(rp, _t([1, 1, 0, 0], torch.int32), ident, _t([0, 1], torch.int32), 3, m=2)
    assert e.value.status == 1
    with pytest.raises(capi.SbxError) as e:  # a column outside [0, m)
        ops.csr_reorder_heatmap(rp, _t([1, 3, 0, 0], torch.int32), ident, ident, 2)
    assert e.value.status == 1
    with pytest.raises(capi.SbxError) as e:  # a negative column
        ops.csr_reorder_heatmap(rp, _t([1, -1, 0, 0], torch.int32), ident, ident, 2)
    assert e.value.status == 1
    with pytest.raises(capi.SbxError) as e:  # a negative row order entry (row 2, whose entry is there)
        ops.csr_reorder_heatmap(rp, col, _t([0, 1, -1], torch.int32), ident, 2)
    assert e.value.status == 1
    with pytest.raises(capi.SbxError) as e:  # a negative column order entry of a column no entry uses
        ops.csr_reorder_heatmap(_t([0, 1, 2, 2], torch.int64), _t([0, 0], torch.int64), _t([0, 1, 2], torch.int64),
                                _t([0, 1, -7], torch.int64), 2)
    assert e.value.status == 1
    # the handle still works
    assert _gpu(RP3, COL3, [0, 1, 2], [0, 1, 2], 3, 3).tolist() == NO_ORDER_TRUE


def test_every_run_gives_the_same_bits():
    rp, col = synth.rmat_symmetric(16, 8, seed=9)
    n = len(rp) - 1
    g = np.random.default_rng(1)
    orr, orc = g.permutation(n), g.permutation(n)
    first = _gpu(rp, col, orr, orc, 5, n)
    for _ in range(3):
        assert np.array_equal(_gpu(rp, col, orr, orc, 5, n).view(np.uint32), first.view(np.uint32))


def test_host_layer_program(built):
    out = run(os.path.join(built, "test_reorder_heatmap"), attempts=1)
    assert "0 failures" in out and "FAIL" not in out, out
