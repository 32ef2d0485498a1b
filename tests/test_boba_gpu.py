"""reorder::BOBAReorder on the MI355X (sbx_boba_reorder / ops.boba_reorder / the C++ host layer): the device's inverse
permutation equals the recorded outputs of the real reference and the restatement in test_boba_host.py exactly, for
every index tuple, on messy, hub-heavy, sorted and rectangular inputs, and on a COO of more than 2^31 entries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from sparsebase_amd import capi, ops, synth
from test_boba_host import boba, golden, random_messy_coo
from test_host_layer import built, run  # noqa: F401  (the host programs' fixture and runner)

pytestmark = pytest.mark.gpu

DTYPES = {"i32": torch.int32, "i64": torch.int64}


def _gpu(row, col, n, m, dt="i32"):
    r = torch.as_tensor(np.asarray(row, np.int64)).to(DTYPES[dt]).cuda()
    c = torch.as_tensor(np.asarray(col, np.int64)).to(DTYPES[dt]).cuda()
    return ops.boba_reorder(r, c, n, m).cpu().numpy().astype(np.int64)


def _gpu_i32_n64(row, col, n, m):
    """The SBX_I32_N64 tag (a COO has no offset array: it is SBX_I32 there)."""
    r = torch.as_tensor(np.asarray(row, np.int32)).cuda()
    c = torch.as_tensor(np.asarray(col, np.int32)).cuda()
    inv = torch.empty(max(n, m), dtype=torch.int32, device="cuda")
    hd = ops.handle_for(r.device)
    hd.check(hd.lib.sbx_boba_reorder(hd.h, capi.SBX_I32_N64, n, m, r.numel(), C.c_void_p(r.data_ptr()),
                                     C.c_void_p(c.data_ptr()), C.c_void_p(inv.data_ptr())))
    return inv.cpu().numpy().astype(np.int64)


def test_recorded_reference_outputs():
    for name, row, col, n, m, seq, par in golden():
        for dt in DTYPES:
            assert np.array_equal(_gpu(row, col, n, m, dt), seq), (name, dt)
        assert np.array_equal(_gpu_i32_n64(row, col, n, m), par), name


def test_random_messy_coos():
    g = np.random.default_rng(20261019)
    for trial in range(150):
        n = int(g.integers(1, 300))
        m = int(g.integers(1, 300)) if trial % 3 else n
        row, col = random_messy_coo(g, n, m, int(g.integers(0, 6 * max(n, m))))
        dt = "i32" if trial % 2 else "i64"
        assert np.array_equal(_gpu(row, col, n, m, dt), boba(row, col, n, m)), (trial, n, m)


def test_rectangular_both_ways():
    for n, m, e in [(5000, 300, 40000), (300, 5000, 40000), (1, 7000, 100), (7000, 1, 100)]:
        g = np.random.default_rng(n + m)
        row = g.integers(0, n, e)
        col = g.integers(0, m, e)
        want = boba(row, col, n, m)
        assert len(want) == max(n, m)
        for dt in DTYPES:
            assert np.array_equal(_gpu(row, col, n, m, dt), want), (n, m, dt)


def test_rmat_shuffled_and_sorted():
    # hub-heavy: the shuffled COO puts a hub's entries in every wave; after sbx_coo_sort they come in runs
    rp, col = synth.rmat_symmetric(18, 8, seed=12)
    n = len(rp) - 1
    row = np.repeat(np.arange(n), np.diff(rp)).astype(np.int64)
    col = col.astype(np.int64)
    p = np.random.default_rng(3).permutation(len(row))
    row, col = row[p], col[p]
    want = boba(row, col, n, n)
    for dt in DTYPES:
        r = torch.as_tensor(row).to(DTYPES[dt]).cuda()
        c = torch.as_tensor(col).to(DTYPES[dt]).cuda()
        assert np.array_equal(ops.boba_reorder(r, c, n, n).cpu().numpy(), want), dt
        ops.coo_sort_(n, n, r, c)
        assert bool((r[1:] >= r[:-1]).all())
        assert np.array_equal(ops.boba_reorder(r, c, n, n).cpu().numpy(), want), dt


def test_every_run_gives_the_same_bits():
    g = np.random.default_rng(5)
    row = (2000 * g.random(300000) ** 4).astype(np.int64)  # a few rows hold most entries
    col = g.integers(0, 2000, 300000)
    first = _gpu(row, col, 2000, 2000)
    assert np.array_equal(first, boba(row, col, 2000, 2000))
    for _ in range(3):
        assert np.array_equal(_gpu(row, col, 2000, 2000), first)


def test_bad_arguments():
    for row, col, n, m in [([0, 3], [1, 1], 3, 3), ([0, 1], [1, -1], 3, 3), ([0, 7], [1, 1], 3, 5)]:
        for dt in DTYPES:
            out = torch.full((max(n, m),), -5, dtype=DTYPES[dt], device="cuda")
            r = torch.tensor(row, dtype=DTYPES[dt], device="cuda")
            c = torch.tensor(col, dtype=DTYPES[dt], device="cuda")
            with pytest.raises(capi.SbxError) as e:
                ops.boba_reorder(r, c, n, m, out=out)
            assert e.value.status == 1
            assert out.cpu().tolist() == [-5] * max(n, m)  # nothing written
    # rows in [n, max(n, m)) are accepted, as in the reference
    assert _gpu([4, 1], [0, 2], 3, 5).tolist() == boba([4, 1], [0, 2], 3, 5).tolist()
    r = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(capi.SbxError) as e:
        ops.boba_reorder(r, r, 1 << 31, 1, out=torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert e.value.status == 5
    # no vertices: nothing to write
    z = torch.zeros(0, dtype=torch.int32, device="cuda")
    assert ops.boba_reorder(z, z, 0, 0).numel() == 0
    # the handle still works
    assert _gpu([0, 0, 1, 2], [1, 2, 0, 0], 3, 3).tolist() == [2, 0, 1]


def test_more_than_2_31_entries():
    # an int32 COO of 2^31 + 2^20 entries on rows 5, 17, 900 of a 1000-vertex graph; the minimum columns sit past
    # position 2^31 (rows 17 and 900) and near the start (row 5)
    N = (1 << 31) + (1 << 20)
    row = torch.full((N,), 17, dtype=torch.int32, device="cuda")
    col = torch.full((N,), 700, dtype=torch.int32, device="cuda")
    row[: 1 << 30] = 5
    col[7] = 650
    row[(1 << 31) + 5] = 900
    col[(1 << 31) + 5] = 10
    col[N - 1] = 3
    inv = ops.boba_reorder(row, col, 1000, 1000).cpu().numpy()
    del row, col
    torch.cuda.empty_cache()
    pairs_r = [5, 5, 17, 17, 900]
    pairs_c = [700, 650, 700, 3, 10]
    want = boba(pairs_r, pairs_c, 1000, 1000)
    assert np.array_equal(inv, want)
    assert inv[17] == 0 and inv[900] == 1 and inv[5] == 2 and inv[3] == 3 and inv[10] == 4


def test_host_layer_program(built):
    out = run(os.path.join(built, "test_boba"), attempts=1)
    assert "0 failures" in out and "FAIL" not in out, out
