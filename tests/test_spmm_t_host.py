"""CPU tests of tests/transpose_restate.py, the restatement tests/test_spmm_t_gpu.py holds include/sbmt.h to: the product
against a dense A^T @ X in int64 on small cases (duplicates, unsorted rows, empty rows and columns, a rectangle), the plan
of the plan's transpose giving back a CSR with sorted rows, and the two guards."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transpose_restate as tr  # noqa: E402


def _random_csr(n, m, nnz, seed, sort_rows=False):
    g = np.random.default_rng(seed)
    rows = np.sort(g.integers(0, n, nnz))
    col = g.integers(0, m, nnz)
    if sort_rows:
        col = col[np.lexsort((col, rows))]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return rp, col.astype(np.int64)


def _dense(n, m, rp, col, val):
    a = np.zeros((n, m), np.int64)
    np.add.at(a, (tr.rows_of(rp, len(col)), col), val)  # (duplicates add)
    return a


CASES = [(1, 1, 1), (5, 4, 0), (7, 3, 40), (40, 30, 200), (3, 50, 60), (60, 2, 300)]


@pytest.mark.parametrize("n,m,nnz", CASES)
@pytest.mark.parametrize("k", [1, 3, 17])
@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_product_against_dense(n, m, nnz, k, dt):
    rp, col = _random_csr(n, m, nnz, 300 + n + nnz)
    g = np.random.default_rng(301)
    val, X = g.integers(-8, 9, nnz).astype(dt), g.integers(-8, 9, (n, k)).astype(dt)
    cp, row, perm = tr.plan(rp, col, m)
    assert cp[0] == 0 and cp[-1] == nnz and (np.diff(cp) >= 0).all() and sorted(perm.tolist()) == list(range(nnz))
    for c in range(m):
        q = slice(cp[c], cp[c + 1])
        assert (col[perm[q]] == c).all() and (np.diff(perm[q]) > 0).all() and (np.diff(row[q]) >= 0).all()
    got = tr.spmm_t_int(n, cp, row, perm, X.reshape(-1), k, val)
    assert got.dtype == dt and np.array_equal(got, (_dense(n, m, rp, col, val).T @ X.astype(np.int64)).astype(dt))
    pat = tr.spmm_t_int(n, cp, row, None, X.reshape(-1), k, None)
    assert np.array_equal(pat, (_dense(n, m, rp, col, np.ones(nnz, np.int64)).T @ X.astype(np.int64)).astype(dt))
    wide = tr.spmm_t_wide(n, cp, row, perm, X.astype(np.float32).reshape(-1), k, val.astype(np.float32))[0]
    assert np.array_equal(wide, got.astype(np.float64))


@pytest.mark.parametrize("n,m,nnz", CASES)
def test_plan_of_the_plan_gives_back_a_sorted_csr(n, m, nnz):
    rp, col = _random_csr(n, m, nnz, 400 + n + nnz, sort_rows=True)
    cp, row, perm = tr.plan(rp, col, m)
    rp2, col2, perm2 = tr.plan(cp, row, n)
    assert np.array_equal(rp2, rp) and np.array_equal(col2, col)
    assert np.array_equal(perm[perm2], np.arange(nnz))  # (the two orders are inverse to each other)


def test_the_guards_drop_entries():
    n, m, nnz, k = 40, 30, 200, 5
    rp, col = _random_csr(n, m, nnz, 500)
    g = np.random.default_rng(501)
    val, X = g.integers(-8, 9, nnz), g.integers(-8, 9, (n, k))
    cp, row, perm = tr.plan(rp, col, m)
    bad_p, bad_r = g.choice(nnz, 30, replace=False), g.choice(nnz, 30, replace=False)
    perm2, row2 = perm.copy(), row.copy()
    perm2[bad_p] = np.array([nnz, nnz + 1, -1])[g.integers(0, 3, 30)]
    row2[bad_r] = np.array([n, -1])[g.integers(0, 2, 30)]
    keep = np.ones(nnz, bool)
    keep[bad_p] = keep[bad_r] = False
    a = np.zeros((m, n), np.int64)
    cols_of = np.repeat(np.arange(m), np.diff(cp))
    np.add.at(a, (cols_of[keep], row[keep]), val[perm[keep]])
    assert np.array_equal(tr.spmm_t_int(n, cp, row2, perm2, X.reshape(-1), k, val), a @ X)
    with pytest.raises(AssertionError):
        tr.plan(rp, np.where(np.arange(nnz) == 3, m, col), m)
