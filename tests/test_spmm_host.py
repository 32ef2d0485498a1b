"""CPU tests of tests/spmm_restate.py, the restatement tests/test_spmm_gpu.py holds sbmm_csr_spmm to: against a dense
product in Python integers on four small matrices, wrap-around, dropped columns, k = 0 and a leading dimension above k."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmm_restate as mm  # noqa: E402
import spmv_restate as mv  # noqa: E402


def _small(n, m, nnz, k, ldx, seed):
    g = np.random.default_rng(seed)
    r = np.sort(g.integers(0, n, nnz))
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    return np.cumsum(rp), g.integers(0, m, nnz), g.integers(-8, 9, nnz), g.integers(-8, 9, m * ldx)


def _dense(n, m, rp, col, x_flat, k, ldx, val):
    """Y in Python integers through spmv_restate.dense_product, column by column."""
    cols = [mv.dense_product(n, m, rp, col, [int(x_flat[c * ldx + j]) for c in range(m)], val) for j in range(k)]
    return [[cols[j][i] for j in range(k)] for i in range(n)]


@pytest.mark.parametrize("n,m,nnz", [(1, 1, 1), (5, 7, 0), (6, 4, 30), (40, 33, 300)])
@pytest.mark.parametrize("k,ldx", [(1, 1), (3, 3), (3, 8), (5, 6)])
@pytest.mark.parametrize("pattern", [False, True])
def test_integers_against_the_dense_product(n, m, nnz, k, ldx, pattern):
    rp, col, val, x = _small(n, m, nnz, k, ldx, 11 + n + k)
    v = None if pattern else val
    want = _dense(n, m, rp, col, x, k, ldx, v)
    for dt in (np.int32, np.int64):
        got = mm.spmm_int(rp, col, x.astype(dt), k, None if pattern else val.astype(dt), m=m, ldx=ldx)
        assert got.dtype == dt and got.shape == (n, k) and got.tolist() == want
    for dt, wide in ((np.float32, np.float64), (np.float64, np.longdouble), (np.float64, "fraction")):
        Y, S, u = mm.spmm_wide(rp, col, x.astype(dt), k, None if pattern else val.astype(dt), m=m, ldx=ldx, wide=wide)
        assert Y.shape == (n, k) and [[int(t) for t in row] for row in Y] == want
        assert (S >= np.abs(Y)).all() and 0 < u < 2.0 ** -50


def test_wrap_around():
    rp, col = np.array([0, 3, 3, 4]), np.array([0, 1, 1, 2])
    for dt, bits in ((np.int32, 32), (np.int64, 64)):
        big = 2 ** (bits - 1) - 1
        x = np.array([big, 1, big, 2, -5, 3], dt)  # 3 x 2
        val = np.array([2, big, 3, big], dt)
        wrap = lambda t: (t + 2 ** (bits - 1)) % 2 ** bits - 2 ** (bits - 1)
        exact = [[2 * big + big * big + 3 * big, 2 + 2 * big + 6], [0, 0], [-5 * big, 3 * big]]
        assert mm.spmm_int(rp, col, x, 2, val).tolist() == [[wrap(t) for t in row] for row in exact]


def test_columns_outside_the_matrix_are_dropped():
    rp, col = np.array([0, 4, 6]), np.array([0, 3, -1, 2, 4, 1])
    x = np.array([1, 2, 10, 20, 100, 200], np.int64)  # m = 3, k = 2: columns 3, -1 and 4 contribute nothing
    assert mm.spmm_int(rp, col, x, 2).tolist() == [[101, 202], [10, 20]]
    Y, S, _ = mm.spmm_wide(rp, col, x.astype(np.float32), 2, np.array([1, 1, 1, -1, 1, 2], np.float32))
    assert Y.tolist() == [[-99.0, -198.0], [20.0, 40.0]] and S.tolist() == [[101.0, 202.0], [20.0, 40.0]]
    # m below the rows of x: column 2 is dropped too
    assert mm.spmm_int(rp, col, x, 2, m=2).tolist() == [[1, 2], [10, 20]]


def test_k_zero_and_a_leading_dimension_above_k():
    rp, col = np.array([0, 2, 3]), np.array([1, 0, 1])
    assert mm.spmm_int(rp, col, np.zeros(0, np.int32), 0, m=2).shape == (2, 0)
    Y, S, _ = mm.spmm_wide(rp, col, np.zeros(0, np.float32), 0, m=2)
    assert Y.shape == (2, 0) and S.shape == (2, 0)
    flat = np.array([1, 2, -77, -77, 3, 4], np.int32)  # ldx = 4, k = 2: the -77 are padding (the last row has none)
    assert mm.spmm_int(rp, col, flat, 2, m=2, ldx=4).tolist() == [[4, 6], [3, 4]]
    assert mm.block(flat, 2, 2, 4).tolist() == [[1, 2], [3, 4]]
    with pytest.raises(AssertionError):
        mm.block(flat, 2, 2, 1)


def test_every_column_is_the_matrix_vector_restatement():
    """Column j of Y is spmv_restate's product with column j of X: integers, the wide floats and S, with ldx > k, columns
    outside the matrix and more columns than one block of the restatement."""
    k, ldx = mm.BLOCK + 5, mm.BLOCK + 9
    rp, col, val, x = _small(40, 33, 300, k, ldx, 5)
    col[::17] = 33
    col[3] = -1
    X = mm.block(x, 33, k, ldx)
    got = mm.spmm_int(rp, col, x, k, val, m=33, ldx=ldx)
    Y, S, u = mm.spmm_wide(rp, col, x.astype(np.float32), k, val.astype(np.float32), m=33, ldx=ldx)
    for j in range(k):
        assert got[:, j].tolist() == mv.spmv_int(rp, col, X[:, j], val, 33).tolist()
        y1, s1, u1 = mv.spmv_wide(rp, col, X[:, j].astype(np.float32), val.astype(np.float32), 33)
        assert Y[:, j].tolist() == y1.tolist() and S[:, j].tolist() == s1.tolist() and u == u1


def test_a_zero_sum_is_plus_zero():
    Y, _, _ = mm.spmm_wide(np.array([0, 1, 3]), np.array([0, 0, 1]), np.array([-3.0, -1.0, 3.0, 1.0], np.float32), 2,
                           np.array([0.0, 1.0, 1.0], np.float32))
    assert Y.tolist() == [[0.0, 0.0], [0.0, 0.0]] and not np.signbit(Y).any()
