"""CPU tests of tests/spmv_restate.py, the restatement tests/test_spmv_gpu.py holds sbmv_csr_spmv to: against a dense
product in Python integers on a few small matrices, wrap-around, dropped columns and the float side included."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmv_restate as mv  # noqa: E402


def _small(n, m, nnz, seed):
    g = np.random.default_rng(seed)
    r = np.sort(g.integers(0, n, nnz))
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    return np.cumsum(rp), g.integers(0, m, nnz), g.integers(-8, 9, nnz), g.integers(-8, 9, m)


@pytest.mark.parametrize("n,m,nnz", [(1, 1, 1), (5, 7, 0), (6, 4, 30), (40, 33, 300)])
@pytest.mark.parametrize("pattern", [False, True])
def test_integers_against_the_dense_product(n, m, nnz, pattern):
    rp, col, val, x = _small(n, m, nnz, 7 + n)
    v = None if pattern else val
    want = mv.dense_product(n, m, rp, col, x, v)
    for dt in (np.int32, np.int64):
        got = mv.spmv_int(rp, col, x.astype(dt), None if pattern else val.astype(dt))
        assert got.dtype == dt and got.tolist() == want
    for dt, wide in ((np.float32, np.float64), (np.float64, np.longdouble)):
        y, S, u = mv.spmv_wide(rp, col, x.astype(dt), None if pattern else val.astype(dt), wide=wide)
        assert y.dtype == wide and [int(t) for t in y] == want and (S >= np.abs(y)).all() and 0 < u < 2.0 ** -50
    y, S, _ = mv.spmv_wide(rp, col, x.astype(np.float64), None if pattern else val.astype(np.float64), wide="fraction")
    assert [int(t) for t in y] == want


def test_wrap_around():
    rp, col = np.array([0, 3, 3, 4]), np.array([0, 1, 1, 2])
    big32, big64 = 2 ** 31 - 1, 2 ** 63 - 1
    for dt, big, bits in ((np.int32, big32, 32), (np.int64, big64, 64)):
        x = np.array([big, big, -5], dt)
        val = np.array([2, big, 3, big], dt)
        exact = [2 * big + big * big + 3 * big, 0, -5 * big]
        wrap = lambda t: (t + 2 ** (bits - 1)) % 2 ** bits - 2 ** (bits - 1)
        assert mv.spmv_int(rp, col, x, val).tolist() == [wrap(t) for t in exact]
        assert mv.spmv_int(rp, col, x).tolist() == [wrap(3 * big), 0, -5]


def test_columns_outside_the_matrix_are_dropped():
    rp, col = np.array([0, 4, 6]), np.array([0, 3, -1, 2, 4, 1])
    x = np.array([1, 10, 100], np.int64)  # m = 3: columns 3, -1 and 4 contribute nothing
    assert mv.spmv_int(rp, col, x).tolist() == [101, 10]
    y, S, _ = mv.spmv_wide(rp, col, x.astype(np.float32), np.array([1, 1, 1, -1, 1, 2], np.float32))
    assert y.tolist() == [-99.0, 20.0] and S.tolist() == [101.0, 20.0]
    assert mv.spmv_int(rp, col, np.arange(1, 6), m=4).tolist() == [1 + 4 + 3, 2]  # m below len(x): column 4 dropped too


def test_a_zero_sum_is_plus_zero():
    y, _, _ = mv.spmv_wide(np.array([0, 1, 3]), np.array([0, 0, 1]), np.array([-3.0, 3.0], np.float32),
                           np.array([0.0, 1.0, 1.0], np.float32))
    assert y.tolist() == [0.0, 0.0] and not np.signbit(y).any()


def test_gamma():
    g = mv.gamma(np.array([1, 1000]), 2.0 ** -24)
    assert abs(float(g[0]) - 2.0 ** -24) < 2.0 ** -47 and float(g[1]) > 1000 * 2.0 ** -24
