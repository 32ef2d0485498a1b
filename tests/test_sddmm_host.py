"""CPU tests of tests/sddmm_restate.py, the restatement tests/test_sddmm_gpu.py holds sbdd_csr_sddmm to: against a triple
loop in Python integers on small random cases (integers, the wide floats and S, patterns, dropped columns, the prefix
form), wrap-around, -0 and +0, k = 0, and the identity that ties it to tests/spmm_restate.py:

    sum over p of sddmm_int(A; W, X)[p]  ==  sum over i, j of W[i, j] * spmm_int(A, X)[i, j]     (mod 2^64)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sddmm_restate as dd  # noqa: E402
import spmm_restate as mm  # noqa: E402


def _small(n, m, nnz, kmax, seed):
    g = np.random.default_rng(seed)
    r = np.sort(g.integers(0, n, nnz))
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    return (np.cumsum(rp), g.integers(0, m, nnz), g.integers(-8, 9, nnz), g.integers(-8, 9, (n, kmax)),
            g.integers(-8, 9, (m, kmax)))


def _loop(n, m, rp, col, U, V, k, val):
    """(out, S) in Python integers: a loop over the rows, their entries and the columns."""
    out, S = [], []
    for i in range(n):
        for p in range(rp[i], rp[i + 1]):
            inside = 0 <= col[p] < m
            dot = sum(int(U[i, j]) * int(V[col[p], j]) for j in range(k)) if inside else 0
            tot = sum(abs(int(U[i, j]) * int(V[col[p], j])) for j in range(k)) if inside else 0
            w = 1 if val is None else int(val[p])
            out.append(w * dot if inside else 0)
            S.append(abs(w) * tot)
    return out, S


@pytest.mark.parametrize("n,m,nnz", [(1, 1, 1), (5, 7, 0), (6, 4, 30), (40, 33, 300)])
@pytest.mark.parametrize("k", [0, 1, 3, 16, 21])
@pytest.mark.parametrize("pattern", [False, True])
def test_against_the_triple_loop(n, m, nnz, k, pattern):
    rp, col, val, U, V = _small(n, m, nnz, 21, 11 + n + k)
    if nnz > 4:
        col[::7] = m  # the column guard
        col[3] = -1
    v = None if pattern else val
    want, want_S = _loop(n, m, rp, col, U, V, k, v)
    for dt in (np.int32, np.int64):
        got = dd.sddmm_int(rp, col, U.astype(dt), V.astype(dt), k, None if pattern else val.astype(dt), m=m)
        assert got.dtype == dt and got.shape == (nnz,) and got.tolist() == want
    for dt, wide in ((np.float32, np.float64), (np.float64, np.longdouble), (np.float64, "fraction")):
        out, S, u = dd.sddmm_wide(rp, col, U.astype(dt), V.astype(dt), k, None if pattern else val.astype(dt), m=m, wide=wide)
        assert out.shape == (nnz,) and [int(t) for t in out] == want and [int(t) for t in S] == want_S
        assert 0 < u < 2.0 ** -50


def test_the_prefix_form_is_the_single_k_form():
    rp, col, val, U, V = _small(40, 33, 300, 40, 5)
    col[::17] = 33
    ks = [0, 1, 5, 16, 17, 32, 40]
    ints = dd.int_prefix(rp, col, U, V, ks, m=33)
    wides, u = dd.wide_prefix(rp, col, U.astype(np.float32), V.astype(np.float32), ks, m=33)
    assert sorted(ints) == ks and sorted(wides) == ks
    for k in ks:
        assert ints[k].tolist() == dd.sddmm_int(rp, col, U, V, k, m=33).tolist()
        out, S, u1 = dd.sddmm_wide(rp, col, U.astype(np.float32), V.astype(np.float32), k, m=33)
        assert wides[k][0].tolist() == out.tolist() and wides[k][1].tolist() == S.tolist() and u == u1
    # V may hold more rows than the matrix has columns: m below them drops column 32 too
    assert (dd.int_prefix(rp, col, U, V, [40], m=32)[40][col == 32] == 0).all()


def test_wrap_around():
    rp, col = np.array([0, 2, 2, 3]), np.array([0, 1, 1])
    for dt, bits in ((np.int32, 32), (np.int64, 64)):
        big = 2 ** (bits - 1) - 1
        U = np.array([[big, 2], [0, 0], [big, big]], dt)
        V = np.array([[big, 3], [2, big]], dt)
        val = np.array([3, big, 2], dt)
        wrap = lambda t: (t + 2 ** (bits - 1)) % 2 ** bits - 2 ** (bits - 1)
        exact = [3 * (big * big + 6), big * (2 * big + 2 * big), 2 * (2 * big + big * big)]
        assert dd.sddmm_int(rp, col, U, V, 2, val).tolist() == [wrap(t) for t in exact]


def test_signed_zeros_and_k_zero():
    rp, col = np.array([0, 2, 4]), np.array([0, 1, 0, 5])
    U = np.array([[1.0, 1.0], [2.0, 3.0]], np.float32)
    V = np.array([[1.0, -1.0], [0.0, 0.0]], np.float32)
    val = np.array([-2.0, -1.0, -3.0, -4.0], np.float32)
    out, S, _ = dd.sddmm_wide(rp, col, U, V, 2, val, m=2)
    # a cancelled dot and a zero row of V are +0, times a negative value -0; the guarded entry is +0 whatever its value
    assert out.tolist() == [0.0, 0.0, 3.0, 0.0] and np.signbit(out).tolist() == [True, True, False, False]
    assert S.tolist() == [4.0, 0.0, 15.0, 0.0]
    dot, _, _ = dd.sddmm_wide(rp, col, U, V, 2, None, m=2)
    assert dot.tolist() == [0.0, 0.0, -1.0, 0.0] and not np.signbit(dot[dot == 0]).any()
    out0, S0, _ = dd.sddmm_wide(rp, col, U, V, 0, val, m=2)
    assert out0.shape == (4,) and S0.tolist() == [0.0] * 4
    assert dd.sddmm_int(rp, col, U.astype(np.int32), V.astype(np.int32), 0, val.astype(np.int32), m=2).tolist() == [0] * 4


@pytest.mark.parametrize("seed", [3, 4])
def test_the_sum_is_the_inner_product_with_the_spmm(seed):
    """sum_p val[p] (W[row p] . X[col p]) == sum_ij W[i, j] (A X)[i, j] modulo 2^64, on values that wrap."""
    n, m, nnz, k = 40, 33, 300, mm.BLOCK + 5
    rp, col, _, _, _ = _small(n, m, nnz, k, seed)
    col[::17] = m
    g = np.random.default_rng(seed)
    big = lambda size: g.integers(-2 ** 62, 2 ** 62, size)
    val, W, X = big(nnz), big((n, k)), big((m, k))
    u64 = lambda a: np.asarray(a).astype(np.uint64)
    for v in (val, None):
        lhs = u64(dd.sddmm_int(rp, col, W, X, k, v, m=m)).sum(dtype=np.uint64)
        rhs = (u64(W) * u64(mm.spmm_int(rp, col, X.reshape(-1), k, v, m=m))).sum(dtype=np.uint64)
        assert int(lhs) == int(rhs)
