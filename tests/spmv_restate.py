"""numpy restatement of sbmv_csr_spmv (include/sbmv.h): y[i] = sum of val[p] * x[col[p]] over the stored entries of row
i, an entry whose column lies outside [0, m) dropped, val=None a pattern matrix.

  spmv_int    the integer value types: uint64 arithmetic (numpy wraps it modulo 2^64), wrapped to the width of x
  spmv_wide   the float value types: the sum in a wider format (np.float64, np.longdouble) or exactly ("fraction":
              fractions.Fraction, returned rounded to np.longdouble), together with S[i] = sum of |val[p]| * |x[col[p]]|

The bound a float result is held to (tests/test_spmv_gpu.py) is the textbook one for k rounded products summed in any
order, gamma(k, u) * S[i] with gamma(k, u) = k u / (1 - k u): it holds with or without fused multiply-add.
"""
from fractions import Fraction

import numpy as np


def _kept(rp, col, m):
    rp = np.asarray(rp, np.int64)
    col = np.asarray(col, np.int64)
    assert rp[0] == 0 and rp[-1] == len(col) and (np.diff(rp) >= 0).all(), "the restatement takes a well-formed row_ptr"
    return rp, col, (col >= 0) & (col < m)


def _row_sums(rp, prod, zero):
    """Every row's sum of prod, added left to right in prod's dtype; rows without entries are `zero`."""
    n = len(rp) - 1
    y = np.full(n, zero, prod.dtype)
    nonempty = rp[:-1] < rp[1:]
    if nonempty.any():
        y[nonempty] = np.add.reduceat(prod, rp[:-1][nonempty])
    return y + zero  # (a sum that is exactly zero is +0, as include/sbmv.h has it: -0 + +0 = +0)


def spmv_int(rp, col, x, val=None, m=None):
    """x (and val) int32 or int64: the product wrapped modulo 2^32 or 2^64, in x's dtype."""
    x = np.asarray(x)
    assert x.dtype in (np.int32, np.int64)
    m = len(x) if m is None else m
    rp, col, keep = _kept(rp, col, m)
    xs = x.astype(np.int64).astype(np.uint64)[np.where(keep, col, 0)] if len(col) else np.zeros(0, np.uint64)
    vs = np.ones(len(col), np.uint64) if val is None else np.asarray(val).astype(np.int64).astype(np.uint64)
    prod = np.where(keep, vs * xs, np.uint64(0)).astype(np.uint64)
    y = _row_sums(rp, prod, np.uint64(0))
    if x.dtype == np.int32:
        return y.astype(np.uint32).view(np.int32)
    return y.view(np.int64)


def gamma(k, u):
    """k u / (1 - k u), elementwise in np.longdouble."""
    ku = np.asarray(k, np.longdouble) * np.longdouble(u)
    return ku / (1 - ku)


def spmv_wide(rp, col, x, val=None, m=None, wide=np.float64):
    """(y, S, u_wide): the product summed in `wide`, S[i] = sum |val||x| in `wide`, and the unit roundoff of the sum
    ("fraction": the sum is exact and only its final rounding to np.longdouble remains, so np.longdouble's)."""
    x = np.asarray(x)
    m = len(x) if m is None else m
    rp, col, keep = _kept(rp, col, m)
    safe = np.where(keep, col, 0)
    if isinstance(wide, str):
        assert wide == "fraction"
        n = len(rp) - 1
        y, S = np.zeros(n, np.longdouble), np.zeros(n, np.longdouble)
        for i in range(n):
            acc, tot = Fraction(0), Fraction(0)
            for p in range(rp[i], rp[i + 1]):
                if keep[p]:
                    t = Fraction(float(x[col[p]])) * (Fraction(1) if val is None else Fraction(float(val[p])))
                    acc += t
                    tot += abs(t)
            y[i] = np.longdouble(acc.numerator) / np.longdouble(acc.denominator)
            S[i] = np.longdouble(tot.numerator) / np.longdouble(tot.denominator)
        return y, S, float(np.finfo(np.longdouble).eps) / 2
    xs = x.astype(wide)[safe] if len(col) else np.zeros(0, wide)
    vs = np.ones(len(col), wide) if val is None else np.asarray(val).astype(wide)
    prod = np.where(keep, vs * xs, wide(0)).astype(wide)
    return _row_sums(rp, prod, wide(0)), _row_sums(rp, np.abs(prod), wide(0)), float(np.finfo(wide).eps) / 2


def dense_product(n, m, rp, col, x, val=None):
    """The same product through a dense n x m matrix of Python ints (small matrices; integer-valued inputs): exact."""
    A = np.zeros((n, m), object)
    rp = np.asarray(rp, np.int64)
    for i in range(n):
        for p in range(rp[i], rp[i + 1]):
            if 0 <= col[p] < m:
                A[i, col[p]] += 1 if val is None else int(val[p])
    return [sum(int(A[i, j]) * int(x[j]) for j in range(m)) for i in range(n)]
