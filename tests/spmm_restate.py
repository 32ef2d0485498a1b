"""numpy restatement of sbmm_csr_spmm (include/sbmm.h): Y[i, j] = sum of val[p] * X[col[p], j] over the stored entries of
row i, an entry whose column lies outside [0, m) dropped, val=None a pattern matrix — column j of Y is
tests/spmv_restate.py's product with column j of X (tests/test_spmm_host.py holds it to that).  X is given as the flat
array the library sees and a leading dimension: X[c, j] = x_flat[c * ldx + j], ldx >= k.

  spmm_int    the integer value types: uint64 arithmetic (numpy wraps it modulo 2^64), wrapped to the width of x;
              an (n, k) array of x's dtype
  spmm_wide   the float value types: (Y, S, u_wide) with the sums in a wider format (np.float64, np.longdouble) or exactly
              ("fraction", through spmv_restate column by column), S[i, j] = sum of |val[p]| * |X[col[p], j]|

Both work through the columns in blocks (an nnz x 16 array of products at a time), so a reference of several hundred
columns is computed once and sliced.
"""
import numpy as np

import spmv_restate as mv

BLOCK = 16


def block(x_flat, m, k, ldx=None):
    """The m x k block of a flat array at a leading dimension of ldx elements (default k), as an (m, k) array."""
    ldx = k if ldx is None else ldx
    assert ldx >= k, "a leading dimension below the width"
    x_flat = np.asarray(x_flat)
    assert m == 0 or k == 0 or len(x_flat) >= (m - 1) * ldx + k, "x is shorter than m rows at this leading dimension"
    idx = np.arange(m, dtype=np.int64)[:, None] * ldx + np.arange(k, dtype=np.int64)[None, :]
    return x_flat[idx] if m and k else np.zeros((m, k), x_flat.dtype)


def _rows_of_m(x_flat, k, ldx, m):
    return len(np.asarray(x_flat)) // (k if ldx is None else ldx) if m is None else m


def _row_sums(rp, prod, zero):
    """Every row's sum of the rows of prod (entries x columns), added top to bottom in prod's dtype."""
    y = np.full((len(rp) - 1, prod.shape[1]), zero, prod.dtype)
    nonempty = rp[:-1] < rp[1:]
    if nonempty.any() and prod.shape[1]:
        y[nonempty] = np.add.reduceat(prod, rp[:-1][nonempty], axis=0)
    return y + zero  # (a sum that is exactly zero is +0, as include/sbmm.h has it)


def spmm_int(rp, col, x_flat, k, val=None, m=None, ldx=None):
    """x (and val) int32 or int64: the product wrapped modulo 2^32 or 2^64, an (n, k) array of x's dtype."""
    x_flat = np.asarray(x_flat)
    assert x_flat.dtype in (np.int32, np.int64)
    m = _rows_of_m(x_flat, k, ldx, m)
    rp, col, keep = mv._kept(rp, col, m)
    X = block(x_flat, m, k, ldx).astype(np.int64).astype(np.uint64)
    safe = np.where(keep, col, 0)
    vs = np.ones(len(col), np.uint64) if val is None else np.asarray(val).astype(np.int64).astype(np.uint64)
    vs = np.where(keep, vs, np.uint64(0)).astype(np.uint64)
    out = np.zeros((len(rp) - 1, k), np.uint64)
    for j in range(0, k, BLOCK):
        xs = X[safe, j:j + BLOCK] if len(col) else np.zeros((0, min(BLOCK, k - j)), np.uint64)
        out[:, j:j + BLOCK] = _row_sums(rp, vs[:, None] * xs, np.uint64(0))
    if x_flat.dtype == np.int32:
        return out.astype(np.uint32).view(np.int32)
    return out.view(np.int64)


def spmm_wide(rp, col, x_flat, k, val=None, m=None, ldx=None, wide=np.float64):
    """(Y, S, u_wide): the product summed in `wide`, S = sum |val||x| in `wide`, and the unit roundoff of the sum."""
    x_flat = np.asarray(x_flat)
    m = _rows_of_m(x_flat, k, ldx, m)
    X = block(x_flat, m, k, ldx)
    n = len(rp) - 1
    if isinstance(wide, str):
        Y, S, u = np.zeros((n, k), np.longdouble), np.zeros((n, k), np.longdouble), float(np.finfo(np.longdouble).eps) / 2
        for j in range(k):
            Y[:, j], S[:, j], u = mv.spmv_wide(rp, col, X[:, j], val, m, wide=wide)
        return Y, S, u
    rp, col, keep = mv._kept(rp, col, m)
    safe = np.where(keep, col, 0)
    vs = np.ones(len(col), wide) if val is None else np.asarray(val).astype(wide)
    Y, S = np.zeros((n, k), wide), np.zeros((n, k), wide)
    Xw = X.astype(wide)
    for j in range(0, k, BLOCK):
        xs = Xw[safe, j:j + BLOCK] if len(col) else np.zeros((0, min(BLOCK, k - j)), wide)
        prod = np.where(keep[:, None], vs[:, None] * xs, wide(0)).astype(wide)
        Y[:, j:j + BLOCK] = _row_sums(rp, prod, wide(0))
        S[:, j:j + BLOCK] = _row_sums(rp, np.abs(prod), wide(0))
    return Y, S, float(np.finfo(wide).eps) / 2
