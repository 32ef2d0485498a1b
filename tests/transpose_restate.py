"""numpy restatement of include/sbmt.h.

  plan(rp, col, m)  (col_ptr, row, perm) of an n x m CSR: perm = the stable order of the stored entries by column
                    (np.argsort(col, kind="stable")), row = the row of entry perm[q], col_ptr = the offsets of the columns.
                    Every column must lie in [0, m): the library refuses the others.
  spmm_t_int / spmm_t_wide   Y = A^T X: tests/spmm_restate.py on the m x n matrix (col_ptr, row) with the values val[perm].
                    An entry whose perm[q] lies outside [0, nnz) or whose row[q] lies outside [0, n) is dropped, as the
                    header has it (the row guard is spmm_restate's own column guard; the perm guard is applied here by
                    moving such an entry's row outside [0, n)).
"""
import numpy as np

import spmm_restate as mm


def rows_of(rp, nnz):
    """The row of every stored entry of a well-formed row_ptr."""
    rp = np.asarray(rp, np.int64)
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp)) if nnz else np.zeros(0, np.int64)


def plan(rp, col, m):
    rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int64)
    assert ((col >= 0) & (col < m)).all(), "a column outside [0, m): the library refuses it"
    perm = np.argsort(col, kind="stable").astype(np.int64)
    row = rows_of(rp, len(col))[perm]
    col_ptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=m))]).astype(np.int64)
    return col_ptr, row, perm


def _gathered(n, row, perm, val):
    """(row with the entries of a bad perm moved outside [0, n), val[perm] with 0 there) — or (row, None) for a pattern."""
    row = np.asarray(row, np.int64)
    if val is None:
        return row, None
    perm, val = np.asarray(perm, np.int64), np.asarray(val)
    ok = (perm >= 0) & (perm < len(val))
    w = np.where(ok, val[np.where(ok, perm, 0)], np.zeros(1, val.dtype)) if len(val) else np.zeros(len(perm), val.dtype)
    return np.where(ok, row, -1), w.astype(val.dtype)


def spmm_t_int(n, col_ptr, row, perm, x_flat, k, val=None, ldx=None):
    """The (m, k) product in x's integer dtype, wrapped as spmm_restate.spmm_int wraps."""
    row, w = _gathered(n, row, perm, val)
    return mm.spmm_int(np.asarray(col_ptr, np.int64), row, x_flat, k, w, m=n, ldx=ldx)


def spmm_t_wide(n, col_ptr, row, perm, x_flat, k, val=None, ldx=None, wide=np.float64):
    """(Y, S, u_wide) as spmm_restate.spmm_wide gives them."""
    row, w = _gathered(n, row, perm, val)
    return mm.spmm_wide(np.asarray(col_ptr, np.int64), row, x_flat, k, w, m=n, ldx=ldx, wide=wide)
