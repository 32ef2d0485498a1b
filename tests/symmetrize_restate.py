"""A plain Python restatement of include/sbsym.h: B = A ∪ Aᵀ of a square CSR with column-sorted rows.

    row i of B   every stored entry of A's row i verbatim (duplicates, stored order, values), plus one entry with column
                 j for every DISTINCT (j, i) stored in A, j != i, whose mirror (i, j) is not stored; it carries the value
                 of the FIRST stored (j, i); the row is column-sorted
    added        the number of such entries (= missing_mirrors)
    no_diagonal  the stored (i, i) are dropped from B

tests/test_symmetrize_host.py holds it to a dense boolean A | A.T; the GPU tests hold the device to it bit for bit.
"""
import numpy as np


def refusal(n, rp, col):
    """Why include/sbsym.h refuses the input, or None."""
    rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int64)
    if len(col) and (col.min() < 0 or col.max() >= n):
        return "a column lies outside [0, n)"
    for i in range(n):
        if np.any(np.diff(col[rp[i]:rp[i + 1]]) < 0):
            return "the columns of a row decrease"
    return None


def missing_mirrors(n, rp, col):
    return symmetrize(n, rp, col)[3]


def symmetrize(n, rp, col, val=None, no_diagonal=False):
    """(row_ptr_out, col_out, val_out, added) with the dtypes of the inputs."""
    rp_in, col_in = np.asarray(rp), np.asarray(col)
    rp, col = rp_in.astype(np.int64), col_in.astype(np.int64)
    assert refusal(n, rp, col) is None
    first = {}  # (row, column) -> position of its first stored entry
    for j in range(n):
        for p in range(rp[j], rp[j + 1]):
            first.setdefault((j, int(col[p])), p)
    rows = [[(int(col[p]), p) for p in range(rp[i], rp[i + 1]) if not (no_diagonal and col[p] == i)] for i in range(n)]
    added = 0
    for (j, i), p in first.items():
        if j != i and (i, j) not in first:
            rows[i].append((j, p))
            added += 1
    out_rp, src = [0], []
    for r in rows:
        r.sort(key=lambda e: e[0])  # (stable: duplicates keep their stored order; an added column is not a stored one)
        src += [p for _, p in r]
        out_rp.append(len(src))
    src = np.asarray(src, np.int64)
    cols = np.asarray([c for r in rows for c, _ in r], np.int64)
    return (np.asarray(out_rp).astype(rp_in.dtype), cols.astype(col_in.dtype),
            None if val is None else np.asarray(val)[src], added)


def random_csr(g, n, density, dup=0.2, diag=0.3, empty=0.2):
    """A random n x n CSR with sorted rows: duplicates, diagonals and empty rows with the given chances."""
    rp, col = [0], []
    for i in range(n):
        if g.random() >= empty:
            c = list(np.nonzero(g.random(n) < density)[0])
            c = [x for x in c if x != i]
            if g.random() < diag:
                c.append(i)
            c += [x for x in c if g.random() < dup]
            col += sorted(c)
        rp.append(len(col))
    return np.asarray(rp, np.int64), np.asarray(col, np.int64)
