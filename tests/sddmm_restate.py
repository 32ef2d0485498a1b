"""numpy restatement of sbdd_csr_sddmm (include/sbdd.h): out[p] = val[p] * sum over j < k of U[row(p), j] * V[col[p], j]
for every stored entry p; an entry whose column lies outside [0, m) gets +0 (the column guard); val=None is a pattern
matrix, out[p] the dot itself.  U is an (n, >= k) array and V an (m', >= k) array with m' >= m: the first k columns of
both are used.  The dot is summed first, from +0, and multiplied by val[p] once, so a negative val[p] on a zero dot
gives -0, as the header has it.

  sddmm_int          the integer value types: uint64 arithmetic (numpy wraps it modulo 2^64), wrapped to the width of U
  sddmm_wide         the float value types: (out, S, u_wide) with the dot summed in a wider format (np.float64,
                     np.longdouble) or exactly ("fraction": fractions.Fraction, rounded to np.longdouble), as
                     tests/test_spmv_gpu.py's _wide_for chooses; S[p] = |val[p]| * sum of |U * V|
  int_prefix, wide_prefix   one pass over the columns in blocks returns the dots (and the sums of the absolute products)
                     of the first k columns for every k of a list: one reference per shape serves every k

Everything works through the columns in blocks (an nnz x 16 array of products at a time).
"""
from fractions import Fraction

import numpy as np

import spmv_restate as mv

BLOCK = 16


def rows_of(rp, nnz):
    """The row of every stored entry of a well-formed row_ptr."""
    rp = np.asarray(rp, np.int64)
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp)) if nnz else np.zeros(0, np.int64)


def _prefix(rp, col, U, V, ks, m, cast, absolute):
    """{k: dots of the first k columns} (absolute: the sums of |U V| instead), summed in cast's type block by block; the
    entries outside the column guard are left at 0.  `keep` comes back beside it."""
    m = V.shape[0] if m is None else m
    rp, col, keep = mv._kept(rp, col, m)
    rows, safe = rows_of(rp, len(col)), np.where(keep, col, 0)
    assert max(ks, default=0) <= min(U.shape[1], V.shape[1]), "k beyond the columns of U or V"
    Uw, Vw = cast(U), cast(V)
    acc = np.zeros(len(col), Uw.dtype)
    out, j = {}, 0
    for kk in sorted(set(ks)):
        while j < kk:
            e = min(kk, j + BLOCK)
            if len(col):
                prod = Uw[rows, j:e] * Vw[safe, j:e]
                acc = acc + (np.abs(prod) if absolute else prod).sum(axis=1, dtype=Uw.dtype)
            j = e
        out[kk] = np.where(keep, acc, np.zeros(1, Uw.dtype)).astype(Uw.dtype)
    return out, keep


def _u64(a):
    return np.asarray(a).astype(np.int64).astype(np.uint64)


def _narrow(x, dtype):
    return x.astype(np.uint32).view(np.int32) if dtype == np.int32 else x.view(np.int64)


def int_prefix(rp, col, U, V, ks, m=None):
    """{k: the nnz dots of the first k columns, wrapped to the width of U} for integer U and V."""
    U, V = np.asarray(U), np.asarray(V)
    assert U.dtype in (np.int32, np.int64) and V.dtype == U.dtype
    dots, _ = _prefix(rp, col, U, V, ks, m, _u64, False)
    return {k: _narrow(d, U.dtype) for k, d in dots.items()}


def sddmm_int(rp, col, U, V, k, val=None, m=None):
    U, V = np.asarray(U), np.asarray(V)
    assert U.dtype in (np.int32, np.int64) and V.dtype == U.dtype
    dots, keep = _prefix(rp, col, U, V, [k], m, _u64, False)
    out = dots[k] if val is None else np.where(keep, _u64(val) * dots[k], np.uint64(0)).astype(np.uint64)
    return _narrow(out, U.dtype)


def wide_prefix(rp, col, U, V, ks, m=None, wide=np.float64):
    """{k: (dots, sums of |U V|)} of the first k columns in `wide`, and the unit roundoff of that format."""
    U, V = np.asarray(U), np.asarray(V)
    if isinstance(wide, str):
        assert wide == "fraction"
        return _fraction_prefix(rp, col, U, V, ks, m), float(np.finfo(np.longdouble).eps) / 2
    cast = lambda a: a.astype(wide)
    dots, _ = _prefix(rp, col, U, V, ks, m, cast, False)
    sums, _ = _prefix(rp, col, U, V, ks, m, cast, True)
    return {k: (dots[k], sums[k]) for k in dots}, float(np.finfo(wide).eps) / 2


def _fraction_prefix(rp, col, U, V, ks, m):
    m = V.shape[0] if m is None else m
    rp, col, keep = mv._kept(rp, col, m)
    rows = rows_of(rp, len(col))
    ld = lambda f: np.longdouble(f.numerator) / np.longdouble(f.denominator)
    out = {k: (np.zeros(len(col), np.longdouble), np.zeros(len(col), np.longdouble)) for k in ks}
    for p in range(len(col)):
        if not keep[p]:
            continue
        acc, tot = Fraction(0), Fraction(0)
        for j in range(max(ks, default=0)):
            t = Fraction(float(U[rows[p], j])) * Fraction(float(V[col[p], j]))
            acc, tot = acc + t, tot + abs(t)
            if j + 1 in out:
                out[j + 1][0][p], out[j + 1][1][p] = ld(acc), ld(tot)
    return out


def sddmm_wide(rp, col, U, V, k, val=None, m=None, wide=np.float64):
    """(out, S, u_wide): val * dot with the dot summed in `wide` and the one product done there too; S = |val| * sum |U V|."""
    pre, u_wide = wide_prefix(rp, col, U, V, [k], m, wide)
    dot, tot = pre[k]
    if val is None:
        return dot, tot, u_wide
    w = np.asarray(val).astype(dot.dtype)
    keep = mv._kept(rp, col, np.asarray(V).shape[0] if m is None else m)[2]
    return np.where(keep, w * dot, dot.dtype.type(0)), np.abs(w) * tot, u_wide  # (+0 behind the column guard)
