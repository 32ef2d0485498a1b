"""The numpy restatement of include/sbsm.h: the softmax over the stored values of every row of a CSR matrix and its
backward, in np.longdouble (and, for small cases, in exact fractions around an exp taken in np.longdouble), the special
values of the header, and the two error bounds the GPU tests hold the kernels to.  Nothing here is ported: the reference
has no such operation.

The forward bound.  With u the unit roundoff of the value type, len_i the stored entries of row i, m_i its maximum and
T_i = min(max over the row's finite entries of (m_i - val[q]), -log(smallest subnormal of the type)):

    |out[p] - ref[p]| <= B_i u ref[p] + tiny(dt),      B_i = len_i + 4 (T_i + EXP_ULPS) + 16

Where it comes from, for e[p] = exp(val[p] - m_i) and s_i = sum e[q]:
  - the rounded difference t = val[p] - m_i carries a relative error u, that is u |t| <= u T_i in the exponent, so a
    relative error u T_i in e[p] (to first order; an entry with |t| beyond T_i has an e below the smallest subnormal and
    is covered by tiny);
  - exp itself is within EXP_ULPS u of the exact exponential of its argument;
  - s_i takes len_i - 1 additions of non-negative terms: a relative error of at most (len_i - 1) u on top of the terms' own
    (T_i + EXP_ULPS) u;
  - where the row crosses spans, a span's partial sum is rescaled once by exp(m_t - m_i): one more difference, one more
    exp and one product, (T_i + EXP_ULPS + 1) u;
  - one division, u.
Numerator and denominator together: len_i + 3 (T_i + EXP_ULPS) and a few units.  B_i leaves one more (T_i + EXP_ULPS)
and a dozen units for the second-order terms, and no more.  tiny(dt), the smallest normal number, absorbs the entries
whose e is subnormal (their relative error is not bounded by u).

EXP_ULPS is measured, not assumed: a row {0, t} with t in [-87, -17.4] (f32; [-708, -37.5] for f64, which the library
does not build yet) has s_i = 1 exactly (1 + e rounds to 1), so its second output is the device's exp(t) bit for bit.
Over 2^16 such t, against
np.longdouble's exp, in units of u relative to the result (an error of one unit in the last place is between 1 and 2 of
these units), the largest error measured on an MI355X on 2026-10-21 was EXP_MEASURED below.  EXP_ULPS is twice that,
rounded up to an integer: the arguments of the other tests are not the probed ones.  test_exp_ulps re-measures and
asserts measured <= EXP_ULPS / 2.

The backward bound.  dz[p] = s[p] (g[p] - d_i), d_i a dot of len_i products in any order, with or without fused
multiply-add (gamma(len_i, u) sum |s g|), then one subtraction and one product:

    |dz[p] - ref[p]| <= gamma(len_i + 4, u) |s[p]| (|g[p]| + sum_q |s[q] g[q]|)   plus the same at the wide type's u.
"""
from fractions import Fraction

import numpy as np

from spmv_restate import gamma

EXP_MEASURED = {"f32": 1.3482}  # the largest |exp_device(t) - exp(t)| / (u exp(t)) over the probe, per type
EXP_ULPS = 3                             # twice the larger of them, rounded up


def unit(dt):
    return np.longdouble(np.finfo(dt).eps) / 2


def tiny(dt):
    return np.longdouble(np.finfo(dt).tiny)


def _rows(rp):
    rp = np.asarray(rp, np.int64)
    return [(int(rp[i]), int(rp[i + 1])) for i in range(len(rp) - 1)]


def _frac(x):
    """The np.longdouble x as an exact fraction (float() would drop its last 11 bits)."""
    mant, ex = np.frexp(np.longdouble(x))
    return Fraction(int(np.ldexp(mant, 64))) * Fraction(2) ** (int(ex) - 64)


def _row_ids(rp):
    rp = np.asarray(rp, np.int64)
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def _ld(q):
    """The fraction q rounded to np.longdouble (through 128 bits of quotient: no overflow of either part)."""
    if q == 0:
        return np.longdouble(0)
    k = 128 + q.denominator.bit_length() - abs(q.numerator).bit_length()
    w = (q.numerator << k) // q.denominator if k >= 0 else q.numerator // (q.denominator << -k)
    return np.ldexp(np.longdouble(w), -k)


def softmax_wide(rp, val, nnz=None):
    """ref (np.longdouble, one per stored entry) under the header's rules.  val=None: a pattern of nnz entries."""
    rp = np.asarray(rp, np.int64)
    n, rows = len(rp) - 1, _row_ids(rp)
    if val is None:
        assert int(nnz) == len(rows)
        return np.longdouble(1) / np.diff(rp).astype(np.longdouble)[rows]
    v = np.asarray(val).astype(np.longdouble)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        poisoned = np.zeros(n, bool)  # exp(NaN) and inf - inf reach the row's sum
        np.logical_or.at(poisoned, rows, np.isnan(v) | np.isposinf(v))
        m = np.full(n, -np.inf, np.longdouble)
        np.maximum.at(m, rows, np.where(np.isnan(v), -np.inf, v))
        e = np.exp(v - np.where(np.isfinite(m), m, 0)[rows])  # (exp(-inf) = 0: a masked entry)
        s = np.zeros(n, np.longdouble)
        np.add.at(s, rows, e)
        ref = np.where(s[rows] > 0, e / np.where(s > 0, s, 1)[rows], 0)  # (a sum of 0: nothing but masked entries, +0)
    ref[poisoned[rows]] = np.nan
    return ref


def softmax_fraction(rp, val):
    """The same, summed and divided exactly: fractions around np.longdouble's exp (finite values and -inf only)."""
    v = np.asarray(val).astype(np.longdouble)
    ref = np.zeros(len(v), np.longdouble)
    for lo, hi in _rows(rp):
        r = v[lo:hi]
        if hi == lo or np.isneginf(r).all():
            continue
        m = r.max()
        e = [Fraction(0) if np.isneginf(x) else _frac(np.exp(x - m)) for x in r]
        s = sum(e)
        for k, x in enumerate(e):
            ref[lo + k] = _ld(x / s)
    return ref


def forward_B(rp, val, dt):
    """B_i of the docstring, one per stored entry (np.longdouble)."""
    rp = np.asarray(rp, np.int64)
    n, rows = len(rp) - 1, _row_ids(rp)
    v = np.asarray(val).astype(np.longdouble)
    fin = np.isfinite(v)
    hi, lo = np.full(n, -np.inf, np.longdouble), np.full(n, np.inf, np.longdouble)
    np.maximum.at(hi, rows[fin], v[fin])
    np.minimum.at(lo, rows[fin], v[fin])
    cap = -np.log(np.longdouble(np.finfo(dt).smallest_subnormal))
    T = np.where(np.isfinite(hi), np.minimum(hi - np.where(np.isfinite(lo), lo, 0), cap), 0)
    return (np.diff(rp) + 4 * (T + EXP_ULPS) + 16)[rows]


def forward_bound(rp, val, ref, dt):
    """The largest |out - ref| the header's arithmetic allows, per stored entry; NaN where ref is NaN."""
    return forward_B(rp, val, dt) * unit(dt) * np.abs(ref) + tiny(dt)


def backward_wide(rp, s, g):
    """(ref, S): dz in np.longdouble and S[p] = |s[p]| (|g[p]| + sum over the row of |s g|)."""
    rp = np.asarray(rp, np.int64)
    n, rows = len(rp) - 1, _row_ids(rp)
    s, g = np.asarray(s).astype(np.longdouble), np.asarray(g).astype(np.longdouble)
    d, a = np.zeros(n, np.longdouble), np.zeros(n, np.longdouble)
    np.add.at(d, rows, s * g)
    np.add.at(a, rows, np.abs(s * g))
    return s * (g - d[rows]), np.abs(s) * (np.abs(g) + a[rows])


def backward_fraction(rp, s, g):
    """dz with the dot, the subtraction and the product exact (small cases)."""
    ref = np.zeros(len(s), np.longdouble)
    fs, fg = [_frac(x) for x in s], [_frac(x) for x in g]
    for lo, hi in _rows(rp):
        d = sum((fs[p] * fg[p] for p in range(lo, hi)), Fraction(0))
        for p in range(lo, hi):
            ref[p] = _ld(fs[p] * (fg[p] - d))
    return ref


def backward_bound(rp, S, dt):
    """gamma(len_i + 4, u) S plus the same at np.longdouble's u, per stored entry."""
    length = np.repeat(np.diff(np.asarray(rp, np.int64)), np.diff(np.asarray(rp, np.int64)))
    return (gamma(length + 4, unit(dt)) + gamma(length + 4, unit(np.longdouble))) * S
