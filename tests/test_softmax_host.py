"""CPU tests of tests/softmax_restate.py, the restatement tests/test_softmax_gpu.py holds include/sbsm.h to: against a
loop in Python fractions around np.longdouble's exp on small cases, the table of special values, the pattern form, and
the bounds' own sanity: float32 and float64 numpy evaluations in three different summation orders stay inside them."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softmax_restate as sm  # noqa: E402

SMALL = [(1, 1), (5, 0), (6, 30), (40, 300)]  # (n, nnz)


def _small(n, nnz, seed):
    g = np.random.default_rng(seed)
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, np.sort(g.integers(0, n, nnz)) + 1, 1)
    return np.cumsum(rp), g.normal(0, 4, nnz), g.uniform(-1, 1, nnz)


def _loop_forward(rp, val):
    """A loop over the rows and their entries, exact but for np.longdouble's exp."""
    out = []
    for i in range(len(rp) - 1):
        r = [np.longdouble(x) for x in val[rp[i]:rp[i + 1]]]
        if not r:
            continue
        m = max(r)
        e = [sm._frac(np.exp(x - m)) for x in r]
        out += [x / sum(e) for x in e]
    return out


@pytest.mark.parametrize("n,nnz", SMALL)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_forward_against_the_loop(n, nnz, dt):
    rp, val, _ = _small(n, nnz, 301)
    val = val.astype(dt)
    want = _loop_forward(rp, val)
    wide, frac = sm.softmax_wide(rp, val), sm.softmax_fraction(rp, val)
    assert len(wide) == len(frac) == len(want) == nnz
    for p in range(nnz):
        assert frac[p] == sm._ld(want[p])
        assert abs(sm._frac(wide[p]) - want[p]) <= (int(np.diff(rp).max()) + 2) * Fraction(float(sm.unit(np.longdouble))) * want[p]
    for i in range(n):
        if rp[i + 1] > rp[i]:
            assert sum(want[rp[i]:rp[i + 1]]) == 1


@pytest.mark.parametrize("n,nnz", SMALL)
def test_backward_against_the_loop(n, nnz):
    rp, val, g = _small(n, nnz, 302)
    s = sm.softmax_wide(rp, val.astype(np.float32)).astype(np.float32)
    g = g.astype(np.float32)
    want = []
    for i in range(n):
        d = sum((Fraction(float(s[p])) * Fraction(float(g[p])) for p in range(rp[i], rp[i + 1])), Fraction(0))
        want += [Fraction(float(s[p])) * (Fraction(float(g[p])) - d) for p in range(rp[i], rp[i + 1])]
    ref, S = sm.backward_wide(rp, s, g)
    frac = sm.backward_fraction(rp, s, g)
    bound = sm.backward_bound(rp, S, np.float32)
    for p in range(nnz):
        assert frac[p] == sm._ld(want[p])
        assert abs(ref[p] - frac[p]) <= bound[p]


def test_special_values():
    inf, nan = np.inf, np.nan
    rp = np.array([0, 3, 5, 5, 8, 10, 12, 13])
    val = np.array([1.0, -inf, 1.0,    -inf, -inf,    0.0, nan, 2.0,    inf, 0.0,    3e38, 3e38,    -inf], np.float32)
    ref = sm.softmax_wide(rp, val)
    assert ref[:3].tolist() == [0.5, 0.0, 0.5]          # -inf is the mask value
    assert ref[3:5].tolist() == [0.0, 0.0]              # a row of -inf alone: +0, not NaN
    assert not np.signbit(ref[3:5]).any()
    assert np.isnan(ref[5:8]).all() and np.isnan(ref[8:10]).all()  # a NaN and a +inf poison their rows, and no other
    assert ref[10:12].tolist() == [0.5, 0.5]            # finite values of any magnitude do not overflow
    assert ref[12] == 0.0
    big = sm.softmax_wide([0, 2], np.array([3e38, -3e38], np.float32))
    assert big.tolist() == [1.0, 0.0]
    assert np.isnan(sm.forward_bound(rp, val, ref, np.float32)[5:10]).all()
    assert np.isfinite(sm.forward_bound(rp, val, ref, np.float32)[[0, 1, 2, 3, 4, 10, 11, 12]]).all()


def test_pattern():
    rp = np.array([0, 1, 1, 5, 12])
    ref = sm.softmax_wide(rp, None, nnz=12)
    assert ref[0] == 1 and (ref[1:5] == 0.25).all() and (ref[5:] == np.longdouble(1) / 7).all()
    assert (ref == sm.softmax_wide(rp, np.full(12, 3.5, np.float32))).all()
    with pytest.raises(AssertionError):
        sm.softmax_wide(rp, None, nnz=11)


def test_forward_B():
    rp = np.array([0, 3, 3, 5, 7])
    val = np.array([1.0, 5.0, -np.inf, 2.0, 2.0, -200.0, 100.0], np.float32)
    B = sm.forward_B(rp, val, np.float32)
    assert B[:3].tolist() == [3 + 4 * (4 + sm.EXP_ULPS) + 16] * 3           # T: the finite entries' spread
    assert B[3:5].tolist() == [2 + 4 * sm.EXP_ULPS + 16] * 2
    cap = -np.log(np.longdouble(np.finfo(np.float32).smallest_subnormal))
    assert 103 < cap < 104 and B[5] == 2 + 4 * (cap + sm.EXP_ULPS) + 16       # T saturates at -log(smallest subnormal)
    assert sm.EXP_ULPS == int(np.ceil(2 * max(sm.EXP_MEASURED.values())))


def _softmax_in(dt, rp, val, order):
    """The header's arithmetic in the value type, the row's sum taken in the given order."""
    out = np.zeros(len(val), dt)
    for i in range(len(rp) - 1):
        v = val[rp[i]:rp[i + 1]]
        if len(v) == 0:
            continue
        e = np.exp(v - v.max()).astype(dt)
        s = dt(0)
        for k in order(len(v)):
            s = dt(s + e[k])
        out[rp[i]:rp[i + 1]] = e / s
    return out


def _pairwise(k):
    idx = list(range(k))
    return idx[::2] + idx[1::2]


ORDERS = {"left_to_right": range, "right_to_left": lambda k: range(k - 1, -1, -1), "evens_then_odds": _pairwise}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_bounds_hold_for_plain_evaluations(dt, order):
    """numpy's exp is within EXP_ULPS u as well (it is correctly rounded to well below one unit in the last place)."""
    g = np.random.default_rng(303)
    rp = np.concatenate([[0], np.cumsum(g.integers(0, 400, 40))])
    val = g.normal(0, 4, rp[-1]).astype(dt)
    ref = sm.softmax_wide(rp, val)
    got = _softmax_in(dt, rp, val, ORDERS[order])
    assert (np.abs(got.astype(np.longdouble) - ref) <= sm.forward_bound(rp, val, ref, dt)).all()
    s, gr = got, g.uniform(-1, 1, rp[-1]).astype(dt)
    ref, S = sm.backward_wide(rp, s, gr)
    dz = np.zeros(len(s), dt)
    for i in range(len(rp) - 1):
        d = dt(0)
        for k in ORDERS[order](int(rp[i + 1] - rp[i])):
            d = dt(d + dt(s[rp[i] + k] * gr[rp[i] + k]))
        dz[rp[i]:rp[i + 1]] = s[rp[i]:rp[i + 1]] * (gr[rp[i]:rp[i + 1]] - d)
    assert (np.abs(dz.astype(np.longdouble) - ref) <= sm.backward_bound(rp, S, dt)).all()
    assert (sm.backward_bound(rp, S, dt) < 1e-3 * (np.abs(ref) + 1)).all()  # (and the bound says something)
