"""tests/symmetrize_restate.py, the Python restatement of include/sbsym.h, against a dense boolean A | A.T on 2 000
random small cases (CPU): duplicates, diagonals, empty rows, n = 0 and n = 1."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symmetrize_restate as sr  # noqa: E402


def _check(n, rp, col, no_diagonal):
    val = np.arange(len(col), dtype=np.int64) * 7 + 3  # (every stored entry tells its position)
    rpo, co, vo, added = sr.symmetrize(n, rp, col, val, no_diagonal)
    A = np.zeros((n, n), bool)
    rows = np.repeat(np.arange(n), np.diff(rp))
    A[rows, col] = True
    want = A | A.T
    assert added == int((want & ~A).sum()) == sr.missing_mirrors(n, rp, col)
    if no_diagonal:
        want[np.arange(n), np.arange(n)] = False
    assert rpo[0] == 0 and len(rpo) == n + 1 and rpo[-1] == len(co) == len(vo)
    ndiag = int((rows == col).sum())
    assert len(co) == len(col) + added - (ndiag if no_diagonal else 0)
    B = np.zeros((n, n), bool)
    for i in range(n):
        c, v = co[rpo[i]:rpo[i + 1]], vo[rpo[i]:rpo[i + 1]]
        assert np.all(np.diff(c) >= 0)
        B[i, c] = True
        src = (v - 3) // 7  # where every entry of B came from
        own = rows[src] == i
        keep = (col[rp[i]:rp[i + 1]] != i) if no_diagonal else np.ones(rp[i + 1] - rp[i], bool)
        assert np.array_equal(src[own & (col[src] == c)], np.arange(rp[i], rp[i + 1])[keep])  # verbatim, stored order
        for cc, s in zip(c[~own], src[~own]):  # an added entry: the FIRST stored (cc, i)
            assert col[s] == i and rows[s] == cc and s == rp[cc] + np.searchsorted(col[rp[cc]:rp[cc + 1]], i)
        assert len(set(c[~own])) == len(c[~own]) and not A[i, c[~own]].any()
    assert np.array_equal(B, want)


def test_restatement_against_dense_or():
    g = np.random.default_rng(2024)
    count = 0
    for n in (0, 1):
        for diag in (0.0, 1.0):
            rp, col = sr.random_csr(g, n, 0.5, diag=diag, empty=0.0)
            for nd in (False, True):
                _check(n, rp, col, nd)
                count += 1
    while count < 2000:
        n = int(g.integers(0, 9))
        rp, col = sr.random_csr(g, n, g.choice([0.1, 0.3, 0.6]))
        _check(n, rp, col, bool(count & 1))
        count += 1


def test_duplicates_add_one_entry_with_the_first_value():
    # row 0 stores (0, 2) three times; row 2 stores nothing: one (2, 0) is added, with the first value
    rp, col, val = np.array([0, 3, 3, 3]), np.array([2, 2, 2]), np.array([10.0, 20.0, 30.0])
    rpo, co, vo, added = sr.symmetrize(3, rp, col, val)
    assert added == 1 and rpo.tolist() == [0, 3, 3, 4] and co.tolist() == [2, 2, 2, 0] and vo.tolist() == [10, 20, 30, 10]


def test_refusals():
    assert sr.refusal(2, [0, 1, 1], [2]) and sr.refusal(2, [0, 2, 2], [1, 0]) and sr.refusal(2, [0, 2, 2], [0, 0]) is None
