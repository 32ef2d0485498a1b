"""BOBAReorder's rule, checked on the CPU (no GPU): a numpy restatement of the closed form in include/sbx.h
(sbx_boba_reorder), a literal transcription of the reference's two modes (reorder/boba_reorder.cc:33-138), the outputs
recorded from the real reference (tests/golden/boba_heatmap.npz, tools/make_boba_heatmap_golden.py), and the
equalities between the three."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boba_heatmap.npz")


def boba(row, col, n, m):
    """The closed form: vertices with a row entry by (mincol, id), then column-only vertices by id, then the rest."""
    nodes = max(int(n), int(m))
    row = np.asarray(row, np.int64)
    col = np.asarray(col, np.int64)
    big = np.int64(nodes + 2)
    key = np.full(nodes, big, np.int64)
    if len(row):
        o = np.lexsort((col, row))
        r, c = row[o], col[o]
        first = np.ones(len(r), bool)
        first[1:] = r[1:] != r[:-1]
        key[r[first]] = c[first]
    seen = np.zeros(nodes, bool)
    seen[col] = True
    key = np.where(key < big, key, np.where(seen, nodes, nodes + 1))
    order = np.lexsort((np.arange(nodes), key))
    inv = np.empty(nodes, np.int64)
    inv[order] = np.arange(nodes)
    return inv


def reference_boba(row, col, n, m, sequential):
    """boba_reorder.cc:33-135 line by line (the parallel loop run by one thread)."""
    nodes = max(int(n), int(m))
    nnzs = len(row)
    coo = sorted(zip((int(x) for x in row), (int(x) for x in col)), key=lambda p: (p[1], p[0]))
    order = [0] * nodes
    order2 = [0] * nodes
    k = 0
    if sequential:
        copied = set()
        for i in range(nnzs):
            e = coo[i][0]
            if e not in copied:
                order[k] = e
                k += 1
                copied.add(e)
        if k == nodes:
            for i in range(nodes):
                order2[order[i]] = i
            return order2
        for i in range(nnzs):
            e = coo[i][1]
            if e not in copied:
                order[k] = e
                k += 1
                copied.add(e)
        if k == nodes:
            for i in range(nodes):
                order2[order[i]] = i
            return order2
        for i in range(nodes):
            if i not in copied:
                order[k] = i
                k += 1
                copied.add(i)
            order2[order[i]] = i
        return order2
    order = [nnzs * 2] * nodes
    for i in range(nnzs * 2):
        if i < nnzs and i < order[coo[i][0]]:
            order[coo[i][0]] = i
        elif i >= nnzs and i < order[coo[i - nnzs][1]]:
            order[coo[i - nnzs][1]] = i
    pq = sorted((order[i], i) for i in range(nodes))
    for i in range(nodes):
        order2[pq[i][1]] = i
    return order2


def random_messy_coo(g, n, m, e):
    """Unsorted entries with duplicates and self loops; ids anywhere in [0, max(n, m)) (rows in [n, m) included)."""
    nodes = max(n, m)
    if e == 0 or nodes == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    row = g.integers(0, nodes, e)
    col = g.integers(0, nodes, e)
    k = int(g.integers(0, e + 1))
    row[:k] = np.minimum(row[:k], max(n - 1, 0))  # most rows inside [0, n)
    dup = g.integers(0, e, e // 4)
    row = np.concatenate([row, row[dup]])
    col = np.concatenate([col, col[dup]])
    loops = g.integers(0, nodes, e // 8)
    row = np.concatenate([row, loops])
    col = np.concatenate([col, loops])
    p = g.permutation(len(row))
    return row[p], col[p]


def messy_coos():
    """(name, row, col, n, m) of the recorded messy inputs."""
    g = np.random.default_rng(20261018)
    out = [("unsorted_dups", np.array([2, 0, 0, 2, 5, 0, 5, 3, 2]), np.array([5, 3, 1, 2, 1, 3, 5, 3, 0]), 6, 6),
           ("rows_past_n", np.array([4, 1, 6, 1]), np.array([0, 2, 2, 6]), 3, 7),
           ("isolated", np.array([3, 3, 1]), np.array([7, 3, 8]), 10, 10),
           ("empty", np.zeros(0, np.int64), np.zeros(0, np.int64), 4, 6),
           ("tall", np.array([9, 0, 5, 5, 2]), np.array([1, 1, 0, 2, 2]), 10, 3)]
    for i, (n, m, e) in enumerate([(9, 9, 20), (14, 20, 30), (17, 5, 45), (25, 25, 60), (30, 12, 70), (8, 40, 25),
                                   (40, 40, 150)]):
        out.append(("random_%d" % i, *random_messy_coo(g, n, m, e), n, m))
    return out


def golden():
    z = np.load(GOLDEN)
    for name in z["names"].tolist():
        n, m = z[name + "/shape"].tolist()
        yield name, z[name + "/row"], z[name + "/col"], n, m, z[name + "/boba_seq"], z[name + "/boba_par"]


def test_golden_is_small():
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_restatement_and_transcription_equal_the_recorded_reference():
    count = 0
    for name, row, col, n, m, seq, par in golden():
        assert len(seq) == max(n, m) and np.array_equal(np.sort(seq), np.arange(max(n, m))), name
        assert np.array_equal(seq, par), name  # the flag does not change the order
        assert np.array_equal(boba(row, col, n, m), seq), name
        assert reference_boba(row, col, n, m, True) == seq.tolist(), name
        assert reference_boba(row, col, n, m, False) == par.tolist(), name
        count += 1
    assert count >= 14


def test_reference_graph():
    # functionality_common.inc: rows {0, 0, 1, 2}, cols {1, 2, 0, 0}: row 1 and 2 have mincol 0, row 0 mincol 1
    assert boba([0, 0, 1, 2], [1, 2, 0, 0], 3, 3).tolist() == [2, 0, 1]


@pytest.mark.parametrize("seed", range(4))
def test_restatement_equals_transcription_on_random_cases(seed):
    g = np.random.default_rng(100 + seed)
    for trial in range(800):
        n = int(g.integers(0, 25))
        m = int(g.integers(0, 25)) if trial % 3 else n
        e = int(g.integers(0, 3 * max(n, m) + 2)) if max(n, m) else 0
        row, col = random_messy_coo(g, n, m, e)
        want = boba(row, col, n, m)
        assert reference_boba(row, col, n, m, True) == want.tolist(), (n, m, row, col)
        assert reference_boba(row, col, n, m, False) == want.tolist(), (n, m, row, col)


def test_entry_order_does_not_matter():
    g = np.random.default_rng(7)
    row, col = random_messy_coo(g, 50, 80, 300)
    want = boba(row, col, 50, 80)
    for _ in range(5):
        p = g.permutation(len(row))
        assert np.array_equal(boba(row[p], col[p], 50, 80), want)
