"""feature::TriangleCount without a GPU: vectorised restatements of both modes of sbx_csr_triangle_count, written from
the rules in include/sbx.h, which every GPU test checks against; the reference mode's restatement checked against a
plain per-vertex marker scan, the exact mode's against known counts.

Reference mode (the reference's value, feature/triangle_count.cc:142-223; entries counted with multiplicity):
  undirected  first[w] = the smallest row u >= 1 holding an entry with column w (+inf if none); count the entry pairs
              ((node, v) in row node, (v, w) in row v) with node < v < w and first[w] <= node.
  directed    first[w] = the smallest column >= 1 among the entries of row w (+inf if none); count the entry pairs
              ((node, v), (v, w)) with node < v, node < w and first[w] <= node.
Exact mode: the triangles of the simple undirected graph of the entries off the diagonal, or the directed 3-cycles of
the simple digraph.  A column outside [0, n) is a vertex with no entries that is never marked.
"""
import os
import re
from math import comb

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHUNK = 1 << 22  # list entries expanded at a time in the exact restatement

# the reference test's graphs (tests/suites/sparsebase/feature/triangle_count_tests.cc), n = 10
DIR_RP = [0, 0, 1, 2, 3, 4, 5, 6, 8, 10, 12]
DIR_COL = [2, 3, 1, 6, 4, 5, 8, 9, 7, 9, 7, 8]
UND_RP = [0, 0, 2, 4, 6, 8, 10, 12, 13, 15, 16]
UND_COL = [2, 3, 1, 3, 1, 2, 5, 6, 4, 6, 4, 5, 8, 7, 9, 8]


def csr_from_pairs(n, src, dst):
    """CSR of the entries (src[i], dst[i]) in the given order inside each row (stable), duplicates kept."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    o = np.argsort(src, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, src + 1, 1)
    return np.cumsum(rp), dst[o]


def undirected(n, edges):
    s = [a for a, b in edges] + [b for a, b in edges]
    d = [b for a, b in edges] + [a for a, b in edges]
    return csr_from_pairs(n, s, d)


def directed(n, arcs):
    return csr_from_pairs(n, [a for a, b in arcs], [b for a, b in arcs])


# (name, n, rp/col builder, directed, reference value, exact value): the table of the issue this feature answers
def table():
    return [
        ("reference undirected graph", UND_RP, UND_COL, False, 2, 2),
        ("reference directed graph", DIR_RP, DIR_COL, True, 4, 4),
        ("4-cycle 1-2-3-4, vertex 0 isolated", *undirected(5, [(1, 2), (2, 3), (3, 4), (4, 1)]), False, 1, 0),
        ("triangle 0-1-2", *undirected(3, [(0, 1), (1, 2), (2, 0)]), False, 0, 1),
        ("directed cycle 0->1->2->0", *directed(3, [(0, 1), (1, 2), (2, 0)]), True, 0, 1),
    ]


def _parts(rp, col):
    rp = np.asarray(rp, np.int64)
    col = np.asarray(col, np.int64)
    n = len(rp) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    return rp, col, n, row


def _count_le(keys, base, row, x):
    """Per query: the keys of `row` (keys are row * base + value, sorted) whose value is <= x."""
    return np.searchsorted(keys, row * base + x, side="right") - np.searchsorted(keys, row * base, side="left")


def tc_reference(rp, col, directed=False):
    rp, col, n, row = _parts(rp, col)
    if n == 0 or len(col) == 0:
        return 0
    inf = n  # larger than every node
    ok = (col >= 0) & (col < n)
    first = np.full(n, inf, np.int64)
    if directed:
        m = ok & (col >= 1)
        np.minimum.at(first, row[m], col[m])
    else:
        m = ok & (row >= 1)
        np.minimum.at(first, col[m], row[m])
    base = n + 1
    fw = np.full(len(col), inf, np.int64)
    fw[ok] = first[col[ok]]
    q = ok & (col > row)  # queries (node, v): node < v < n
    node, v = row[q], col[q]
    if directed:
        has = fw < inf
        ka = np.sort(row[has] * base + fw[has])
        kb = np.sort(row[has] * base + np.maximum(fw[has], col[has]))
        return int((_count_le(ka, base, v, node) - _count_le(kb, base, v, node)).sum())
    has = (fw < inf) & (col > row)
    ka = np.sort(row[has] * base + fw[has])
    return int(_count_le(ka, base, v, node).sum())


def marker_scan(rp, col, directed=False):
    """The rule as a plain per-vertex scan: marks hold the id of the last vertex that set them and are never cleared,
    so a mark set by vertex 0 reads as unset.  Undirected: vertex `node` marks the columns of its row; directed: it
    marks the rows that hold an entry with column `node`.  Then every entry (node, v) with node < v counts the
    entries (v, w) of row v with w > v (directed: w > node) whose mark is set."""
    rp, col, n, row = _parts(rp, col)
    into = [[] for _ in range(n)]
    if directed:
        for r, c in zip(row.tolist(), col.tolist()):
            if 0 <= c < n:
                into[c].append(r)
    mark = [0] * n
    rpl, coll = rp.tolist(), col.tolist()
    total = 0
    for node in range(n):
        for w in (into[node] if directed else coll[rpl[node]:rpl[node + 1]]):
            if 0 <= w < n:
                mark[w] = node
        for v in coll[rpl[node]:rpl[node + 1]]:
            if node < v < n:
                low = node if directed else v
                for w in coll[rpl[v]:rpl[v + 1]]:
                    if low < w < n and mark[w] != 0:
                        total += 1
    return total


def _simple(n, a, b):
    """Sorted duplicate-free arcs a -> b (keys a * n + b) of the entries off the diagonal inside [0, n)."""
    ok = (a >= 0) & (a < n) & (b >= 0) & (b < n) & (a != b)
    return np.unique(a[ok] * n + b[ok])


def _lists(n, keys):
    """CSR of sorted keys: offsets per row, and the values."""
    src, dst = keys // n, keys % n
    off = np.searchsorted(src, np.arange(n + 1))
    return off, dst


def _probe(start, ln, vals, keys, key_of):
    """Sum over items i of #{x in vals[start[i] : start[i] + ln[i]] with key_of(i, x) in keys}."""
    ends = np.cumsum(ln)
    total, lo = 0, 0
    while lo < len(ln):
        hi = max(lo + 1, int(np.searchsorted(ends, (ends[lo - 1] if lo else 0) + _CHUNK, side="right")))
        d = ln[lo:hi]
        pid = np.repeat(np.arange(lo, hi), d)
        x = vals[start[pid] + np.arange(int(d.sum())) - np.repeat(np.cumsum(d) - d, d)]
        k = key_of(pid, x)
        i = np.searchsorted(keys, k)
        total += int((keys[np.minimum(i, len(keys) - 1)] == k).sum())
        lo = hi
    return total


def tc_exact(rp, col, directed=False):
    rp, col, n, row = _parts(rp, col)
    if n < 3 or len(col) == 0:
        return 0
    if directed:
        arcs = _simple(n, row, col)
        if len(arcs) == 0:
            return 0
        out_off, out_v = _lists(n, arcs)
        rev = np.sort((arcs % n) * n + arcs // n)  # c -> a as a * n + c: in-lists
        in_off, in_v = _lists(n, rev)
        a, b = arcs // n, arcs % n
        fw = a < b
        a, b = a[fw], b[fw]
        # per arc a -> b, a < b: c > a with b -> c and c -> a.  Both lists cut to the values > a; the shorter expanded
        os_ = np.searchsorted(arcs, b * n + a + 1)
        ol = out_off[b + 1] - os_
        is_ = np.searchsorted(rev, a * n + a + 1)
        il = in_off[a + 1] - is_
        s1 = ol <= il
        s2 = ~s1
        a1, a2, b2 = a[s1], a[s2], b[s2]
        return (_probe(os_[s1], ol[s1], out_v, arcs, lambda i, c: c * n + a1[i]) +
                _probe(is_[s2], il[s2], in_v, arcs, lambda i, c: b2[i] * n + c))
    sym = _simple(n, np.concatenate([row, col]), np.concatenate([col, row]))
    if len(sym) == 0:
        return 0
    u, v = sym // n, sym % n
    deg = np.bincount(u, minlength=n)
    keep = (deg[u] < deg[v]) | ((deg[u] == deg[v]) & (u < v))
    ori = sym[keep]
    off, vals = _lists(n, ori)
    u, v = ori // n, ori % n
    # per oriented edge (u, v): w in N+(u) with v -> w oriented
    return _probe(off[u], off[u + 1] - off[u], vals, ori, lambda i, w: v[i] * n + w)


def dense_trace(rp, col):
    """trace(A^3) / 6 of the simple undirected graph: its triangles."""
    rp, col, n, row = _parts(rp, col)
    A = np.zeros((n, n), np.int64)
    ok = (col >= 0) & (col < n) & (col != row)
    A[row[ok], col[ok]] = 1
    A[col[ok], row[ok]] = 1
    return int(np.trace(A @ A @ A)) // 6


def dense_cycles(rp, col):
    """Directed 3-cycles of the simple digraph: trace(A^3) / 3."""
    rp, col, n, row = _parts(rp, col)
    A = np.zeros((n, n), np.int64)
    ok = (col >= 0) & (col < n) & (col != row)
    A[row[ok], col[ok]] = 1
    return int(np.trace(A @ A @ A)) // 3


def random_messy_graph(g, n, e, symmetric, hub0=False, oob=False):
    """Entries with duplicates, self loops, unsorted rows; symmetric or not; optionally vertex 0 as a hub and
    columns outside [0, n)."""
    src = g.integers(0, n, e)
    dst = g.integers(0, n, e)
    if hub0:
        k = e // 3
        dst[:k] = 0
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    dup = g.integers(0, len(src), len(src) // 5 + 1) if len(src) else np.zeros(0, np.int64)
    src, dst = np.concatenate([src, src[dup], np.arange(n)[: n // 4]]), np.concatenate([dst, dst[dup], np.arange(n)[: n // 4]])
    p = g.permutation(len(src))
    src, dst = src[p], dst[p]
    if oob and len(dst):
        bad = g.random(len(dst)) < 0.1
        dst = np.where(bad, np.where(g.random(len(dst)) < 0.5, -1 - g.integers(0, 3, len(dst)), n + g.integers(0, 3, len(dst))), dst)
    return csr_from_pairs(n, src, dst)


# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,rp,col,dirn,ref,exact", table(), ids=[t[0] for t in table()])
def test_table(name, rp, col, dirn, ref, exact):
    assert tc_reference(rp, col, dirn) == ref
    assert marker_scan(rp, col, dirn) == ref
    assert tc_exact(rp, col, dirn) == exact


@pytest.mark.parametrize("dirn", [False, True])
def test_reference_restatement_matches_marker_scan(dirn):
    g = np.random.default_rng(20261015 + dirn)
    for trial in range(1500):
        n = int(g.integers(1, 14))
        e = int(g.integers(0, 3 * n + 2))
        rp, col = random_messy_graph(g, n, e, symmetric=bool(trial % 2), hub0=trial % 5 == 0, oob=trial % 7 == 0)
        assert tc_reference(rp, col, dirn) == marker_scan(rp, col, dirn), (trial, rp.tolist(), col.tolist())


def test_reference_restatement_larger_graphs():
    g = np.random.default_rng(7)
    for trial in range(12):
        n = int(g.integers(30, 120))
        rp, col = random_messy_graph(g, n, 4 * n, symmetric=trial % 2 == 0, hub0=trial % 3 == 0, oob=trial % 4 == 0)
        for dirn in (False, True):
            assert tc_reference(rp, col, dirn) == marker_scan(rp, col, dirn)


def test_exact_known_counts():
    for k in range(3, 9):  # K_k
        edges = [(a, b) for a in range(k) for b in range(a + 1, k)]
        rp, col = undirected(k, edges)
        assert tc_exact(rp, col) == comb(k, 3)
        rp, col = directed(k, [(a, b) for a in range(k) for b in range(k) if a != b])
        assert tc_exact(rp, col, True) == 2 * comb(k, 3)
    for k in range(3, 9):  # cycles
        rp, col = undirected(k, [(i, (i + 1) % k) for i in range(k)])
        assert tc_exact(rp, col) == (1 if k == 3 else 0)
        rp, col = directed(k, [(i, (i + 1) % k) for i in range(k)])
        assert tc_exact(rp, col, True) == (1 if k == 3 else 0)
    for k in range(4, 10):  # wheel: hub 0 and a rim of k vertices
        edges = [(0, i) for i in range(1, k + 1)] + [(i, i % k + 1) for i in range(1, k + 1)]
        rp, col = undirected(k + 1, edges)
        assert tc_exact(rp, col) == k


def test_exact_matches_dense_trace():
    g = np.random.default_rng(11)
    for trial in range(300):
        n = int(g.integers(1, 40))
        rp, col = random_messy_graph(g, n, int(g.integers(0, 4 * n + 1)), symmetric=trial % 3 == 0,
                                     hub0=trial % 4 == 0, oob=trial % 5 == 0)
        assert tc_exact(rp, col) == dense_trace(rp, col)
        assert tc_exact(rp, col, True) == dense_cycles(rp, col)


def test_empty_graphs():
    for dirn in (False, True):
        for rp, col in (([0], []), ([0, 0], []), ([0, 1], [0]), ([0, 0, 0, 0], [])):
            assert tc_reference(rp, col, dirn) == 0 == tc_exact(rp, col, dirn) == marker_scan(rp, col, dirn)


def test_entry_point_declared():
    text = open(os.path.join(ROOT, "include", "sbx.h")).read()
    assert re.search(r"int sbx_csr_triangle_count\(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t nnz,\s*"
                     r"const void \*row_ptr,\s*const void \*col, unsigned flags, int64_t \*count_host\);", text)
    assert "#define SBX_TC_DIRECTED 0x1u" in text and "#define SBX_TC_EXACT 0x2u" in text
    from sparsebase_amd import capi, ops
    assert "sbx_csr_triangle_count" in capi.PROTOTYPES
    assert callable(ops.csr_triangle_count)
