"""feature::JaccardWeights without a GPU: the restatement of the rules every GPU test checks against, checked on a
worked example, and the entry point's presence in the C ABI.

The rules (reference feature/jaccard_weights_cuda.cu:99-150; include/sbx.h, sbx_csr_jaccard_weights), with
deg(x) = row_ptr[x+1] - row_ptr[x], for the entry at position p of row u with column v:
  1. skipped when deg(v) < deg(u), or deg(v) == deg(u) and v > u;
  2. otherwise I = entries t of row u, with multiplicity, that occur in row v, and other = the position the
     reference's binary search bst(v, u) lands on (1-based midpoints (left + right) >> 1 over row v), or -1;
  3. J = float32(I) / float32(deg(u) + deg(v) - I), correctly rounded; a float64 output holds it widened;
  4. out[p] = J, and out[other] = J when other != -1.
Positions no rule writes get J of their own (row, column) pair.
"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHUNK = 1 << 23  # row entries expanded at a time when counting intersections


def _csr_parts(rp, col):
    rp = np.asarray(rp, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(rp) - 1
    deg = np.diff(rp)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    return rp, col, n, deg, row


def _intersections(rp, col, n, keys, u, v):
    """I for every (u, v) pair: entries t of row u (with multiplicity) with t in row v (rows sorted).  v outside
    [0, n) is a row without entries."""
    out = np.zeros(len(u), np.int64)
    if len(u) == 0:
        return out
    du = rp[u + 1] - rp[u]
    vok = (v >= 0) & (v < n)
    ends = np.cumsum(du)
    start = 0
    while start < len(u):  # pairs [start, stop) expand to at most _CHUNK entries (or one pair)
        stop = max(start + 1, int(np.searchsorted(ends, (ends[start - 1] if start else 0) + _CHUNK, side="right")))
        d = du[start:stop]
        pid = np.repeat(np.arange(start, stop), d)
        off = np.arange(int(d.sum())) - np.repeat(np.cumsum(d) - d, d)
        t = col[rp[u[pid]] + off]
        key = v[pid] * n + t
        i = np.searchsorted(keys, key)
        hit = (i < len(keys)) & (keys[np.minimum(i, len(keys) - 1)] == key) & vok[pid]
        out[start:stop] = np.bincount(pid - start, weights=hit, minlength=stop - start).astype(np.int64)
        start = stop
    return out


def reference_bst(rp, col, n, v, target):
    """The reference's bst(v, target) (jaccard_weights_cuda.cu:69-90), vectorised: the position it lands on or -1."""
    vok = (v >= 0) & (v < n)
    vs = np.where(vok, v, 0)
    left = rp[vs] + 1
    right = np.where(vok, rp[vs + 1], 0)
    match = np.full(len(v), -1, np.int64)
    live = left <= right
    while live.any():
        mid = (left + right) >> 1
        c = col[np.where(live, mid - 1, 0)]
        gt, lt = live & (c > target), live & (c < target)
        eq = live & ~gt & ~lt
        match[eq] = mid[eq] - 1
        right = np.where(gt, mid - 1, right)
        left = np.where(lt, mid + 1, left)
        live = live & ~eq & (left <= right)
    return match


def _weights(rp, col, n, keys, deg, u, v):
    inter = _intersections(rp, col, n, keys, u, v)
    vok = (v >= 0) & (v < n)
    dv = np.where(vok, deg[np.where(vok, v, 0)], 0)
    den = deg[u] + dv - inter
    return inter.astype(np.float32) / den.astype(np.float32)


def jaccard_reference(rp, col, dtype=np.float32, return_written=False):
    """The rules above over a CSR with sorted rows: one `dtype` weight per nonzero.  With return_written, also the
    mask of the positions rules 1-4 write (the others hold the fill rule's value)."""
    rp, col, n, deg, row = _csr_parts(rp, col)
    nnz = len(col)
    keys = row * n + col  # sorted: rows are consecutive and their columns sorted
    vok = (col >= 0) & (col < n)
    dv = np.where(vok, deg[np.where(vok, col, 0)], -1)
    du = deg[row]
    kept = np.nonzero(~((dv < du) | ((dv == du) & (col > row))))[0]
    out = np.full(nnz, np.nan, np.float32)
    u, v = row[kept], col[kept]
    j = _weights(rp, col, n, keys, deg, u, v)
    other = reference_bst(rp, col, n, v, u)
    out[kept] = j
    has = other >= 0
    out[other[has]] = j[has]
    written = ~np.isnan(out)
    rest = np.nonzero(~written)[0]
    out[rest] = _weights(rp, col, n, keys, deg, row[rest], col[rest])
    out = out.astype(dtype)
    return (out, written) if return_written else out


# the worked example: edges 0-1, 0-2, 1-2, 2-3 of an undirected graph
EX_RP = [0, 2, 4, 7, 8]
EX_COL = [1, 2, 0, 2, 0, 1, 3, 2]
THIRD = np.float32(1) / np.float32(3)
EX_WANT = np.array([THIRD, 0.25, THIRD, 0.25, 0.25, 0.25, 0, 0], np.float32)
# the reference's test matrix (functionality_common.inc:6-12): 4 weights, all 0 (jaccard_weights_tests.cc)
REF_RP = [0, 2, 3, 4]
REF_COL = [1, 2, 0, 0]


def test_restatement_worked_example():
    assert THIRD.view(np.int32) == 0x3EAAAAAB
    got = jaccard_reference(EX_RP, EX_COL)
    assert np.array_equal(got.view(np.int32), EX_WANT.view(np.int32))
    got64 = jaccard_reference(EX_RP, EX_COL, np.float64)
    assert got64[0] == 0.3333333432674408 and got64[0] != 1 / 3
    assert np.array_equal(got64.view(np.int64), EX_WANT.astype(np.float64).view(np.int64))
    out, written = jaccard_reference(EX_RP, EX_COL, return_written=True)
    assert written.all()  # symmetric, no duplicates: the reference writes every position


def test_restatement_reference_matrix():
    out, written = jaccard_reference(REF_RP, REF_COL, return_written=True)
    assert np.array_equal(out.view(np.int32), np.zeros(4, np.int32)) and written.all()


def test_restatement_bst_and_fill_rule():
    # row 0 = [1, 1, 2]: duplicates; row 1 = [0]; row 2 = [] (asymmetric: 0 -> 2 has no way back)
    rp, col = [0, 3, 4, 4], [1, 1, 2, 0]
    r, c = np.array(rp, np.int64), np.array(col, np.int64)
    # bst(0, 1) over [1, 1, 2]: left 1, right 3, mid 2 -> col[1] == 1: position 1, not 0
    assert reference_bst(r, c, 3, np.array([0]), np.array([1]))[0] == 1
    assert reference_bst(r, c, 3, np.array([2]), np.array([0]))[0] == -1
    out, written = jaccard_reference(rp, col, return_written=True)
    # entry (1, 0): deg 1 <= 3 kept, I = 0 (row 1 = [0], 0 not in row 0) -> 0, written at 3 and at bst(0, 1) = 1
    assert written.tolist() == [False, True, False, True]
    # position 0 (0, 1): own weight, I = |{1, 1, 2} in {0}| = 0 -> 0; position 2 (0, 2): row 2 empty -> 0 / 3
    assert out.tolist() == [0.0, 0.0, 0.0, 0.0]
    # a self loop on a 2-row graph: (0,0) kept, I = 2 (0 and 1 both in row 0), J = 2 / (2 + 2 - 2) = 1
    out = jaccard_reference([0, 2, 3], [0, 1, 0])
    assert out[0] == 1.0 and out[1] == out[2] == np.float32(1) / np.float32(2)


def _header_functions():
    text = open(os.path.join(ROOT, "include", "sbx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(sbx_[a-z0-9_]+)\s*\(", text))


def test_entry_point_declared_bound_and_exported():
    from sparsebase_amd import build, capi
    assert "sbx_csr_jaccard_weights" in _header_functions()
    assert "sbx_csr_jaccard_weights" in capi.PROTOTYPES
    lib = build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    assert re.search(r"\bT sbx_csr_jaccard_weights\b", out)
    from sparsebase_amd import ops
    assert callable(ops.csr_jaccard_weights)
    import torch
    if not torch.cuda.is_available():  # the tensor layer refuses host tensors instead of computing there
        with pytest.raises(ValueError):
            ops.csr_jaccard_weights(torch.tensor(EX_RP, dtype=torch.int32), torch.tensor(EX_COL, dtype=torch.int32))
