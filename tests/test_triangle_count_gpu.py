"""feature::TriangleCount on the MI355X (sbx_csr_triangle_count / ops.csr_triangle_count / the C++ host layer): the
device count equals the restatements in test_triangle_count_host.py exactly, for every mode, direction and index
tuple."""
import os
from math import comb

import numpy as np
import pytest
import torch

from sparsebase_amd import ops, synth
from test_host_layer import built, run  # noqa: F401  (the host programs' fixture and runner)
from test_triangle_count_host import (csr_from_pairs, directed, random_messy_graph, table, tc_exact, tc_reference,
                                      undirected)

pytestmark = pytest.mark.gpu

# index tuples: (row_ptr dtype, col dtype) -> SBX_I32, SBX_I64, SBX_I32_N64
TUPLES = {"i32": (torch.int32, torch.int32), "i64": (torch.int64, torch.int64), "i32_n64": (torch.int64, torch.int32)}
MODES = [(d, e) for d in (False, True) for e in (False, True)]  # (directed, exact)
# exact mode bins by the probed list's length: <= 8, <= 16, <= 128 lanes-per-item groups; above, a workgroup per
# item with the searched list in LDS up to 16384 ids, searched in global memory beyond
BINS = (8, 16, 128, 16384)


def _gpu(rp, col, tup, dirn, exact):
    rd, cd = TUPLES[tup]
    r = torch.as_tensor(np.asarray(rp, np.int64)).to(rd).cuda()
    c = torch.as_tensor(np.asarray(col, np.int64)).to(cd).cuda()
    return ops.csr_triangle_count(r, c, directed=dirn, exact=exact)


def _check(rp, col, tups=tuple(TUPLES), modes=tuple(MODES)):
    for dirn, exact in modes:
        want = (tc_exact if exact else tc_reference)(rp, col, dirn)
        for tup in tups:
            got = _gpu(rp, col, tup, dirn, exact)
            assert got == want, f"{tup} directed={dirn} exact={exact}: {got} != {want}"


@pytest.mark.parametrize("tup", list(TUPLES))
def test_table_and_reference_graphs(tup):
    for name, rp, col, dirn, ref, exact in table():
        assert _gpu(rp, col, tup, dirn, False) == ref, name
        assert _gpu(rp, col, tup, dirn, True) == exact, name
    for k in (3, 5, 9):
        rp, col = undirected(k, [(a, b) for a in range(k) for b in range(a + 1, k)])
        assert _gpu(rp, col, tup, False, True) == comb(k, 3)
        assert _gpu(rp, col, tup, True, True) == 2 * comb(k, 3)
        _check(rp, col, (tup,))


def _power_law(n, seed, hub0):
    g = np.random.default_rng(seed)
    e = n * 6
    src = g.integers(0, n, e)
    dst = (n * g.random(e) ** 3).astype(np.int64)  # heavy towards low ids: hubs
    if not hub0:
        dst = (dst + n // 2) % n
    return synth.csr_from_edges(n, np.concatenate([src, dst]), np.concatenate([dst, src]), np.int64)


@pytest.mark.parametrize("seed,n,hub0", [(1, 2000, True), (2, 30000, True), (3, 30000, False)])
def test_power_law_with_hubs(seed, n, hub0):
    rp, col = _power_law(n, seed, hub0)
    if hub0:
        assert np.diff(rp).argmax() == 0
    _check(rp, col)


def test_exact_bins_and_lds_directed():
    """Per size d: an arc a -> b (a < b) and d vertices s with b -> s -> a, the probed lists out(b), in(a) of length d
    (d = 20000: beyond the LDS); plus noise arcs into low ids that the cut to values > a removes."""
    sizes = [d + k for d in BINS for k in (-1, 0, 1)] + [1, 2, 20000]
    src, dst, nxt = [], [], 0
    for d in sizes:
        a, b = nxt, nxt + 1
        s = np.arange(nxt + 2, nxt + 2 + d)
        nxt += 2 + d
        src += [[a], np.full(d, b), s]
        dst += [[b], s, np.full(d, a)]
    n = nxt
    s, d = np.concatenate(src), np.concatenate(dst)
    rp, col = csr_from_pairs(n, s, d)
    assert tc_exact(rp, col, True) == sum(sizes)
    _check(rp, col, modes=((True, True), (True, False), (False, False)))


def test_exact_bins_undirected():
    # a clique of 300 (oriented lists of every length 0 .. 299) joined to a sparse random graph
    g = np.random.default_rng(9)
    k = 300
    e = [(a, b) for a in range(k) for b in range(a + 1, k)]
    n = 6000
    rs, rd = g.integers(0, n, 30000), g.integers(0, n, 30000)
    rp, col = csr_from_pairs(n, np.concatenate([[a for a, b in e], [b for a, b in e], rs, rd]),
                             np.concatenate([[b for a, b in e], [a for a, b in e], rd, rs]))
    assert tc_exact(rp, col) >= comb(k, 3)
    _check(rp, col)


@pytest.mark.parametrize("seed", [4, 5])
def test_asymmetric_duplicates_self_loops_unsorted(seed):
    g = np.random.default_rng(seed)
    for trial in range(6):
        n = int(g.integers(50, 3000))
        rp, col = random_messy_graph(g, n, 8 * n, symmetric=trial % 2 == 0, hub0=trial % 3 == 0)
        _check(rp, col)


def test_out_of_range_columns():
    g = np.random.default_rng(8)
    for trial in range(4):
        n = int(g.integers(20, 2000))
        rp, col = random_messy_graph(g, n, 6 * n, symmetric=trial % 2 == 0, hub0=trial == 1, oob=True)
        assert ((col < 0) | (col >= n)).any()
        _check(rp, col)


def test_small_and_empty():
    cases = [([0], []), ([0, 0], []), ([0, 1], [0]), ([0, 2], [0, 0]), ([0, 0, 0, 0, 0, 0], []),
             ([0, 1, 2], [1, 0]), directed(3, [(0, 1), (1, 2), (2, 0), (0, 0)])]
    for rp, col in cases:
        _check(rp, col)


def test_random_small_graphs_many_calls():
    g = np.random.default_rng(12)
    for trial in range(40):
        n = int(g.integers(1, 40))
        rp, col = random_messy_graph(g, n, int(g.integers(0, 4 * n + 1)), symmetric=trial % 2 == 0,
                                     hub0=trial % 4 == 0, oob=trial % 5 == 0)
        _check(rp, col, tups=(("i32", "i64", "i32_n64")[trial % 3],))


def test_rmat_scale18():
    rp, col = synth.rmat_symmetric(18, 8, seed=3)
    _check(rp, col, tups=("i32", "i32_n64"))
    tri = tc_exact(rp, col)
    assert tri > 0 and _gpu(rp, col, "i64", True, True) == 2 * tri  # every edge both ways: two 3-cycles per triangle


def test_cpp_api(built):  # noqa: F811
    out = run(os.path.join(built, "test_triangle_count"))
    assert "0 failures" in out and "FAIL" not in out, out
