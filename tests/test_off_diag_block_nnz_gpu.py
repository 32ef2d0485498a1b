"""sbxstat_csr_off_diag_block_nnz on the MI355X (ops.csr_off_diag_block_nnz): the count equals off_diag of
test_degree_stats_host.py exactly, for the three index tuples.  A tile of the stream over `col` is 2048 entries."""
import numpy as np
import pytest
import torch

from sparsebase_amd import capi, ops, synth
from test_degree_stats_host import REF_COL, REF_ROW_PTR, off_diag

pytestmark = pytest.mark.gpu

# index tuples: (row_ptr dtype, col dtype) -> SBX_I32, SBX_I64, SBX_I32_N64
TUPLES = {"i32": (torch.int32, torch.int32), "i64": (torch.int64, torch.int64), "i32_n64": (torch.int64, torch.int32)}
TILE = 2048


def _gpu(rp, col, m, h, w, tup):
    rd, cd = TUPLES[tup]
    r = torch.as_tensor(np.asarray(rp, np.int64)).to(rd).cuda()
    c = torch.as_tensor(np.asarray(col, np.int64)).to(cd).cuda()
    return ops.csr_off_diag_block_nnz(r, c, m, h, w)


def _check(rp, col, m, shapes, tups=tuple(TUPLES)):
    n = len(rp) - 1
    for h, w in shapes:
        want = off_diag(rp, col, n, m, h, w)
        for tup in tups:
            got = _gpu(rp, col, m, h, w, tup)
            assert got == want, f"{tup} n={n} m={m} h={h} w={w}: {got} != {want}"


def _csr(deg, m, seed, lo=0, hi=None):
    g = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(np.asarray(deg, np.int64))])
    return rp, g.integers(lo, m if hi is None else hi, int(rp[-1]))


def test_reference_case():
    for tup in TUPLES:
        assert _gpu(REF_ROW_PTR, REF_COL, 7, 3, 3, tup) == 8
    _check(REF_ROW_PTR, REF_COL, 7, [(1, 1), (7, 7), (2, 5), (5, 2), (10, 3), (3, 10)])


def test_block_shapes_on_a_rectangular_matrix():
    g = np.random.default_rng(1)
    rp, col = _csr(g.poisson(6, 203), 157, 2)
    # h = w = 1, h > n, h > w, w > h, neither dimension divisible, as many blocks as rows
    _check(rp, col, 157, [(1, 1), (500, 3), (204, 204), (13, 5), (5, 13), (7, 7), (203, 157), (2, 1), (1, 2), (64, 200)])
    rp, col = _csr(g.poisson(6, 90), 400, 3)
    _check(rp, col, 400, [(9, 9), (90, 400), (91, 7), (4, 33)])


@pytest.mark.parametrize("nnz", [0, TILE - 1, TILE, TILE + 1])
def test_nnz_around_a_tile(nnz):
    deg = np.zeros(64, np.int64)
    if nnz:
        deg[:] = nnz // 64
        deg[:nnz % 64] += 1
    rp, col = _csr(deg, 64, nnz)
    assert rp[-1] == nnz
    _check(rp, col, 64, [(4, 4), (64, 64), (1, 1)])


def test_block_boundaries_on_and_inside_a_tile_edge():
    rp, col = _csr([1024, 1024, 1000, 1000], 50, 4)      # rows 0-1 | 2-3: the boundary at position 2048
    _check(rp, col, 50, [(2, 2), (4, 4)])
    rp, col = _csr([1000, 1000, 1024, 1024, 3], 50, 5)    # the boundary at 2000, inside the first tile
    _check(rp, col, 50, [(2, 2), (5, 5), (3, 2)])
    rp, col = _csr([3, 3 * TILE + 500, 5], 9, 6)          # one row longer than three tiles
    _check(rp, col, 9, [(3, 3), (2, 2), (1, 3)])


def test_empty_rows_at_block_boundaries():
    deg = np.array([5, 0, 0, 7, 0, 3000, 0, 0, 0, 2, 0, 4000, 0, 0], np.int64)
    rp, col = _csr(deg, 14, 7)
    _check(rp, col, 14, [(2, 2), (7, 7), (14, 14), (3, 5), (20, 14)])
    rp, col = _csr(np.zeros(10, np.int64), 10, 8)
    _check(rp, col, 10, [(3, 3)])


def test_columns_outside_the_matrix():
    g = np.random.default_rng(9)
    rp, col = _csr(g.poisson(9, 700), 300, 10, lo=-6, hi=306)
    assert (col < 0).any() and (col >= 300).any()
    _check(rp, col, 300, [(7, 7), (1, 1), (700, 300), (30, 11)])


def test_power_law_matrix():
    n = 30000
    g = np.random.default_rng(11)
    e = n * 6
    src, dst = g.integers(0, n, e), (n * g.random(e) ** 3).astype(np.int64)
    rp, col = synth.csr_from_edges(n, np.concatenate([src, dst]), np.concatenate([dst, src]), np.int64)
    _check(rp, col, n, [(8, 8), (64, 64), (4096, 4096), (n + 1, 5)])


def test_rmat_scale18():
    rp, col = synth.rmat_symmetric(18, 8, seed=3)
    _check(rp, col, len(rp) - 1, [(64, 64)])


def test_no_blocks_and_no_column_blocks():
    rp, col = _csr([3, 4, 5], 3, 12)
    for tup in TUPLES:
        for h in (0, -1, -(2 ** 40)):
            assert _gpu(rp, col, 3, h, 3, tup) == 0 and _gpu(rp, col, 3, h, 0, tup) == 0
        for w in (0, -5):
            with pytest.raises(capi.SbxError) as e:
                _gpu(rp, col, 3, 2, w, tup)
            assert e.value.status == 1
