"""feature::JaccardWeights on the MI355X (sbx_csr_jaccard_weights / ops.csr_jaccard_weights / the C++ host layer),
compared bit for bit with the restatement in test_jaccard_host.py."""
import os

import numpy as np
import pytest
import torch

from sparsebase_amd import ops, synth
from test_host_layer import built, run  # noqa: F401  (the host programs' fixture and runner)
from test_jaccard_host import EX_COL, EX_RP, EX_WANT, REF_COL, REF_RP, jaccard_reference

pytestmark = pytest.mark.gpu

# index tuples: (row_ptr dtype, col dtype) -> SBX_I32, SBX_I64, SBX_I32_N64
TUPLES = {"i32": (torch.int32, torch.int32), "i64": (torch.int64, torch.int64), "i32_n64": (torch.int64, torch.int32)}
# bins of the kernel by deg(u): <= 8, <= 16, <= 128 lanes-per-edge groups; above, a workgroup per edge with row v in
# LDS up to 64 KiB of ids (16384 int32 / 8192 int64), searched in global memory beyond
EDGES = (8, 16, 128)
LDS_IDS = {4: 16384, 8: 8192}


def _gpu(rp, col, tup="i32", dtype=torch.float32):
    rd, cd = TUPLES[tup]
    r = torch.as_tensor(np.asarray(rp, np.int64)).to(rd).cuda()
    c = torch.as_tensor(np.asarray(col, np.int64)).to(cd).cuda()
    out = ops.csr_jaccard_weights(r, c, dtype=dtype)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(got, want):
    it = np.int32 if want.dtype == np.float32 else np.int64
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.nonzero(got.view(it) != want.view(it))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} weights differ, first at {bad[:8]}: {got[bad[:8]]} vs {want[bad[:8]]}"


@pytest.mark.parametrize("tup", list(TUPLES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_worked_example_and_reference_matrix(tup, dtype):
    npd = np.float32 if dtype == torch.float32 else np.float64
    got = _gpu(EX_RP, EX_COL, tup, dtype)
    _same_bits(got, EX_WANT.astype(npd))
    if dtype == torch.float64:
        assert got[0] == 0.3333333432674408
    got = _gpu(REF_RP, REF_COL, tup, dtype)
    _same_bits(got, np.zeros(4, npd))


def _power_law_graph(n, seed, self_loop_frac=0.02):
    """Symmetric pattern with power-law degrees (preferential targets), ties of equal degree, self loops."""
    g = np.random.default_rng(seed)
    e = n * 6
    src = g.integers(0, n, e)
    dst = (n * g.random(e) ** 3).astype(np.int64)  # heavy towards low ids: hubs
    loops = np.nonzero(g.random(n) < self_loop_frac)[0]
    s = np.concatenate([src, dst, loops])
    d = np.concatenate([dst, src, loops])
    return synth.csr_from_edges(n, s, d, np.int64)


@pytest.mark.parametrize("seed,n", [(1, 2000), (2, 30000), (3, 120000)])
@pytest.mark.parametrize("tup", list(TUPLES))
def test_random_symmetric_power_law(seed, n, tup):
    rp, col = _power_law_graph(n, seed)
    want, written = jaccard_reference(rp, col, return_written=True)
    assert written.all()
    _same_bits(_gpu(rp, col, tup), want)
    if seed == 2:
        _same_bits(_gpu(rp, col, tup, torch.float64), want.astype(np.float64))


def test_generator_graph_with_isolated_vertices():
    rp, col = synth.random_symmetric_graph(50000, avg_deg=9.0, seed=4, isolated_frac=0.2, self_loop_frac=0.05)
    _same_bits(_gpu(rp, col), jaccard_reference(rp, col))


def test_empty_inputs():
    for tup, (rd, cd) in TUPLES.items():
        for n in (0, 5):
            r = torch.zeros(n + 1, dtype=rd, device="cuda")
            c = torch.zeros(0, dtype=cd, device="cuda")
            out = ops.csr_jaccard_weights(r, c)
            assert out.numel() == 0
    # empty rows between non-empty ones, and at both ends
    rp, col = [0, 0, 2, 2, 3, 3, 5], [1, 5, 5, 1, 3]
    _same_bits(_gpu(rp, col), jaccard_reference(rp, col))


def _hub_pairs(degrees, n_leaves, seed):
    """For every d: two hubs a, b of degree d adjacent to each other and to d - 1 leaves each, half of them shared
    (the edge a-b has deg(u) == deg(v) == d: it runs in d's bin, with row v of length d)."""
    g = np.random.default_rng(seed)
    hubs = 2 * len(degrees)
    n = hubs + n_leaves
    src, dst = [], []
    for i, d in enumerate(degrees):
        a, b = 2 * i, 2 * i + 1
        la = hubs + g.choice(n_leaves, d - 1, replace=False)
        keep = la[: (d - 1) // 2]
        fresh = np.setdiff1d(np.arange(hubs, n), la)
        lb = np.concatenate([keep, g.choice(fresh, d - 1 - len(keep), replace=False)])
        src += [np.full(d - 1, a), np.full(d - 1, b), [a]]
        dst += [la, lb, [b]]
    s, d = np.concatenate(src), np.concatenate(dst)
    rp, col = synth.csr_from_edges(n, np.concatenate([s, d]), np.concatenate([d, s]), np.int64)
    deg = np.diff(rp)
    for i, d in enumerate(degrees):
        assert deg[2 * i] == deg[2 * i + 1] == d
    return rp, col


@pytest.mark.parametrize("tup", list(TUPLES))
def test_bin_and_lds_boundaries(tup):
    ids = LDS_IDS[4 if TUPLES[tup][1] == torch.int32 else 8]
    degrees = [d + k for d in EDGES + (ids,) for k in (-1, 0, 1)] + [2, 3, 40000]  # 40000: a hub beyond the LDS
    rp, col = _hub_pairs(degrees, 60000, seed=11)
    want = jaccard_reference(rp, col)
    _same_bits(_gpu(rp, col, tup), want)


def test_asymmetric_and_duplicates_fill_rule():
    for seed in (5, 6):
        rp, col = synth.random_rect_csr(3000, 3000, 40000, seed=seed, idx_dtype=np.int64, dup_frac=0.1)
        want, written = jaccard_reference(rp, col, return_written=True)
        assert not written.all() and len(col) > len(np.unique(np.repeat(np.arange(3000), np.diff(rp)) * 3000 + col))
        for tup in TUPLES:
            got = _gpu(rp, col, tup)
            assert not np.isnan(got).any()
            _same_bits(got, want)
        _same_bits(_gpu(rp, col, "i32", torch.float64), want.astype(np.float64))


def test_rmat_scale18():
    rp, col = synth.rmat_symmetric(18, 8, seed=3)
    want = jaccard_reference(rp, col)
    _same_bits(_gpu(rp, col, "i32"), want)
    _same_bits(_gpu(rp, col, "i32_n64"), want)


def test_cpp_api(built):  # noqa: F811
    out = run(os.path.join(built, "test_jaccard"))
    assert "0 failures" in out and "FAIL" not in out, out
