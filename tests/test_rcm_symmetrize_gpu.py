"""ops.rcm_reorder(..., symmetrize=True) on the GPU: on a structurally unsymmetric pattern it orders A ∪ Aᵀ — bit for bit
what ops.rcm_reorder gives on the numpy-symmetrized CSR and what the oracle's rcm_reorder (tests/orc.py) gives on it;
on a symmetric pattern it is the plain call; without the flag the unsymmetric pattern is refused as before."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TUPLES = {"i32": (np.int32, np.int32), "i64": (np.int64, np.int64), "i32_n64": (np.int64, np.int32)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import ops
    return ops


@pytest.fixture(scope="module")
def oracle():
    from orc import Oracle
    return Oracle()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _edges(name):
    """(n, src, dst) of a directed graph without duplicate edges."""
    g = np.random.default_rng(31)
    if name == "path":  # 0 -> 1 -> 2 ...
        n = 300
        return n, np.arange(n - 1), np.arange(1, n)
    if name == "digraph":
        n = 2000
        return n, g.integers(0, n, 3 * n), g.integers(0, n, 3 * n)
    n, hub = 6000, 5000  # one stored row of 5000 entries and none of their mirrors, next to a short chain
    cols = np.sort(g.choice(np.arange(1, n), hub, replace=False))
    return n, np.concatenate([np.zeros(hub, np.int64), np.arange(10, 40)]), np.concatenate([cols, np.arange(11, 41)])


@pytest.mark.parametrize("tup", list(TUPLES))
@pytest.mark.parametrize("name", ("path", "digraph", "hub"))
def test_unsymmetric_graphs(ops, oracle, name, tup):
    from sparsebase_amd import synth
    ot, idt = TUPLES[tup]
    n, src, dst = _edges(name)
    rp, col = synth.csr_from_edges(n, src, dst, np.int64)
    s2, d2 = synth.symmetrize(src, dst)
    rp_s, col_s = synth.csr_from_edges(n, s2, d2, np.int64)  # the numpy-symmetrized CSR
    assert len(col_s) > len(col)
    got = ops.rcm_reorder(_dev(rp.astype(ot)), _dev(col.astype(idt)), symmetrize=True)
    assert got.dtype == _dev(np.zeros(1, idt)).dtype
    got = got.cpu().numpy()
    assert np.array_equal(np.sort(got), np.arange(n))
    on_sym = ops.rcm_reorder(_dev(rp_s.astype(ot)), _dev(col_s.astype(idt))).cpu().numpy()
    assert got.tobytes() == on_sym.tobytes()
    want = oracle.rcm_reorder(rp_s.astype(np.int32), col_s.astype(np.int32))
    assert np.array_equal(got, want)


def test_symmetric_graph_is_the_plain_call(ops):
    from sparsebase_amd import synth
    rp, col = synth.random_symmetric_graph(3000, seed=3)
    plain, stats = ops.rcm_reorder(_dev(rp), _dev(col), return_stats=True)
    flagged, stats_f = ops.rcm_reorder(_dev(rp), _dev(col), return_stats=True, symmetrize=True)
    assert torch.equal(plain, flagged) and stats == stats_f
    out = torch.empty_like(plain)
    assert ops.rcm_reorder(_dev(rp), _dev(col), out=out, symmetrize=True) is out and torch.equal(out, plain)


def test_without_the_flag_the_directed_path_is_still_refused(ops):
    from sparsebase_amd import capi, synth
    n, src, dst = _edges("path")
    rp, col = synth.csr_from_edges(n, dst, src)  # k -> k - 1: the sweep from the smallest vertex reaches nothing else
    with pytest.raises(capi.SbxError) as e:
        ops.rcm_reorder(_dev(rp), _dev(col))
    assert e.value.status == 1 and "symmetric" in str(e.value)
    with pytest.raises(capi.SbxError):
        ops.rcm_reorder(_dev(rp), _dev(col), symmetrize=False)
    got = ops.rcm_reorder(_dev(rp), _dev(col), symmetrize=True).cpu().numpy()
    assert np.array_equal(np.sort(got), np.arange(n))
