"""reorder::SlashburnReorder on the MI355X (sbx_slashburn_reorder / ops.slashburn_reorder / the C++ host layer): the
device's inverse permutation equals the recorded outputs of the real reference and the restatement in
test_slashburn_host.py exactly, for every index tuple and flag combination."""
import os

import numpy as np
import pytest
import torch

from sparsebase_amd import capi, ops, synth
from test_host_layer import built, run  # noqa: F401  (the host programs' fixture and runner)
from test_slashburn_host import (FLAGS, GreedyPicksOutsideE, csr_from_pairs, golden, k_choices, random_messy_graph,
                                 reference_slashburn, slashburn)

pytestmark = pytest.mark.gpu

# index tuples: (row_ptr dtype, col dtype) -> SBX_I32, SBX_I64, SBX_I32_N64
TUPLES = {"i32": (torch.int32, torch.int32), "i64": (torch.int64, torch.int64), "i32_n64": (torch.int64, torch.int32)}


def _dev(rp, col, tup):
    rd, cd = TUPLES[tup]
    return (torch.as_tensor(np.asarray(rp, np.int64)).to(rd).cuda(),
            torch.as_tensor(np.asarray(col, np.int64)).to(cd).cuda())


def _gpu(rp, col, k, greedy, hub_order, tup="i32", stats=False):
    r, c = _dev(rp, col, tup)
    out = ops.slashburn_reorder(r, c, k, greedy=greedy, hub_order=hub_order, return_stats=stats)
    if stats:
        return out[0].cpu().numpy().astype(np.int64), out[1]
    return out.cpu().numpy().astype(np.int64)


def _check(rp, col, ks, flags=FLAGS, tups=tuple(TUPLES)):
    n = len(rp) - 1
    for k in ks:
        for greedy, hub_order in flags:
            want, want_stats = slashburn(rp, col, k, greedy, hub_order, return_stats=True)
            for tup in tups:
                got, stats = _gpu(rp, col, k, greedy, hub_order, tup, stats=True)
                assert np.array_equal(np.sort(got), np.arange(n)), (tup, k, greedy, hub_order)
                assert np.array_equal(got, want), (tup, k, greedy, hub_order)
                assert stats == want_stats, (tup, k, greedy, hub_order)  # all five of sbx_slashburn_stats


@pytest.mark.parametrize("tup", list(TUPLES))
def test_recorded_reference_outputs(tup):
    for name, rp, col, cases, invs in golden():
        for (k, greedy, hub_order), inv in zip(cases.tolist(), invs):
            args = (rp, col, k, bool(greedy), bool(hub_order))
            try:
                reference_slashburn(*args)
                want = np.asarray(inv, np.int64)
            except GreedyPicksOutsideE:  # the reference leaves E there; the device keeps to the rule
                want = slashburn(*args)
            assert np.array_equal(_gpu(*args, tup), want), (name, k, greedy, hub_order)


def test_random_messy_graphs():
    g = np.random.default_rng(20261017)
    for trial in range(240):
        n = int(g.integers(1, 60))
        rp, col = random_messy_graph(g, n, int(g.integers(0, 4 * n + 2)), symmetric=trial % 3 == 0)
        ks = k_choices(n)
        tup = list(TUPLES)[trial % 3]
        _check(rp, col, [ks[trial % len(ks)], ks[(trial + 3) % len(ks)]], tups=(tup,))


def _power_law(n, seed, hub0):
    g = np.random.default_rng(seed)
    e = n * 6
    src = g.integers(0, n, e)
    dst = (n * g.random(e) ** 3).astype(np.int64)  # heavy towards low ids: hubs
    if not hub0:
        dst = (dst + n // 2) % n
    return csr_from_pairs(n, np.concatenate([src, dst]), np.concatenate([dst, src]))


@pytest.mark.parametrize("hub0", [True, False])
def test_power_law(hub0):
    rp, col = _power_law(3000, 5 + hub0, hub0)
    _check(rp, col, [1, 15, 150])


def _banded(n, w):
    src, dst = [], []
    for d in range(-w, w + 1):
        i = np.arange(max(0, -d), min(n, n - d))
        src.append(i)
        dst.append(i + d)
    return csr_from_pairs(n, np.concatenate(src), np.concatenate(dst))


def test_banded_many_rounds_deep_bfs():
    rp, col = _banded(4000, 3)  # k = 10: hundreds of rounds; the final GCC is a deep chain
    want = slashburn(rp, col, 10)
    got, st = _gpu(rp, col, 10, False, False, stats=True)
    assert np.array_equal(got, want)
    assert st["rounds"] >= 250 and st["hubs"] == 10 * st["rounds"]
    _check(rp, col, [10, 40], flags=[(True, False), (False, True)], tups=("i64",))
    rp, col = _banded(20000, 2)  # k > n: one component placed by one BFS of 10,000 levels
    _check(rp, col, [20001], flags=[(False, False)], tups=("i32",))


def test_shapes():
    # star, clique, grid, 10^4 tiny components, n = 1, k >= n
    star = csr_from_pairs(50, [0] * 49 + list(range(1, 50)), list(range(1, 50)) + [0] * 49)
    _check(*star, [1, 2, 49, 50, 60])
    k = 12
    clique = csr_from_pairs(k, [a for a in range(k) for b in range(k) if a != b],
                            [b for a in range(k) for b in range(k) if a != b])
    _check(*clique, [1, 3, 12, 13])
    s, d = [], []
    for i in range(30):
        for j in range(30):
            v = i * 30 + j
            if j + 1 < 30:
                s += [v, v + 1]
                d += [v + 1, v]
            if i + 1 < 30:
                s += [v, v + 30]
                d += [v + 30, v]
    _check(*csr_from_pairs(900, s, d), [1, 5, 45])
    pairs = np.arange(0, 20000, 2)
    tiny = csr_from_pairs(20000, np.concatenate([pairs, pairs + 1]), np.concatenate([pairs + 1, pairs]))
    _check(*tiny, [1, 3, 20000], tups=("i32", "i64"))
    _check(np.array([0, 0]), np.array([], np.int64), [1, 5])
    _check(np.array([0, 1]), np.array([0]), [1, 2])
    _check(np.array([0, 0, 0, 0]), np.array([], np.int64), [1, 2, 3, 4])


@pytest.mark.parametrize("greedy", [False, True])
def test_rmat_scale_18(greedy):
    rp, col = synth.rmat_symmetric(18, 8, seed=11)
    n = len(rp) - 1
    k = 1310
    want = slashburn(rp, col, k, greedy, False)
    got, st = _gpu(rp, col, k, greedy, False, stats=True)
    assert np.array_equal(got, want)
    assert st["rounds"] >= 2 and st["hubs"] == k * st["rounds"]
    assert st["initial_components"] >= 1
    assert np.array_equal(_gpu(rp, col, k, greedy, True, "i32_n64"), slashburn(rp, col, k, greedy, True))
    assert n == 1 << 18


def test_flags_are_held_per_call():
    g = np.random.default_rng(9)
    rp, col = random_messy_graph(g, 200, 700, symmetric=True)
    plain = _gpu(rp, col, 3, False, False)
    greedy = _gpu(rp, col, 3, True, True)
    assert not np.array_equal(plain, greedy)
    again = _gpu(rp, col, 3, False, False)  # the same handle: a greedy call does not stick
    assert np.array_equal(plain, again)
    assert np.array_equal(plain, slashburn(rp, col, 3))


def test_bad_arguments():
    rp, col = _dev([0, 2, 3, 4], [1, 2, 0, 0], "i32")
    with pytest.raises(capi.SbxError) as e:
        ops.slashburn_reorder(rp, col, 0)
    assert e.value.status == 1
    rp2, col2 = _dev([0, 2, 3, 4], [1, 3, 0, 0], "i32")
    with pytest.raises(capi.SbxError) as e:
        ops.slashburn_reorder(rp2, col2, 1)
    assert e.value.status == 1
    rp3, col3 = _dev([0, 2, 3, 4], [1, -1, 0, 0], "i64")
    with pytest.raises(capi.SbxError) as e:
        ops.slashburn_reorder(rp3, col3, 1)
    assert e.value.status == 1
    # the handle still works after the refusals
    assert ops.slashburn_reorder(rp, col, 1).cpu().tolist() == [0, 1, 2]
    # n = 0: nothing to write
    empty = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert ops.slashburn_reorder(empty, torch.zeros(0, dtype=torch.int32, device="cuda"), 1).numel() == 0


def test_host_layer_program(built):
    out = run(os.path.join(built, "test_slashburn"), attempts=1)
    assert "0 failures" in out and "FAIL" not in out, out
