"""Every size-dependent route of sbx_slashburn.hip at its boundaries, with proof that it ran.  The parity tests
(test_slashburn_gpu.py) compare results on inputs that meet these boundaries only by accident; here each input is
built to sit on one (slashburn_routes.py; test_slashburn_routes_host.py checks that it does), and every case

  * compares the device's inv with the restatement (test_slashburn_host.slashburn) exactly, and checks a permutation;
  * compares all five statistics with the restatement's;
  * runs the call twice on one handle and requires identical bytes: the atomics of the BFS keys, the appends and the
    component hooking must not reach the output;
  * takes the launch counts of the profiler's bfs_small_levels, bfs_expand, level_order and degree groups around the
    first call and requires the counts that the host driver's loop gives on the restatement's own level widths
    (slashburn_routes.expected_launches): a call that never left the workgroup kernel, or took one digit pass too
    few, fails even where its result is right.

The restatement on the long rows of the digit-pass cases, on this project's test host (one CPU thread): 1.1 to 1.4 s
per call with one row of 2^23 entries (24 bits, three passes) and 2.0 to 3.0 s with one row of 2^24 + a few entries
(25 bits, four passes), building the 17 M-entry input 0.8 s; so the restatement stays the oracle there too.
"""
import functools

import numpy as np
import pytest
import torch

import slashburn_routes as R
from sparsebase_amd import ops
from test_slashburn_host import slashburn

pytestmark = pytest.mark.gpu

# index tuples: (row_ptr dtype, col dtype) -> SBX_I32, SBX_I64, SBX_I32_N64
TUPLES = {"i32": (torch.int32, torch.int32), "i64": (torch.int64, torch.int64), "i32_n64": (torch.int64, torch.int32)}
STATS = ("rounds", "hubs", "spoke_components", "initial_components", "final_gcc")


def counted(call):
    """(result of call(), launches it added to each group of R.GROUPS) — the profiler is off again whatever happens."""
    ops.profile_enable(True)
    try:
        before = ops.profile_report()
        got = call()
        torch.cuda.synchronize()
        after = ops.profile_report()
    finally:
        ops.profile_enable(False)
    return got, {g: after.get(g, (0, 0, 0))[1] - before.get(g, (0, 0, 0))[1] for g in R.GROUPS}


def check(rp, col, k, greedy=False, hub_order=False, tups=tuple(TUPLES), maxdeg=None):
    """One case: the restatement once, the device for every index tuple.  Returns (inv, stats, expected launches)."""
    n = len(rp) - 1
    trace = []
    want, wst = slashburn(rp, col, k, greedy, hub_order, return_stats=True, trace=trace)
    launches = R.expected_launches(trace, wst["rounds"], greedy, R.maxdeg_s(rp, col) if maxdeg is None else maxdeg)
    rp64, col64 = torch.as_tensor(np.asarray(rp, np.int64)), torch.as_tensor(np.asarray(col, np.int64))
    for tup in tups:
        rd, cd = TUPLES[tup]
        r, c = rp64.to(rd).cuda(), col64.to(cd).cuda()
        call = lambda: ops.slashburn_reorder(r, c, k, greedy=greedy, hub_order=hub_order, return_stats=True)  # noqa: E731
        (inv, st), got_launches = counted(call)
        inv2, st2 = call()
        where = (tup, k, greedy, hub_order)
        assert inv.dtype == cd and torch.equal(inv, inv2) and st == st2, where  # twice, identical bytes
        got = inv.cpu().numpy().astype(np.int64)
        assert np.array_equal(np.sort(got), np.arange(n)), where
        assert np.array_equal(got, want), where
        assert {s: st[s] for s in STATS} == wst, where
        assert got_launches == launches, (where, got_launches, launches)
    return want, wst, launches


# ---- (a) level widths around SB_CAP, phase 0 only ---------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.LAYERED))
def test_level_widths_around_the_cap(name):
    widths = R.LAYERED[name]
    rp, col, n = R.layered_graph(widths)
    _, st, launches = check(rp, col, n + 1)
    assert st == dict(rounds=0, hubs=0, spoke_components=0, initial_components=1, final_gcc=n)
    small, expand, order = R.bfs_launches(widths)  # (the stated widths, not only the restatement's)
    assert launches == {"bfs_small_levels": small, "bfs_expand": expand, "level_order": order, "degree": 0}
    assert (expand > 0) == (max(widths) > R.SB_CAP)


# ---- (b) level 0 around SB_CAP ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1023, 1024, 1025, 1026])
def test_level_0_around_the_cap(count):
    rp, col, n = R.path_forest(count)
    _, st, launches = check(rp, col, n + 1)  # every component in one BFS from `count` roots
    assert st["initial_components"] == count and st["rounds"] == 0
    assert (launches["bfs_expand"] > 0) == (count > R.SB_CAP)
    _, st, launches = check(rp, col, 1)  # the largest component enters the loop: count - 1 roots
    assert st["rounds"] >= 1
    assert (launches["bfs_expand"] > 0) == (count - 1 > R.SB_CAP)


# ---- (c) the same boundaries inside a round ---------------------------------------------------------------------------

@pytest.mark.parametrize("hub_order", [False, True])
@pytest.mark.parametrize("two_hubs", [False, True])
@pytest.mark.parametrize("roots", [1024, 1025])
def test_boundaries_inside_a_round(roots, two_hubs, hub_order):
    rp, col, n, hubs = R.hub_graph(roots, two_hubs)
    inv, st, _ = check(rp, col, len(hubs), hub_order=hub_order)
    assert sorted(inv[hubs].tolist()) == list(range(len(hubs))) and st["rounds"] >= 2


# ---- (d) digit passes of the select -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def select_graph(name):
    return R.select_graph({**R.SELECT, **R.SELECT_25}[name][2])


def select_case(name, bits, degrees, k):
    rp, col, n = select_graph(name)
    _, st, launches = check(rp, col, k, tups=("i32", "i64"), maxdeg=max(degrees))
    passes = (bits + 7) // 8
    assert st["rounds"] >= 1 and launches["degree"] == st["rounds"] * (6 + 2 * passes)


@pytest.mark.parametrize("name", [s for s in R.SELECT if R.SELECT[s][0] <= 17])
def test_select_digit_passes(name):
    bits, _, degrees = R.SELECT[name]
    for k in range(1, len(degrees) + 1):
        select_case(name, bits, degrees, k)


@pytest.mark.parametrize("k", range(1, 7))
@pytest.mark.parametrize("name", [s for s in R.SELECT if R.SELECT[s][0] == 24])
def test_select_three_passes_24_bits(name, k):
    select_case(name, 24, R.SELECT[name][2], k)


@pytest.mark.parametrize("k", range(1, 7))
@pytest.mark.parametrize("name", list(R.SELECT_25))
def test_select_four_passes_25_bits(name, k):
    select_case(name, 25, R.SELECT_25[name][2], k)


# ---- (e) greedy beyond one chunk ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def greedy_graph(kind, n):
    return {"circulant": R.circulant, "degree345": R.degree345}[kind](n)


@pytest.mark.parametrize("hub_order", [False, True])
@pytest.mark.parametrize("k", [1, 3, 64])
@pytest.mark.parametrize("n", R.GREEDY_SIZES)
@pytest.mark.parametrize("kind", ["circulant", "degree345"])
def test_greedy_beyond_one_chunk(kind, n, k, hub_order):
    rp, col, _ = greedy_graph(kind, n)
    _, st, launches = check(rp, col, k, True, hub_order)
    assert st["rounds"] >= 1 and launches["degree"] == 4 * st["rounds"]


@pytest.mark.parametrize("hub_order", [False, True])
@pytest.mark.parametrize("zero_outside", [False, True])
@pytest.mark.parametrize("ring", [1100, 2300])
def test_greedy_negative_degrees(ring, zero_outside, hub_order):
    rp, col, n, h = R.negative_ring(ring, zero_outside)
    for k in (3, 64):
        inv, st, launches = check(rp, col, k, True, hub_order)
        assert inv[h] == 0 and launches["degree"] == 4 * st["rounds"]
        assert (np.flatnonzero(inv < k) >= (2 if zero_outside else 0)).all()  # every pick of round 0 comes from E


@pytest.mark.parametrize("hub_order", [False, True])
@pytest.mark.parametrize("k", [2, 3, 64])
@pytest.mark.parametrize("name", list(R.LATE))
def test_greedy_winner_beyond_the_first_chunk(name, k, hub_order):
    # after the hub every pick of round 0 is decided in a later chunk than the one its scan starts in, behind a chunk
    # whose last initial degree equals the best current degree (test_slashburn_routes_host.py checks that it is so)
    rp, col, n, h = R.late_winner(R.LATE[name])
    nb1 = R.LATE[name][1]
    inv, st, launches = check(rp, col, k, True, hub_order)
    assert inv[h] == 0 and inv[nb1] == 1 and launches["degree"] == 4 * st["rounds"]
