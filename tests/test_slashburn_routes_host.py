"""The inputs of test_slashburn_routes_gpu.py are what that module claims, checked without a GPU: a route test whose
input silently missed its boundary would hide a failure.  The restatement (test_slashburn_host.slashburn) reports the
level widths of every placement BFS; the launch-count walk (slashburn_routes.bfs_launches) is checked on them and
against its neighbours: 1024 <-> 1025 vertices and 16 <-> 17 bits change the expected counts."""
import numpy as np
import pytest

import slashburn_routes as R
from test_slashburn_host import slashburn, sym_adjacency


def run(rp, col, k, greedy=False, hub_order=False):
    trace = []
    inv, st = slashburn(rp, col, k, greedy, hub_order, return_stats=True, trace=trace)
    assert np.array_equal(np.sort(inv), np.arange(len(rp) - 1))
    return inv, st, trace


# ---- the walk --------------------------------------------------------------------------------------------------------

def test_walk_by_hand():
    assert R.bfs_launches([1]) == (1, 0, 0)
    assert R.bfs_launches([1, 1023, 1]) == (1, 0, 0)
    assert R.bfs_launches([1, 1024, 1024, 1]) == (1, 0, 0)
    # narrow ends WIDE (gather, commit), one grid level, its narrow child gathered and committed, back in the workgroup
    assert R.bfs_launches([1, 1025, 1]) == (2, 1, 4)
    assert R.bfs_launches([1, 1025]) == (1, 1, 2)
    assert R.bfs_launches([1024]) == (1, 0, 0) and R.bfs_launches([1025]) == (0, 1, 0)
    assert R.bfs_launches([1025, 7, 7]) == (1, 1, 2)
    # narrow, wide, wide, narrow after wide (3), stays in the workgroup for 1024, wide again, narrow
    assert R.bfs_launches([1, 1025, 1025, 3, 1024, 1025, 2]) == (3, 3, 10)
    assert R.degree_launches(3, True, 12345) == 12
    assert [R.passes_for(1 << (b - 1)) for b in (1, 8, 9, 16, 17, 24, 25, 31)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert R.degree_launches(2, False, 255) == 16 and R.degree_launches(2, False, 256) == 20


def test_a_neighbouring_input_changes_the_expected_counts():
    # 1024 <-> 1025 in a level, in the roots and after a wide level; 16 <-> 17 bits (and the other digit edges)
    assert R.bfs_launches([1, 1024, 1]) != R.bfs_launches([1, 1025, 1])
    assert R.bfs_launches([1024, 1024]) != R.bfs_launches([1025, 1025])
    assert R.bfs_launches([1025, 1024, 5]) != R.bfs_launches([1025, 1025, 5])
    for bits in (8, 16, 24):
        lo, hi = (1 << bits) - 1, 1 << bits
        assert lo.bit_length() == bits and hi.bit_length() == bits + 1
        assert R.degree_launches(1, False, hi) == R.degree_launches(1, False, lo) + 2
    assert R.degree_launches(5, False, 0xFFFF) == 5 * 10 and R.degree_launches(5, False, 0x10000) == 5 * 12


# ---- (a) level widths around SB_CAP ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.LAYERED))
def test_layered_graphs_have_the_stated_levels(name):
    widths = R.LAYERED[name]
    rp, col, n = R.layered_graph(widths)
    assert n == sum(widths)
    inv, st, trace = run(rp, col, n + 1)
    assert trace == [widths]  # one BFS from vertex 0
    assert st == dict(rounds=0, hubs=0, spoke_components=0, initial_components=1, final_gcc=n)
    assert inv[0] == n - 1
    order = np.argsort(-inv)  # the BFS order
    assert not np.array_equal(order[1:], np.sort(order[1:]))  # not the id order
    rows = [col[rp[i]:rp[i + 1]] for i in range(n)]
    assert any(len(r) > 1 and not np.array_equal(r, np.sort(r)) for r in rows)  # unsorted rows
    assert any(len(np.unique(r)) < len(r) for r in rows)  # a row that holds a child twice
    # some children of the second level have two parents in the first (only where that level has two vertices)
    srp, scol = sym_adjacency(rp, col, n)
    level = np.empty(n, np.int64)
    level[order] = np.repeat(np.arange(len(widths)), widths)
    src = np.repeat(np.arange(n), np.diff(srp))
    assert (np.abs(level[src] - level[scol]) <= 1).all()
    assert (level[src] == level[scol]).any()  # edges inside a level
    if max(widths[:-1]) > 1 and len(widths) > 3:
        up = np.unique(np.stack([src, scol])[:, level[scol] == level[src] - 1], axis=1)
        assert (np.bincount(up[0], minlength=n) >= 2).any()


def test_layered_walks():
    want = {"w1023": (1, 0, 0), "w1024": (1, 0, 0), "w1025": (2, 1, 4), "zigzag": (3, 3, 10), "w5000": (2, 1, 4)}
    assert {k: R.bfs_launches(w) for k, w in R.LAYERED.items()} == want


# ---- (b) level 0 around SB_CAP -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1023, 1024, 1025, 1026])
def test_path_forests_have_the_stated_roots(count):
    rp, col, n = R.path_forest(count)
    inv, st, trace = run(rp, col, n + 1)
    assert st["initial_components"] == count and st["rounds"] == 0 and st["final_gcc"] == 4
    assert len(trace) == 1 and trace[0][0] == count and trace[0][1] == count and len(trace[0]) == 4
    assert R.bfs_launches(trace[0])[1] == (2 if count > 1024 else 0)
    inv, st, trace = run(rp, col, 1)  # the largest component (the last by (size, root)) enters the loop
    assert trace[0][0] == count - 1 and st["rounds"] >= 1
    assert R.bfs_launches(trace[0])[1] == (2 if count - 1 > 1024 else 0)
    sizes = np.bincount(np.bincount(_component_of(rp, col, n)))
    assert sizes[2] > 100 and sizes[3] > 100 and sizes[4] > 100  # many equal sizes: the root breaks the ties


def _component_of(rp, col, n):
    from test_slashburn_host import _labels
    srp, scol = sym_adjacency(rp, col, n)
    return _labels(srp, scol, np.ones(n, bool))


# ---- (c) the same boundaries inside a round ----------------------------------------------------------------------------

@pytest.mark.parametrize("roots", [1024, 1025])
@pytest.mark.parametrize("two_hubs", [False, True])
def test_hub_graphs_place_the_stated_roots_in_round_0(roots, two_hubs):
    rp, col, n, hubs = R.hub_graph(roots, two_hubs)
    k = len(hubs)
    srp, _ = sym_adjacency(rp, col, n)
    deg = np.diff(srp)
    assert deg[hubs].min() > np.delete(deg, hubs).max()  # round 0 removes exactly the hub(s)
    outs = []
    for hub_order in (False, True):
        inv, st, trace = run(rp, col, k, False, hub_order)
        assert sorted(inv[hubs].tolist()) == list(range(k))
        assert st["initial_components"] == 1 and st["rounds"] > 1  # the star goes on as the GCC
        # round 0: one BFS from every path's root and the layered root; the 1025-wide level, a narrow one behind it
        w = trace[0]
        assert w[0] == roots and w[1] == roots - 1 + 8 and w[2] > 1025 and 0 < w[3] <= 1024 and len(w) == 4
        assert R.bfs_launches(w) == ((2, 2, 6) if roots <= 1024 else (1, 3, 6))
        # round 1: the star's leaves are all roots (k = 1: one of them goes on as the GCC; k = 2: one is the 2nd hub)
        assert trace[1] == [R.HUB_STAR - 1]
        outs.append(inv)
    assert np.array_equal(outs[0], outs[1]) == (not two_hubs)  # with two hubs the hub index orders the components


# ---- (d) digit passes --------------------------------------------------------------------------------------------------

def test_select_families():
    decided = {}
    for name, (bits, digit, degrees) in R.SELECT.items():
        rp, col, n = R.select_graph(degrees)
        assert n == 2 * len(degrees) <= 16
        stored = np.diff(rp)
        assert stored[0::2].tolist() == degrees and (stored[1::2] == 1).all()
        assert int(stored.max()).bit_length() == bits
        if bits <= 17:  # S adds nothing: every mirror is stored (the long rows' S is the GPU test's business)
            assert np.array_equal(sym_adjacency(rp, col, n)[0], rp)
            assert run(rp, col, n + 1)[1]["initial_components"] == 1
        differ = {p for p in range(4) for a in degrees[1:] for b in degrees[1:] if (a ^ b) >> 8 * p & 255}
        assert differ == {digit}, name  # (all heads up to 17 bits, all but the long one above)
        if bits <= 17:
            assert {p for p in range(4) if (degrees[0] ^ degrees[1]) >> 8 * p & 255} <= {digit}
        ks = [k for k in range(1, len(degrees) + 1)]
        decided.setdefault(bits, set()).update(R.decides(stored.tolist(), k) for k in ks)
        # a tie at tau: some k whose tau is shared by two or three heads and spans more than one digit when it can
        ties = [sorted(degrees, reverse=True)[k - 1] for k in ks if degrees.count(sorted(degrees, reverse=True)[k - 1]) > 1]
        assert ties and (bits <= 8 or max(ties) > 255), name
    for bits, seen in decided.items():
        assert seen >= set(range(R.passes_for(1 << (bits - 1)))), (bits, seen)  # every digit decides tau somewhere


def test_select_25_bits():
    # (no graph is built here: the 17 M-entry rows are the GPU test's; the degrees are the construction's own)
    seen = set()
    for name, (bits, digit, degrees) in R.SELECT_25.items():
        assert max(degrees).bit_length() == bits == 25 and R.passes_for(max(degrees)) == 4
        assert sorted(degrees)[-2] < 1 << 18 and sum(degrees) < (1 << 24) + (1 << 20)  # one long row only
        assert {p for p in range(4) for a in degrees[1:] for b in degrees[1:] if (a ^ b) >> 8 * p & 255} == {digit}
        every = degrees + [1] * len(degrees)  # the leaves are candidates too
        assert R.decides(every, 1) == 3  # the long head: the top digit
        assert all(R.decides(every, k) == digit for k in (2, 3, 4)), name  # ... and the digit of the family below it
        seen |= {R.decides(every, k) for k in range(1, 7)}
        tau = sorted(degrees, reverse=True)[3 - 1]
        assert degrees.count(tau) >= 2 or name == "b25_d0"  # k = 3: a tie at tau (b25_d0: at k = 4)
    assert seen >= {0, 1, 2, 3}  # every digit of a four-pass select decides tau somewhere
    assert R.SELECT_25["b25_d0"][2].count(5) == 3


# ---- (e) greedy beyond one chunk ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.GREEDY_SIZES)
def test_greedy_graphs(n):
    for build, degs in ((R.circulant, {4}), (R.degree345, {3, 4, 5})):
        rp, col, m = build(n)
        assert m == n
        srp, scol = sym_adjacency(rp, col, n)
        assert np.array_equal(srp, rp)  # symmetric and simple
        assert set(np.diff(srp).tolist()) == degs
        assert len(np.unique(_component_of(rp, col, n))) == 1  # E = every vertex
    assert -(-n // R.SB_WG) == {1023: 1, 1024: 1, 1025: 2, 2049: 3, 5003: 5}[n]  # chunks a full scan takes


@pytest.mark.parametrize("ring", [1100, 2300])
@pytest.mark.parametrize("zero_outside", [False, True])
def test_negative_ring(ring, zero_outside):
    rp, col, n, h = R.negative_ring(ring, zero_outside)
    srp, scol = sym_adjacency(rp, col, n)
    lab = _component_of(rp, col, n)
    E = lab == lab[h]
    assert E.sum() == ring + 1 > R.SB_WG and E[0] == (not zero_outside)
    deg = np.diff(srp)
    assert deg[h] == 5 * ring == deg.max()
    cur = deg.astype(np.int64)
    np.subtract.at(cur, scol[srp[h]:srp[h + 1]], 1)  # the first pick is h
    members = np.flatnonzero(E & (np.arange(n) != h))
    assert (cur[members] == -2).all()  # every eligible current degree is negative afterwards
    inv, st, _ = run(rp, col, 3, True)
    assert inv[h] == 0 and inv[members[0]] == 1  # then the smallest id of E, never vertex 0 outside it
    if zero_outside:
        assert inv[0] >= n - 2 and st["initial_components"] == 2


@pytest.mark.parametrize("name", list(R.LATE))
def test_late_winner_is_decided_beyond_the_first_chunk(name):
    na, nb1, nb2 = R.LATE[name]
    rp, col, n, h = R.late_winner(R.LATE[name])
    srp, scol = sym_adjacency(rp, col, n)
    assert len(np.unique(_component_of(rp, col, n))) == 1  # E = every vertex
    deg = np.diff(srp)
    assert deg[h] == na + nb1 == deg.max()
    assert (deg[:nb1] == 5).all() and (deg[nb1:nb1 + nb2] == 5).all() and (deg[nb1 + nb2:n - 1] == 6).all()
    assert na > R.SB_WG
    # round 0 as the restatement picks (the smallest id of the largest current degree), next to the kernel's scan
    k = 64
    elig, cur = np.ones(n, bool), deg.astype(np.int64)
    lst = R.picker_list(deg, elig)
    assert lst[0] == h and (lst[1:1 + na] >= nb1 + nb2).all()
    beyond = 0
    for j in range(k):
        want = int(np.argmax(np.where(elig, cur, np.iinfo(np.int64).min)))
        got, at, start = R.chunked_pick(lst, deg, cur, elig)
        assert got == want  # the kernel's stop rule is right
        if j >= 1:
            assert at >= start + R.SB_WG and nb1 <= want < nb1 + nb2  # the winner lies beyond the first chunk
            beyond += 1
            for wrong in ("first_chunk", "le", "init"):  # each wrong stop rule takes another vertex
                assert R.chunked_pick(lst, deg, cur, elig, wrong)[0] != want, (j, wrong)
        elig[want] = False
        row = scol[srp[want]:srp[want + 1]]
        np.subtract.at(cur, row[elig[row]], 1)
    assert beyond == k - 1
    inv, st, _ = run(rp, col, k, True)
    assert inv[h] == 0 and inv[nb1] == 1  # the second pick is the first B''
