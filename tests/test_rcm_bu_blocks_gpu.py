"""The block front end of RCM's bottom-up levels (k_bfs_bottom_up_blocks / k_ubfs_bottom_up_blocks, sbx_rcm.hip): the
candidates of a level are read off the visited and the empty-row bitmaps a block of words at a time instead of giving a
lane to every vertex.  Every order is compared bit for bit with the oracle, with 32-bit and with 64-bit index arrays,
with the front end (the default) and, in a child process, without it (SBX_RCM_BU_BLOCKS=0: read once per process).

The graphs are "wheels": a centre, S spokes chained to their next few neighbours, a tail vertex behind some of the
spokes, and "late hubs" adjacent to a stretch of K spokes each.  The level of the spokes is wide and owns nearly every edge, so the
level behind it is expanded bottom-up, with the tails and the late hubs as candidates:
  * an unordered sweep goes bottom-up from a frontier of 1024 vertices on (more than 1024, or the small-level kernel keeps
    it) that owns more than half the unvisited edges: S = 1200 does it at n of two thousand;
  * the Cuthill-McKee sweep does from 8192 vertices on that own more than four times the unvisited edges: S = 10 000.
`pull_levels` restates the rule on the CPU (with a margin) and the first test checks, without a GPU, that every case
reaches the levels it is here for; on the GPU every case that has an edge asserts edges_scanned_bottom_up > 0.  (A graph
without an edge has no level at all: its case asserts the order alone, behind the others, on the scratch they left.)
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

# vertices per block of the front end's default build (32 words; a build with 16 has two in it; a variant build with
# 64 finds no whole block of its own size empty in these graphs: the product is what is tested)
BLOCK = 1024


# ------------------------------------------------------------------------------------------------ the graphs (CPU)
def wheel(S, T, hubs=(), reach=3):
    """Edges (u < v) of a wheel on 1 + S + T + len(hubs) vertices: 0 the centre, 1 .. S the spokes, then the tails
    (tail j behind spoke j), then one late hub per entry of `hubs`, adjacent to that many spokes."""
    assert T <= S and sum(hubs) <= S
    sp = np.arange(1, S + 1, dtype=np.int64)
    e = [np.stack([np.zeros(S, np.int64), sp])]
    for d in range(1, reach + 1):
        e.append(np.stack([sp[:-d], sp[d:]]))
    e.append(np.stack([sp[:T], S + 1 + np.arange(T, dtype=np.int64)]))
    at = min(T + 200, S - sum(hubs))  # a stretch of spokes per hub, behind the spokes with tails where there is room
    for i, k in enumerate(hubs):      # (a sweep from a tail then meets the hubs one level behind the spokes)
        e.append(np.stack([sp[at:at + k], np.full(k, 1 + S + T + i, np.int64)]))
        at += k
    return np.concatenate(e, axis=1), 1 + S + T + len(hubs)


def csr(n, edges, dtype=np.int32):
    """Symmetric CSR with sorted rows of the edges (2 x E) on n vertices."""
    u = np.concatenate([edges[0], edges[1]])
    v = np.concatenate([edges[1], edges[0]])
    key = np.unique(u * n + v)
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, key // n + 1, 1)
    return np.cumsum(rp).astype(dtype), (key % n).astype(dtype)


def small_wheel(n):
    """n vertices, none isolated: 1200-odd spokes, a late hub of 1100 (above the 1024 entries a lane scans alone)."""
    S = max(1200, (n - 2) * 11 // 20)
    edges, m = wheel(S, n - 2 - S, hubs=(1100,))
    assert m == n
    return n, edges, {"root": 0}


BIG = dict(S=10000, T=3007, hubs=(300, 1500, 2500), reach=6)  # 13 011 vertices: no multiple of 32; hubs of one, two, three chunks


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (n, edges, info): info['root'] the root of a component's first sweep (its smallest id) that must go bottom-up,
    info['big'] a member of a component whose Cuthill-McKee sweep must (or None)."""
    if name.startswith("n="):
        n, edges, info = small_wheel(int(name[2:]))
        return n, edges, dict(info, big=None)
    edges, m = wheel(**BIG)
    ids = np.arange(m, dtype=np.int64)
    if name == "big":
        return m, edges, {"root": 0, "big": 0}
    if name == "empty_blocks":
        # whole blocks of isolated ids in front, in the middle (three of them) and at the end (one and a partial one)
        place = ids + BLOCK + np.where(ids >= 4 * BLOCK + 100, 3 * BLOCK, 0)
        n = int(place[-1]) + 1
        n = (n + BLOCK - 1) // BLOCK * BLOCK + BLOCK + 77
        return n, place[edges], {"root": int(place[0]), "big": int(place[0])}
    if name == "alternating":
        place = 2 * ids + 1
        return 2 * m + 1, place[edges], {"root": 1, "big": 1}
    if name in ("second_wheel_behind", "second_wheel_in_front", "second_path_behind"):
        # two components: the sweeps of one never reach the other, whose vertices stay candidates in every level; the
        # component behind the first is ordered with labels.  (The rule sets a frontier's edges against ALL unvisited
        # edges of the graph: only the big wheel goes bottom-up — without labels where it comes first, with them
        # behind the small one.)
        if name == "second_path_behind":
            k = 2 * BLOCK + 300
            e2 = np.stack([np.arange(k - 1, dtype=np.int64), np.arange(1, k, dtype=np.int64)])
            m2 = k
        else:
            e2, m2 = wheel(1300, 900, hubs=(1100,), reach=1)
        if name == "second_wheel_in_front":
            return m + m2, np.concatenate([e2, edges + m2], axis=1), {"root": m2, "big": m2}
        return m + m2, np.concatenate([edges, e2 + m], axis=1), {"root": 0, "big": 0}
    raise KeyError(name)


CASES = ["n=2047", "n=2048", "n=2049", "n=4609", "big", "empty_blocks", "alternating", "second_wheel_behind",
         "second_wheel_in_front", "second_path_behind"]


@functools.lru_cache(maxsize=None)
def graph(name, bits):
    n, edges, info = case(name)
    return csr(n, edges, np.int32 if bits == 32 else np.int64) + (info,)


@functools.lru_cache(maxsize=None)
def want(name):
    from orc import Oracle
    rp, col, _ = graph(name, 32)
    out = Oracle().rcm_reorder(rp, col)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the rule (CPU)
def bfs_levels(rp, col, root):
    seen = np.zeros(len(rp) - 1, bool)
    seen[root] = True
    front, levels = np.array([root]), []
    while len(front):
        levels.append(front)
        lens = (rp[front + 1] - rp[front]).astype(np.int64)
        at = np.repeat(rp[front].astype(np.int64) - (np.cumsum(lens) - lens), lens) + np.arange(lens.sum())
        nb = np.unique(col[at])
        front = nb[~seen[nb]]
        seen[front] = True
    return levels


def pull_levels(rp, col, root, min_front, ratio):
    """Largest degree among the vertices each bottom-up level of the sweep from `root` finds: a level is expanded
    bottom-up when it holds min_front vertices and owns more than ratio times the unvisited edges."""
    deg, left, out = np.diff(rp).astype(np.int64), len(col), []
    levels = bfs_levels(rp, col, root)
    for k, lv in enumerate(levels[:-1]):
        fe = int(deg[lv].sum())
        left -= fe
        if len(lv) >= min_front and fe > ratio * left:
            out.append(int(deg[levels[k + 1]].max()))
    return out


def test_every_case_reaches_the_levels_it_is_here_for():
    """The direction rule restated, with a margin of a quarter on the ratios and 10 % on the sizes (the library counts
    the edges of the root's level a little differently from sweep to sweep): the first sweep of every case goes
    bottom-up at a level where a vertex of more than 1024 entries is still unvisited (the 16-lane groups of the
    unordered kernel), and the Cuthill-McKee sweep of the big wheels — from the root the oracle's order ends on — at a
    level that finds the late hubs of 300 (one chunk of the queue), 1500 and 2500 entries (several)."""
    for name in CASES:
        rp, col, info = graph(name, 32)
        assert max(pull_levels(rp, col, info["root"], 1130, 0.5 * 1.25), default=0) > 1024, name
        if info["big"] is not None:
            inv = want(name)
            comp = np.concatenate(bfs_levels(rp, col, info["big"]))
            cm_root = int(comp[np.argmax(inv[comp])])  # the order is reversed: the root comes last
            lv = bfs_levels(rp, col, cm_root)
            deg = np.diff(rp)
            hit = [k for k in range(len(lv) - 1) if 2500 in deg[lv[k + 1]]]
            assert hit and {300, 1500, 2500} <= set(deg[lv[hit[0] + 1]].tolist()), name
            assert len(lv[hit[0]]) >= 8192 * 1.1, name
            assert pull_levels(rp, col, cm_root, 8192 * 1.1, 4 * 1.25) and \
                max(pull_levels(rp, col, cm_root, 8192 * 1.1, 4 * 1.25)) >= 2500, name
    # the shapes: the last word and the last block partial, whole blocks empty, no edge
    assert [case(c)[0] % 32 for c in CASES[:5]] == [31, 0, 1, 1, 19] and case("n=4609")[0] % BLOCK
    rp, _, _ = graph("empty_blocks", 32)
    empty = np.diff(rp) == 0
    n = len(empty)
    assert empty[:BLOCK].all() and empty[n - n % BLOCK - BLOCK:].all() and n % BLOCK and n % 32
    assert any(empty[b:b + 2 * BLOCK].all() for b in range(BLOCK, n - 3 * BLOCK, BLOCK))
    rp, _, _ = graph("alternating", 32)
    assert (np.diff(rp)[0::2] == 0).all() and (np.diff(rp)[1::2] > 0).all()


# ------------------------------------------------------------------------------------------------ on the GPU
def run_case(ops, torch, name, bits):
    rp, col, _ = graph(name, bits)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got, stats = ops.rcm_reorder(d(rp), d(col), return_stats=True)
    got = got.cpu().numpy()
    assert got.dtype == rp.dtype
    assert np.array_equal(got, want(name)), (name, bits)
    assert stats["edges_scanned_bottom_up"] > 0, (name, bits, stats)


def run_no_edge(ops, torch, bits):
    """No edge at all (so no level of either direction: the one case without the edges_scanned_bottom_up assertion)."""
    from orc import Oracle
    n = 2 * BLOCK + 75
    rp = np.zeros(n + 1, np.int32 if bits == 32 else np.int64)
    col = np.zeros(0, rp.dtype)
    d = lambda a: torch.from_numpy(a).cuda()
    got, stats = ops.rcm_reorder(d(rp), d(col), return_stats=True)
    assert np.array_equal(got.cpu().numpy(), Oracle().rcm_reorder(rp.astype(np.int32), col.astype(np.int32)))
    assert stats["edges_scanned_bottom_up"] == 0


def run_all():
    """Every case, both index widths, in this process (the child of the test below)."""
    import torch
    from sparsebase_amd import ops
    for bits in (32, 64):
        for name in CASES:
            run_case(ops, torch, name, bits)
        run_no_edge(ops, torch, bits)
    print("bu blocks ok", 2 * (len(CASES) + 1))


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import ops
    return ops, torch


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", CASES)
def test_orders_with_the_block_front_end(gpu, name, bits):
    run_case(*gpu, name, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_no_edge_behind_the_others(gpu, bits):
    run_case(*gpu, "empty_blocks", bits)  # (leaves bitmaps of a larger graph in the scratch the next call reuses)
    run_no_edge(*gpu, bits)


@pytest.mark.gpu
def test_orders_without_the_block_front_end_in_a_child():
    """SBX_RCM_BU_BLOCKS=0 launches the kernels with a lane per vertex: the same cases, the same orders."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_rcm_bu_blocks_gpu as t\nt.run_all()\n"
            % (root, os.path.join(root, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SBX_RCM_BU_BLOCKS="0"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "bu blocks ok %d" % (2 * (len(CASES) + 1)) in r.stdout, r.stdout + r.stderr
