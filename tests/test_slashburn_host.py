"""reorder::SlashburnReorder without a GPU: a line-by-line transcription of the reference (reorder/slashburn_reorder.cc:
heap, DFS stack, FIFO), a numpy restatement of the rules include/sbx.h documents, and the closed form of the default
hub selection.  The transcription equals the recorded outputs of the real reference (tests/golden/slashburn.npz); the
restatement equals the transcription on thousands of random messy graphs; the device is compared with the restatement
(test_slashburn_gpu.py).  Numpy only."""
import heapq
import os
import re
import subprocess
from collections import deque

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "slashburn.npz")
FLAGS = [(g, h) for g in (False, True) for h in (False, True)]  # (greedy, hub_order)


class GreedyPicksOutsideE(Exception):
    """The reference's greedy seed (degree[0], 0) wins over every eligible vertex: only when vertex 0 is outside E and
    every eligible current degree is negative (a row that holds w more often than w's row holds it).  The reference
    then picks vertex 0 again; the device keeps to the rule (include/sbx.h lists the divergence)."""


# ---- the reference, line by line -------------------------------------------------------------------------------------

def _ref_symmetrize(rp, col, nodes):
    nnz = len(col)
    t_count = [0] * nodes
    for i in range(nnz):
        t_count[col[i]] += 1
    t_row = [0] * (nodes + 1)
    for i in range(1, nodes):
        t_row[i] = t_row[i - 1] + t_count[i - 1]
    t_row[nodes] = nnz
    t_col = [0] * nnz
    for i in range(nodes):
        for ptr in range(rp[i], rp[i + 1]):
            node_id = col[ptr]
            t_col[t_row[node_id] + t_count[node_id] - 1] = i
            t_count[node_id] -= 1
    last_row, last_col, s_flag = [0] * (nodes + 1), [], [0] * nodes
    for i in range(nodes):
        for ptr in range(rp[i], rp[i + 1]):
            node_id = col[ptr]
            last_col.append(node_id)
            s_flag[node_id] = i + 1
        for ptr in range(t_row[i], t_row[i + 1]):
            node_id = t_col[ptr]
            if s_flag[node_id] != i + 1:
                last_col.append(node_id)
        last_row[i + 1] = len(last_col)
    return last_row, last_col


def _find_cc(rptr, col, v_flag, level, root):
    cc_count = 1
    dfs = [root]
    v_flag[root] = level + 1
    while dfs:
        u = dfs.pop()
        for ptr in range(rptr[u], rptr[u + 1]):
            node_id = col[ptr]
            if v_flag[node_id] == level:
                dfs.append(node_id)
                v_flag[node_id] = level + 1
                cc_count += 1
    return cc_count


def _order_cc(rptr, col, v_flag, order, level, root, max_id):
    qwp2 = 0
    q = deque([root])
    order[max_id - qwp2] = root
    v_flag[root] = -level
    qwp2 += 1
    while q:
        u = q.popleft()
        for ptr in range(rptr[u], rptr[u + 1]):
            node_id = col[ptr]
            if v_flag[node_id] == level + 1:
                v_flag[node_id] = -level
                q.append(node_id)
                order[max_id - qwp2] = node_id
                qwp2 += 1
    return qwp2


def _compute_degree(rptr, col, n, v_flag, level):
    degree = [0] * n
    for i in range(n):
        if v_flag[i] == level:
            for ptr in range(rptr[i], rptr[i + 1]):
                if v_flag[col[ptr]] == level:
                    degree[i] += 1
        else:
            degree[i] = -1
    return degree


def _remove_k_hubset_greedy(rptr, col, n, k, v_flag, order, degree, level, min_id, strict):
    k_hub = [0] * k
    for i in range(k):
        pq = [(degree[0], 0)]
        for v in range(n):
            if v_flag[v] == level and degree[v] > pq[0][0]:
                heapq.heapreplace(pq, (degree[v], v))
        u = pq[0][1]
        if v_flag[u] != level and strict:
            raise GreedyPicksOutsideE()
        order[min_id + i] = u
        v_flag[u] = 0
        k_hub[i] = u
        degree[u] = -1
        for ptr in range(rptr[u], rptr[u + 1]):
            if v_flag[col[ptr]] == level:
                degree[col[ptr]] -= 1
    return k_hub


def _remove_k_hubset(rptr, col, n, k, v_flag, order, level, min_id):
    pq, k_hub = [], [0] * k
    i = j = 0

    def deg(v):
        return sum(1 for ptr in range(rptr[v], rptr[v + 1]) if v_flag[col[ptr]] == level)

    while i < n:
        if v_flag[i] == level:
            heapq.heappush(pq, (deg(i), i))
            j += 1
        if j == k:
            break
        i += 1
    for i in range(i + 1, n):
        if v_flag[i] == level:
            d = deg(i)
            if d > pq[0][0]:
                heapq.heapreplace(pq, (d, i))
    qwp1 = 0
    while pq:
        node_id = heapq.heappop(pq)[1]
        order[min_id + k - 1 - qwp1] = node_id
        v_flag[node_id] = 0
        k_hub[k - 1 - qwp1] = node_id
        qwp1 += 1
    return k_hub


def _slashloop(rptr, col, n, k, v_flag, order, level, max_id, greedy, hub_order, strict):
    pq_cc_hub = []
    while True:
        if greedy:
            degree = _compute_degree(rptr, col, n, v_flag, level)
            k_hub = _remove_k_hubset_greedy(rptr, col, n, k, v_flag, order, degree, level, (level - 2) * k, strict)
        else:
            k_hub = _remove_k_hubset(rptr, col, n, k, v_flag, order, level, (level - 2) * k)
        gcc_count, gcc_id, cmp_counter = 0, -1, 0
        for i in range(k - 1, -1, -1):
            u = k_hub[i]
            for ptr in range(rptr[u], rptr[u + 1]):
                node_id = col[ptr]
                if v_flag[node_id] == level:
                    n_cc = _find_cc(rptr, col, v_flag, level, node_id)
                    if n_cc > gcc_count:
                        gcc_count, gcc_id = n_cc, node_id
                    heapq.heappush(pq_cc_hub, (i if hub_order else 0, n_cc, node_id))
                    cmp_counter += 1
        if cmp_counter == 0:
            break
        for _ in range(cmp_counter):
            root = heapq.heappop(pq_cc_hub)
            if root[2] == gcc_id:
                continue
            max_id += _order_cc(rptr, col, v_flag, order, level, root[2], n - 1 - max_id)
        if gcc_count < k:
            _order_cc(rptr, col, v_flag, order, level, gcc_id, n - 1 - max_id)
            break
        level += 1


def reference_slashburn(rp, col, k, greedy=False, hub_order=False, strict=True):
    """GetReorderCSR (:296-419) with the call's own flags (a fresh process): inv[old] = new.  strict: raise
    GreedyPicksOutsideE where the reference's greedy pick leaves E instead of following it."""
    rp, col = [int(x) for x in rp], [int(x) for x in col]
    nodes = len(rp) - 1
    last_row, last_col = _ref_symmetrize(rp, col, nodes)
    order, v_flag = [0] * nodes, [1] * nodes
    pq, cmp_counter, max_id = [], 0, 0
    for i in range(nodes):
        if v_flag[i] == 1:
            heapq.heappush(pq, (_find_cc(last_row, last_col, v_flag, 1, i), i))
            cmp_counter += 1
    for _ in range(cmp_counter - 1):
        root = heapq.heappop(pq)[1]
        max_id += _order_cc(last_row, last_col, v_flag, order, 1, root, nodes - 1 - max_id)
    if pq[0][0] < k:
        _order_cc(last_row, last_col, v_flag, order, 1, heapq.heappop(pq)[1], nodes - 1 - max_id)
    else:
        heapq.heappop(pq)
        _slashloop(last_row, last_col, nodes, k, v_flag, order, 2, max_id, greedy, hub_order, strict)
    order2 = np.zeros(nodes, np.int64)
    order2[np.asarray(order, np.int64)] = np.arange(nodes)
    return order2


# ---- the rules, restated with numpy ----------------------------------------------------------------------------------

def sym_adjacency(rp, col, n):
    """S (:333-376): row i = its stored entries in stored order, then r for every stored (r, i) whose r is not among
    row i's stored columns, once per entry, in descending r."""
    rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    stored = np.unique(rows * n + col)
    keep = ~np.isin(col * n + rows, stored)  # the mirror (col, row) is not stored
    kr, kc = col[keep], rows[keep]            # row kr gets kc
    srow = np.concatenate([rows, kr])
    scol = np.concatenate([col, kc])
    second = np.concatenate([np.arange(len(rows)), len(rows) + (n - 1 - kc)])  # stored order, then descending r
    o = np.lexsort((second, srow))
    srp = np.zeros(n + 1, np.int64)
    np.add.at(srp, srow + 1, 1)
    return np.cumsum(srp), scol[o]


def _labels(srp, scol, alive):
    """Connected components of S limited to `alive`: every member labelled with the component's smallest id."""
    n = len(srp) - 1
    src = np.repeat(np.arange(n), np.diff(srp))
    ok = alive[src] & alive[scol]
    a, b = src[ok], scol[ok]
    lab = np.where(alive, np.arange(n), -1)
    if len(a) == 0:
        return lab
    while True:
        # every label is a root here (lab[lab[v]] == lab[v]): hook each root under the smallest label next to its tree
        m = lab.copy()
        np.minimum.at(m, lab[a], lab[b])
        while True:  # pointer jumping: labels stay ids of the same component
            mm = np.where(alive, m[np.maximum(m, 0)], -1)
            if np.array_equal(mm, m):
                break
            m = mm
        if np.array_equal(m, lab):
            return lab
        lab = m


def _members(lab, mask):
    """label -> its members (ascending), for the vertices in mask."""
    v = np.flatnonzero(mask)
    o = np.argsort(lab[v], kind="stable")
    keys, first = np.unique(lab[v][o], return_index=True)
    return dict(zip(keys.tolist(), np.split(v[o], first[1:])))


def _bfs_levels(srp, scol, members, root):
    """orderCC (:191-222): FIFO BFS over S limited to `members` from root, children in adjacency order; the order and
    the width of every level.  A long row is cut to the first occurrence of each column first (a repeat is seen
    already when its turn comes, so the order is the same)."""
    seen = {root}
    out, widths = [root], []
    level = [root]
    while level:
        widths.append(len(level))
        nxt = []
        for u in level:
            row = scol[srp[u]:srp[u + 1]]
            if len(row) > 256:
                row = row[np.sort(np.unique(row, return_index=True)[1])]
            for w in row.tolist():
                if w in members and w not in seen:
                    seen.add(w)
                    nxt.append(w)
        out += nxt
        level = nxt
    return out, widths


def _bfs_order(srp, scol, members, root):
    return _bfs_levels(srp, scol, members, root)[0]


def default_hubs(deg, elig, k):
    """The closed form of removeKHubset's size-k min-heap with strict replacement (:108-158): every vertex with
    deg > tau plus the LAST c (by id) of the degree-tau vertices with id <= T, in descending (deg, id) order."""
    ids = np.flatnonzero(elig)
    d = deg[ids]
    tau = np.sort(d)[::-1][k - 1]
    c = k - int((d > tau).sum())
    ge = ids[d >= tau]
    T = ge[k - 1]
    eq = ids[(d == tau) & (ids <= T)]
    hubs = np.concatenate([ids[d > tau], eq[len(eq) - c:]])
    return hubs[np.lexsort((-hubs, -deg[hubs]))]


def heap_hubs(deg, elig, k):
    """removeKHubset's heap itself, for the closed form's check."""
    pq, j, ids = [], 0, np.flatnonzero(elig)
    for v in ids:
        v = int(v)
        if j < k:
            heapq.heappush(pq, (int(deg[v]), v))
            j += 1
        elif deg[v] > pq[0][0]:
            heapq.heapreplace(pq, (int(deg[v]), v))
    return np.array([v for _, v in sorted(pq, reverse=True)], np.int64)


def slashburn(rp, col, k, greedy=False, hub_order=False, return_stats=False, trace=None):
    """The rules of include/sbx.h (sbx_slashburn_reorder): inv[old] = new.  return_stats: (inv, the five statistics of
    sbx_slashburn_stats).  trace: a list that receives, per batch of components placed together (phase 0, then each
    round), the level widths of the BFS from all of the batch's roots at once, W[0] = the number of roots."""
    n = len(rp) - 1
    srp, scol = sym_adjacency(rp, col, n)
    src = np.repeat(np.arange(n), np.diff(srp))
    pos = np.full(n, -1, np.int64)
    back = 0
    stats = dict(rounds=0, hubs=0, spoke_components=0, initial_components=0, final_gcc=0)
    batch = []

    def done():
        return (pos, stats) if return_stats else pos

    def place(members, root):
        nonlocal back
        order, widths = _bfs_levels(srp, scol, members, root)
        assert len(order) == len(members)
        pos[np.asarray(order)] = n - 1 - back - np.arange(len(order))
        back += len(order)
        batch.append(widths)

    def end_batch():
        if trace is not None and batch:
            trace.append([sum(w[i] for w in batch if i < len(w)) for i in range(max(map(len, batch)))])
        batch.clear()

    # phase 0
    lab = _labels(srp, scol, np.ones(n, bool))
    roots, sizes = np.unique(lab, return_counts=True)
    comps = sorted(zip(sizes.tolist(), roots.tolist()))
    stats["initial_components"] = len(comps)
    groups = _members(lab, np.ones(n, bool))
    for size, root in comps[:-1]:
        place(set(groups[root].tolist()), root)
    g_size, g_root = comps[-1]
    if g_size < k:
        place(set(groups[g_root].tolist()), g_root)
        end_batch()
        stats["final_gcc"] = g_size
        return done()
    end_batch()
    E = lab == g_root
    t = 0
    while True:
        inE = E[scol]
        deg = np.bincount(src[inE], minlength=n)
        if greedy:
            cur, elig, hubs = deg.astype(np.int64), E.copy(), []
            for _ in range(k):
                h = int(np.argmax(np.where(elig, cur, np.iinfo(np.int64).min)))  # smallest id of the maximum
                hubs.append(h)
                elig[h] = False
                row = scol[srp[h]:srp[h + 1]]
                np.subtract.at(cur, row[elig[row]], 1)
            hubs = np.asarray(hubs, np.int64)
        else:
            hubs = default_hubs(deg, E, k)
        pos[hubs] = t * k + np.arange(k)
        E[hubs] = False
        stats["rounds"] += 1
        stats["hubs"] += k
        lab = _labels(srp, scol, E)
        # the scan: rows h_{k-1} .. h_0; each component's first entry is its root, that row's j its hub index
        scan_j = np.concatenate([np.full(srp[h + 1] - srp[h], j) for j, h in reversed(list(enumerate(hubs)))])
        scan_c = np.concatenate([scol[srp[h]:srp[h + 1]] for h in hubs[::-1]])
        live = E[scan_c]
        first_lab, first_at = np.unique(lab[scan_c[live]], return_index=True)
        if len(first_lab) == 0:
            break
        root = scan_c[live][first_at]
        hub_j = scan_j[live][first_at]
        size = np.bincount(lab[E], minlength=n)[first_lab]
        g = min(range(len(first_lab)), key=lambda i: (-size[i], first_at[i]))  # largest, then earliest root entry
        others = sorted((int(hub_j[i]) if hub_order else 0, int(size[i]), int(root[i]), int(first_lab[i]))
                        for i in range(len(first_lab)) if i != g)
        stats["spoke_components"] += len(others)
        groups = _members(lab, E)
        for _, _, r, lb in others:
            members = groups[lb]
            E[members] = False
            place(set(members.tolist()), r)
        if size[g] < k:
            place(set(groups[int(first_lab[g])].tolist()), int(root[g]))
            end_batch()
            stats["final_gcc"] = int(size[g])
            break
        end_batch()
        E = lab == first_lab[g]
        t += 1
    assert (pos >= 0).all()
    return done()


# ---- graphs ----------------------------------------------------------------------------------------------------------

def csr_from_pairs(n, src, dst):
    """CSR that keeps the given entry order inside each row (unsorted rows, duplicates)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    o = np.argsort(src, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, src + 1, 1)
    return np.cumsum(rp), dst[o]


def random_messy_graph(g, n, e, symmetric=False):
    """Duplicates, self loops, unsorted rows, asymmetric patterns, isolated vertices."""
    src = g.integers(0, n, e)
    dst = g.integers(0, n, e)
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    dup = g.integers(0, len(src), len(src) // 5 + 1) if len(src) else np.zeros(0, np.int64)
    loops = g.integers(0, n, n // 4)
    src, dst = np.concatenate([src, src[dup], loops]), np.concatenate([dst, dst[dup], loops])
    p = g.permutation(len(src))
    return csr_from_pairs(n, src[p], dst[p])


def k_choices(n):
    return sorted({1, 2, 3, -(-n * 5 // 100), n, n + 5})


# ---- tests -----------------------------------------------------------------------------------------------------------

def golden():
    z = np.load(GOLDEN)
    for name in z["names"]:
        name = str(name)
        yield name, z[name + "/rp"], z[name + "/col"], z[name + "/cases"], z[name + "/inv"]


def test_transcription_matches_the_real_reference():
    seen = outside = 0
    for name, rp, col, cases, invs in golden():
        for (k, greedy, hub_order), inv in zip(cases.tolist(), invs):
            want = np.asarray(inv, np.int64)
            args = (rp, col, k, bool(greedy), bool(hub_order))
            assert np.array_equal(reference_slashburn(*args, strict=False), want), (name, k, greedy, hub_order)
            try:
                reference_slashburn(*args)
            except GreedyPicksOutsideE:
                outside += 1
                continue
            assert np.array_equal(slashburn(*args), want), (name, k, greedy, hub_order)
            seen += 1
    assert seen >= 240 and outside <= 10, (seen, outside)


def test_reference_test_graph():
    # reorder/slashburn_reorder tests: the 3-vertex graph of the reference suite, recorded from the reference
    z = np.load(GOLDEN)
    assert "ref3" in [str(x) for x in z["names"]] and "ash958" in [str(x) for x in z["names"]]


def test_restatement_matches_transcription():
    g = np.random.default_rng(20261016)
    checked = skipped = 0
    for trial in range(2100):
        n = int(g.integers(1, 16))
        rp, col = random_messy_graph(g, n, int(g.integers(0, 3 * n + 2)), symmetric=trial % 3 == 0)
        ks = k_choices(n)
        k = ks[trial % len(ks)]
        for greedy, hub_order in FLAGS:
            try:
                want = reference_slashburn(rp, col, k, greedy, hub_order)
            except GreedyPicksOutsideE:
                skipped += 1
                continue
            got = slashburn(rp, col, k, greedy, hub_order)
            assert np.array_equal(got, want), (trial, k, greedy, hub_order, rp.tolist(), col.tolist())
            checked += 1
    assert checked >= 8000 and skipped < 400, (checked, skipped)  # (at least 2,000 graphs in all four modes)


def test_restatement_larger_graphs():
    g = np.random.default_rng(5)
    for trial in range(16):
        n = int(g.integers(40, 160))
        rp, col = random_messy_graph(g, n, 3 * n, symmetric=trial % 2 == 0)
        for k in (1, 3, -(-n * 5 // 100)):
            for greedy, hub_order in FLAGS:
                try:
                    want = reference_slashburn(rp, col, k, greedy, hub_order)
                except GreedyPicksOutsideE:
                    continue
                assert np.array_equal(slashburn(rp, col, k, greedy, hub_order), want), (trial, k)


def test_closed_form_hubs_match_the_heap():
    g = np.random.default_rng(3)
    for trial in range(20000):
        n = int(g.integers(1, 40))
        deg = g.integers(0, int(g.integers(1, 8)), n)
        elig = g.random(n) < 0.8
        if not elig.any():
            elig[g.integers(0, n)] = True
        k = int(g.integers(1, elig.sum() + 1))
        assert np.array_equal(default_hubs(deg, elig, k), heap_hubs(deg, elig, k)), (trial, deg.tolist(), k)


def test_symmetrized_rows():
    # rows 0: [2, 1, 1], 1: [], 2: [0]; S row 1 gets 0 twice (two entries (0, 1)), row 2 keeps [0] (0 -> 2 is mirrored)
    srp, scol = sym_adjacency([0, 3, 3, 4], [2, 1, 1, 0], 3)
    assert srp.tolist() == [0, 3, 5, 6] and scol.tolist() == [2, 1, 1, 0, 0, 0]
    last_row, last_col = _ref_symmetrize([0, 3, 3, 4], [2, 1, 1, 0], 3)
    assert last_row == srp.tolist() and last_col == scol.tolist()
    # descending r for the added entries
    srp, scol = sym_adjacency([0, 1, 2, 3, 3], [3, 3, 3], 4)
    assert scol[srp[3]:srp[4]].tolist() == [2, 1, 0]


def test_is_a_permutation_and_flags_matter():
    g = np.random.default_rng(1)
    rp, col = random_messy_graph(g, 60, 200, symmetric=True)
    outs = {f: slashburn(rp, col, 3, *f) for f in FLAGS}
    for inv in outs.values():
        assert np.array_equal(np.sort(inv), np.arange(60))
    assert not np.array_equal(outs[(False, False)], outs[(True, False)])


def test_entry_point_declared():
    text = open(os.path.join(ROOT, "include", "sbx.h")).read()
    assert re.search(r"int sbx_slashburn_reorder\(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t nnz, "
                     r"const void \*row_ptr,\s*const void \*col, int64_t k, unsigned flags, void \*inv_perm_out,\s*"
                     r"sbx_slashburn_stats \*stats_host /\* may be NULL \*/\);", text)
    assert "#define SBX_SB_GREEDY 0x1u" in text and "#define SBX_SB_HUB_ORDER 0x2u" in text
    from sparsebase_amd import build, capi, ops
    assert "sbx_slashburn_reorder" in capi.PROTOTYPES
    assert [f for f, _ in capi.SlashburnStats._fields_] == ["rounds", "hubs", "spoke_components",
                                                            "initial_components", "final_gcc"]
    assert callable(ops.slashburn_reorder)
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()], text=True)
    assert re.search(r"\bT sbx_slashburn_reorder\b", out)
