"""Inputs that pin sbx_slashburn.hip's size-dependent routes, and the launch counts its host driver must produce on
them.  Shared by test_slashburn_routes_host.py (the inputs are what they claim) and test_slashburn_routes_gpu.py (the
device on them).  Numpy only; every builder is deterministic."""
import numpy as np

from test_slashburn_host import csr_from_pairs, sym_adjacency

SB_CAP = 1024  # widest BFS level of the one-workgroup kernel (sbx_slashburn.hip)
SB_WG = 1024   # chunk of the one-workgroup greedy picker
GROUPS = ("bfs_small_levels", "bfs_expand", "level_order", "degree")


# ---- the host driver's launches, from level widths -------------------------------------------------------------------

def bfs_launches(widths):
    """sb_place_components' BFS loop on level widths W (W[0] = the roots): launches of (bfs_small_levels, bfs_expand,
    level_order).  A frontier of at most SB_CAP vertices takes ONE workgroup launch that consumes levels while the
    next one is 1 .. SB_CAP wide; a wider next level is gathered and committed by the grid path (2 level_order
    launches).  A wider frontier takes one bfs_expand launch per level, and every non-empty next level, narrow or
    not, is gathered and committed."""
    w = [int(x) for x in widths] + [0]
    assert w[0] > 0 and all(x > 0 for x in w[:-1])
    small = expand = order = 0
    i = 0
    while True:
        if w[i] <= SB_CAP:
            small += 1
            while 0 < w[i + 1] <= SB_CAP:
                i += 1
            if w[i + 1] == 0:
                break
        else:
            expand += 1
            if w[i + 1] == 0:
                break
        order += 2
        i += 1
    return small, expand, order


def passes_for(maxdeg):
    """8-bit digit passes of the default hub select: ceil(bits(maxdeg) / 8)."""
    return (int(maxdeg).bit_length() + 7) // 8


def degree_launches(rounds, greedy, maxdeg):
    """sb_hubs' launches in the degree group: greedy 4 per round (degrees, keys, the picker, the commit), default
    6 + 2 per digit pass (degrees, select init, flags, T, mark, commit; histogram and pick per pass)."""
    return rounds * (4 if greedy else 6 + 2 * passes_for(maxdeg))


def expected_launches(trace, rounds, greedy, maxdeg):
    """{group: launches} of one call: trace = the level widths of every placement BFS (slashburn(..., trace=))."""
    parts = [bfs_launches(w) for w in trace]
    return {"bfs_small_levels": sum(p[0] for p in parts), "bfs_expand": sum(p[1] for p in parts),
            "level_order": sum(p[2] for p in parts), "degree": degree_launches(rounds, greedy, maxdeg)}


def maxdeg_s(rp, col):
    """The longest row of S."""
    return int(np.diff(sym_adjacency(rp, col, len(rp) - 1)[0]).max())


# ---- builders ----------------------------------------------------------------------------------------------------

class Pairs:
    """Directed entries collected in order; csr() keeps that order inside each row (after one fixed shuffle)."""

    def __init__(self, seed):
        self.g = np.random.default_rng(seed)
        self.src, self.dst = [], []

    def edge(self, a, b, how=None):
        """a - b stored in both directions (0), only a -> b (1) or only b -> a (2); how=None draws it."""
        how = int(self.g.integers(0, 3)) if how is None else how
        if how != 2:
            self.src.append(a)
            self.dst.append(b)
        if how != 1:
            self.src.append(b)
            self.dst.append(a)

    def csr(self, n, relabel=None):
        src, dst = np.asarray(self.src, np.int64), np.asarray(self.dst, np.int64)
        if relabel is not None:
            src, dst = relabel[src], relabel[dst]
        p = self.g.permutation(len(src))  # unsorted rows
        return csr_from_pairs(n, src[p], dst[p])


def _layered_into(pairs, widths, first):
    """A layered component on the ids first ..: level l holds widths[l] vertices, each joined to one parent in level
    l - 1 (a quarter of them to two, a fifth of the parent rows hold the child twice) and to nothing further up; a
    few edges run inside a level.  Returns (root, next free id)."""
    g = pairs.g
    levels, nxt = [], first
    for w in widths:
        levels.append(np.arange(nxt, nxt + w))
        nxt += w
    assert len(levels[0]) == 1
    for prev, cur in zip(levels[:-1], levels[1:]):
        for c in cur.tolist():
            ps = g.choice(prev, size=min(len(prev), 2 if g.random() < 0.25 else 1), replace=False)
            for p in ps.tolist():
                if g.random() < 0.2:  # the parent's row holds the child twice
                    pairs.edge(p, c, 1)
                    pairs.edge(p, c, 0)
                else:
                    pairs.edge(p, c)
        for _ in range(min(4, len(cur) // 2)):  # inside the level
            a, b = g.choice(cur, size=2, replace=False).tolist()
            pairs.edge(a, b)
    return int(levels[0][0]), nxt


def layered_graph(widths, seed=1):
    """(rp, col, n): one layered component; vertex 0 is the root, every other id shuffled (BFS order != id order)."""
    pairs = Pairs(seed)
    root, n = _layered_into(pairs, widths, 0)
    relabel = np.concatenate([[0], 1 + pairs.g.permutation(n - 1)])
    assert relabel[root] == 0
    rp, col = pairs.csr(n, relabel)
    return rp, col, n


LAYERED = {
    "w1023": [1, 1023, 1],
    "w1024": [1, 1024, 1024, 1],
    "w1025": [1, 1025, 1],
    "zigzag": [1, 1025, 1025, 3, 1024, 1025, 2],
    "w5000": [1, 5000, 1],
}


def _paths_into(pairs, count, first, join=None, mult=1):
    """count paths of 2 .. 4 vertices (sizes cycle, so many are equal) on the ids first ..; the first vertex of each
    is joined to `join` when given, and the row of `join` holds it `mult` times.  Returns (the paths as id lists,
    next free id)."""
    paths, nxt = [], first
    for i in range(count):
        size = 2 + (i * 7 + i // 5) % 3
        ids = list(range(nxt, nxt + size))
        nxt += size
        for a, b in zip(ids[:-1], ids[1:]):
            pairs.edge(a, b)
        if join is not None:
            pairs.edge(join, ids[0], 0)
            for _ in range(mult - 1):
                pairs.edge(join, ids[0], 1)
        paths.append(ids)
    return paths, nxt


def path_forest(count, seed=2):
    """(rp, col, n): `count` components, paths of 2 .. 4 vertices.  Ids are shuffled, but every component's smallest
    id (its root) sits at an end of its path, so the BFS levels are `count` wide for as long as the paths last."""
    pairs = Pairs(seed)
    paths, n = _paths_into(pairs, count, 0)
    ids = pairs.g.permutation(n)
    relabel = np.empty(n, np.int64)
    at = 0
    for p in paths:
        mine = np.sort(ids[at:at + len(p)])
        at += len(p)
        relabel[p[0]] = mine[0]
        relabel[p[1:]] = pairs.g.permutation(mine[1:])
    rp, col = pairs.csr(n, relabel)
    return rp, col, n


HUB_LAYERS = [1, 8, 1025, 2]  # the layered component of hub_graph: a 1025-wide level, 1036 vertices
HUB_STAR = 1200               # leaves of its star, the largest component once the hubs are gone


def hub_graph(roots, two_hubs, seed=3):
    """(rp, col, n, hubs): roots - 1 short paths, one layered component (HUB_LAYERS) and one star of HUB_STAR leaves,
    held together by the hub(s), whose rows hold every path's first vertex more than once: the largest degrees.
    One hub: it is joined to every path, to the layered root and to the star's centre; k = 1 removes exactly it, the
    star is round 0's GCC, and ONE BFS from `roots` roots places the paths and the layered component, its 1025-wide
    level and the narrow one behind it included.  Two hubs, joined to each other: hub A takes all but 300 paths, hub
    B 300 paths, the layered root and the star; k = 2 removes both, and both hub indices occur in the order keys."""
    pairs = Pairs(seed)
    nh = 2 if two_hubs else 1
    a, b = 0, nh - 1
    if two_hubs:
        pairs.edge(a, b, 0)
        _, nxt = _paths_into(pairs, roots - 1 - 300, nh, join=a, mult=2)
        _, nxt = _paths_into(pairs, 300, nxt, join=b, mult=5)
    else:
        _, nxt = _paths_into(pairs, roots - 1, nh, join=a, mult=2)
    root, nxt = _layered_into(pairs, HUB_LAYERS, nxt)
    pairs.edge(b, root, 0)
    centre, n = nxt, nxt + 1 + HUB_STAR
    pairs.edge(b, centre, 0)
    for leaf in range(centre + 1, n):
        pairs.edge(centre, leaf)
    relabel = pairs.g.permutation(n)
    rp, col = pairs.csr(n, relabel)
    return rp, col, n, [int(relabel[h]) for h in range(nh)]


# ---- the digit passes of the select -----------------------------------------------------------------------------------

def select_graph(degrees, ids=None):
    """(rp, col, n): heads a_0 .. a_{H-1} joined in a path; row a_i stores a private leaf b_i as often as it takes to
    give a_i the degree degrees[i]; row b_i stores a_i once.  ids: the heads' ids (default 2 i; the leaf is id + 1)."""
    H = len(degrees)
    ids = [2 * i for i in range(H)] if ids is None else ids
    n = 2 * H
    src, dst = [], []
    for i, d in enumerate(degrees):
        nb = [ids[j] for j in (i - 1, i + 1) if 0 <= j < H]
        mult = d - len(nb)
        assert mult >= 1
        src.append(np.full(len(nb) + mult, ids[i], np.int64))
        dst.append(np.concatenate([np.asarray(nb[:1], np.int64), np.full(mult, ids[i] + 1, np.int64),
                                   np.asarray(nb[1:], np.int64)]))
        src.append(np.asarray([ids[i] + 1], np.int64))
        dst.append(np.asarray([ids[i]], np.int64))
    rp, col = csr_from_pairs(n, np.concatenate(src), np.concatenate(dst))
    return rp, col, n


# multipliers of the digit that decides: three heads share the value 2, and ids run against the degrees
_C = (2, 1, 2, 3, 2, 0)
_TOP = (0, 1, 0, 1, 0, 1)  # for a top digit that can only be 0 or 1


def _fam(base, step, mult=_C):
    return [base + m * step for m in mult]


# name -> (bits(maxdeg_S), the digit position (from the low end) in which the heads differ, degrees).  Up to 17 bits
# the heads agree in every other digit.  At 24 and 25 bits one head alone carries the top bit (a family that agreed in
# the top digit would need six rows of 2^23 entries or more): the select finds it for k = 1 through the top digit, and
# for k >= 2 carries krem = k - 1 through a zero top digit down to the digit in which the five others differ.
SELECT = {
    "b8_d0": (8, 0, _fam(0x80, 1)),
    "b9_d0": (9, 0, _fam(0x105, 1)),
    "b9_d1": (9, 1, _fam(0x07, 0x100, _TOP)),
    "b16_d0": (16, 0, _fam(0x8010, 1)),
    "b16_d1": (16, 1, _fam(0x8011, 0x100)),
    "b17_d0": (17, 0, _fam(0x10110, 1)),
    "b17_d1": (17, 1, _fam(0x11011, 0x100)),
    "b17_d2": (17, 2, _fam(0x00111, 0x10000, _TOP)),
    "b24_d0": (24, 0, [0x800113] + _fam(0x000110, 1)[1:]),
    "b24_d1": (24, 1, [0x801311] + _fam(0x001011, 0x100)[1:]),
    "b24_d2": (24, 2, [0x800111] + _fam(0x010111, 0x10000)[1:]),
}
# 25 bits, four passes: one row of 2^24 + a few entries carries the top digit; the five others differ in digit 0, 1 or
# 2, so that for k >= 2 the pass of that digit decides tau with krem and the prefix carried through the passes above
SELECT_25 = {
    "b25_d0": (25, 0, [0x1000005, 5, 7, 5, 5, 6]),
    "b25_d1": (25, 1, [0x1000005, 0x105, 0x205, 0x305, 0x205, 0x005]),
    "b25_d2": (25, 2, [0x1000105, 0x010105, 0x020105, 0x030105, 0x020105, 0x000105]),
}


def decides(degrees, k):
    """The digit position (from the low end) of the last pass of the radix select at which a degree other than tau,
    the k-th largest, is still among the candidates: the pass that decides tau.  None when all degrees are equal."""
    degrees = [int(d) for d in degrees]
    tau = sorted(degrees, reverse=True)[k - 1]
    cands, last = degrees, None
    for p in reversed(range(passes_for(max(degrees)))):
        if any(x != tau for x in cands):
            last = p
        cands = [x for x in cands if (x >> 8 * p) & 255 == (tau >> 8 * p) & 255]
    return last


# ---- greedy beyond one chunk ------------------------------------------------------------------------------------------

GREEDY_SIZES = (1023, 1024, 1025, 2049, 5003)


def circulant(n, seed=4):
    """(rp, col, n): C_n(1, 2) with shuffled ids: every degree is 4."""
    g = np.random.default_rng(seed)
    relabel = g.permutation(n)
    i = np.arange(n)
    src = np.concatenate([i, i, i, i])
    dst = np.concatenate([(i + 1) % n, (i - 1) % n, (i + 2) % n, (i - 2) % n])
    p = g.permutation(len(src))
    rp, col = csr_from_pairs(n, relabel[src[p]], relabel[dst[p]])
    return rp, col, n


def degree345(n, seed=5):
    """(rp, col, n): a connected simple graph with degrees in {3, 4, 5}: the cycle, the chords i - i + n // 2 (3 each;
    an odd n joins its last vertex to vertex 2), chords i - i + 7 from every third vertex (4 on i and i + 7) and
    chords i - i + 9 from every sixth (5 on both ends).  Ids are shuffled, so degree and id are unrelated."""
    g = np.random.default_rng(seed)
    edges = {(i, (i + 1) % n) for i in range(n)}
    edges |= {(i, i + n // 2) for i in range(n // 2)}
    if n % 2:
        edges.add((2, n - 1))
    edges |= {(i, i + 7) for i in range(0, n - 7, 3)}
    edges |= {(i, i + 9) for i in range(0, n - 9, 6)}
    assert len({(min(a, b), max(a, b)) for a, b in edges}) == len(edges)
    a = np.asarray(sorted(edges), np.int64)
    relabel = g.permutation(n)
    src = relabel[np.concatenate([a[:, 0], a[:, 1]])]
    dst = relabel[np.concatenate([a[:, 1], a[:, 0]])]
    p = g.permutation(len(src))
    rp, col = csr_from_pairs(n, src[p], dst[p])
    return rp, col, n


def negative_ring(ring, zero_outside, seed=6):
    """(rp, col, n, h): a ring of `ring` vertices and one hub h whose row stores every ring vertex five times while
    each ring vertex stores h once: after h is picked every eligible current degree is 3 - 5 < 0.  zero_outside: the
    ids 0 and 1 form a component of their own, so vertex 0 lies outside E."""
    g = np.random.default_rng(seed)
    lo = 2 if zero_outside else 0
    n = lo + ring + 1
    relabel = np.concatenate([np.arange(lo), lo + g.permutation(ring + 1)])
    r = lo + np.arange(ring)
    h = lo + ring
    src = [r, r, r, np.repeat(h, 5 * ring)]
    dst = [lo + (np.arange(ring) + 1) % ring, lo + (np.arange(ring) - 1) % ring, np.full(ring, h), np.tile(r, 5)]
    if zero_outside:
        src.append(np.array([0, 1]))
        dst.append(np.array([1, 0]))
    src, dst = np.concatenate(src), np.concatenate(dst)
    p = g.permutation(len(src))
    rp, col = csr_from_pairs(n, relabel[src[p]], relabel[dst[p]])
    return rp, col, n, int(relabel[h])


LATE = {"late_1100": (1100, 1500, 1500), "late_2100": (2100, 1000, 300)}  # (|A|, |B'|, |B''|)


def late_winner(sizes, seed=7):
    """(rp, col, n, h): a graph on which every pick of round 0 after the first is decided beyond the first chunk of
    the picker's list.  All vertices but the hub h lie on a circulant C_m(1, 2) in shuffled positions (degree 4).
      B'   the lowest ids: joined to h                    initial degree 5, after h is picked 4
      B''  the ids above them: a self loop               initial degree 5, never lowered by h
      A    the highest ids: joined to h, and a self loop  initial degree 6, after h is picked 5
    The list is h, A by id, B' by id, B'' by id.  After h every A stands at 5 with a high id: the smallest id of
    current degree 5 is the first B'', behind all of A (more than one chunk) and all of B' (lowered to 4, so a
    chunk that ends inside B' has last initial degree 5 = the best current degree and must not stop the scan)."""
    na, nb1, nb2 = sizes
    m = na + nb1 + nb2
    g = np.random.default_rng(seed)
    h = m
    ring = g.permutation(m)  # ring position -> id
    i = np.arange(m)
    src = [ring[i], ring[i], ring[i], ring[i]]
    dst = [ring[(i + 1) % m], ring[(i - 1) % m], ring[(i + 2) % m], ring[(i - 2) % m]]
    b1, b2, a = np.arange(nb1), np.arange(nb1, nb1 + nb2), np.arange(nb1 + nb2, m)
    to_h = np.concatenate([b1, a])
    loops = np.concatenate([b2, a])
    src += [to_h, np.full(len(to_h), h), loops]
    dst += [np.full(len(to_h), h), to_h, loops]
    src, dst = np.concatenate(src), np.concatenate(dst)
    p = g.permutation(len(src))
    rp, col = csr_from_pairs(m + 1, src[p], dst[p])
    return rp, col, m + 1, h


def picker_list(deg, elig):
    """k_sb_greedy's list: the eligible vertices by (initial degree desc, id asc)."""
    ids = np.flatnonzero(elig)
    return ids[np.lexsort((ids, -deg[ids]))]


def chunked_pick(lst, init, cur, elig, rule="right"):
    """One pick as k_sb_greedy scans for it: chunks of SB_WG list entries from the first eligible one, the best
    (current degree, smallest id) so far, and a stop rule after each chunk.  Returns (vertex, its list index, the
    index the scan started at).  rule: "right" = the kernel's (last initial degree < best current degree); three
    wrong ones: "first_chunk" (never look further), "le" (<=), "init" (compare with the best's INITIAL degree)."""
    start = next(i for i, v in enumerate(lst) if elig[v])
    best = None  # (cur, -id, index)
    for c0 in range(start, len(lst), SB_WG):
        for i in range(c0, min(c0 + SB_WG, len(lst))):
            v = lst[i]
            if elig[v] and (best is None or (cur[v], -v) > best[:2]):
                best = (int(cur[v]), -int(v), i)
        last_init = int(init[lst[min(c0 + SB_WG, len(lst)) - 1]])
        if best is not None:
            bound = {"right": best[0], "le": best[0] + 1, "init": int(init[-best[1]]), "first_chunk": 1 << 62}[rule]
            if last_init < bound:
                break
    return -best[1], best[2], start
