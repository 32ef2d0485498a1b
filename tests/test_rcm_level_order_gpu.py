"""Every way run_bfs (sbx_rcm.hip) orders a BFS level of more than 4096 vertices, at the smallest sizes that reach it,
with the proof that it ran.

A level above RCM_LDS_SORT = 4096 vertices is ordered by one of seven routes.  CM is the final Cuthill-McKee sweep,
plain an ordered sweep of the pseudo-peripheral search; fsize is the parent level's size, nf this level's;
bitmap_pass = nf >= max(32768, n / 128); set_bits = !bitmap_pass:

    count:fresh         counting sort on, nf <= 2^20, plain, bitmap pass                       (k_fresh_words)
    count:fresh_ranked  counting sort on, nf <= 2^20, CM, 16 nf >= n_ranked                     (k_fresh_words_ranked)
    count:scatter       counting sort on, nf <= 2^20, everything else                           (k_rank_scatter + k_rank_counts)
    radix:fresh         counting sort off or nf > 2^20; plain, bitmap pass
    radix:fresh_ranked  the same; CM, bitmap pass, SBX_RCM_RANKED_KEYS on, nf * ranked_div >= n_ranked
    radix:full          the same; everything else       (k_level_keys, a packed key: low_mask != 0 in the fused emit)
    emit_only           a radix:fresh* level behind a one-vertex parent level: no digit to sort by, k_level_emit

SBX_DEBUG_RCM_LEVEL_PATHS=1 makes run_bfs print the route of every such level (host side only: the launches are the
same).  Each mode below is one child process (the switches are read once per process) that runs a list of graphs
through ops.rcm_reorder, compares every order bit for bit with the CPU restatement and leaves that trace on stderr; the
parent asserts that the routes the mode exists for are IN the trace — a change that reroutes levels turns these tests
red, it cannot make them vacuous — and prints the trace when anything fails.

The graphs are built for the conditions of the table, not taken from a workload (none has more than 110 000 vertices
or 600 000 stored entries):
  layers      layers of 30, 9000, 33000, 60000, 5000, 300 vertices between two tails of eight single vertices, edges
              between neighbouring layers only, every vertex with a neighbour in both of them: the tails' ends are the
              farthest vertices of all (the search ends at one) and from either end the sweep's levels are the layers.
              33000: a bitmap pass below n_ranked / 3 (radix:full without bits); 60000: above it (radix:fresh_ranked);
              9000 and 5000: no bitmap pass; 16 * 5000 < n_ranked (count:scatter in a CM sweep)
  lens        1, 1, 1, 200, 40000, 200, 1, 1, 1 with edges inside the wide layer: that level owns more than four times
              the edges left, so the next one goes bottom-up (mark_frontier = 1); a parent level of 200: one digit pass
  lens_small  the same around 12000 vertices: mark_frontier = 1 without a bitmap pass (both bitmaps from the emit)
  star        a hub, 40000 leaves, 3000 empty rows (n != n_ranked): the leaves' parent level is the hub alone (emit_only)
  two_wide    two components with a wide level each (9000 and 10000 vertices)
  rmat16      synth.rmat_symmetric(16, 8): hubs, the split expansion, bottom-up levels
A level of up to 8192 vertices behind a frontier of up to 4096 vertices and 32768 adjacency entries never gets here
(k_bfs_small_levels orders it in LDS), hence 9000 behind the 30 and the 5000 only behind the 60000.
In the wide layers a vertex has one or two neighbours a layer up (several discoverers: the atomicMin on the parent
position), degrees differ (the degree rank decides) and many vertices share (parent, degree): the sort must be stable.
Labels are shuffled.  layers, lens_small and star also run with int64 arrays (sbx_rcm64.hip: the same routes).

Not covered, neither has a small shape: the `scanned` leg of the *fresh* routes (more than RCM_FW_INLINE = 4096
workgroups: a span above 2^24 vertices) and three digit passes of the counting sort (a parent level above 262 144
vertices).

Wall time per child on an MI355X, interpreter and torch start-up included (the graphs' part in brackets):
  default 2.4 - 2.8 s (0.14 - 0.20 s: the list twice, once under the profiler), ordered 2.3 - 2.7 s (0.12 s),
  radix 2.4 - 2.5 s (0.13 - 0.14 s, the list twice), radix_ordered 2.3 - 2.5 s (0.12 s), radix_full_keys 2.3 - 2.6 s
  (0.12 s), radix_ranked_all 2.4 - 2.5 s (0.12 s): two runs of each; the reference orders are computed before the clock
  of the graphs' part starts.  In the same run of the whole suite the children of test_rcm_sweep_variants_in_a_child took
  3.2 - 3.8 s each.
"""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = {
    "default": {},
    "ordered": {"SBX_RCM_UNORDERED": "0"},
    "radix": {"SBX_RCM_COUNT_SORT": "0"},
    "radix_ordered": {"SBX_RCM_COUNT_SORT": "0", "SBX_RCM_UNORDERED": "0"},
    "radix_full_keys": {"SBX_RCM_COUNT_SORT": "0", "SBX_RCM_RANKED_KEYS": "0"},
    "radix_ranked_all": {"SBX_RCM_COUNT_SORT": "0", "SBX_DEBUG_RCM_RANKED_DIV": "100000"},
}
RADIX_MODES = [m for m in MODES if m.startswith("radix")]
PROFILED = ("default", "radix")  # these two run their list once more under the handle's profiler
LDS_SORT, REBUILD_BITS, COUNT_SORT_MAX = 4096, 32768, 1 << 20  # RCM_LDS_SORT, RCM_REBUILD_BITS, RCM_COUNT_SORT_MAX


# ---- graphs -----------------------------------------------------------------------------------------------------------
def _layered_edges(sizes, g, second=0.3, inside=None):
    """Vertices 0 .. sum(sizes) - 1 in layers of the given sizes.  Between neighbouring layers every vertex of the larger
    one gets a neighbour in the smaller one, the first of them one each (no vertex of either layer is left out, so the
    BFS levels from either end are the layers), and a fraction `second` of them a second one.  inside = {layer: k}: k
    random neighbours in its own layer for every vertex of that layer."""
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    layer = [np.arange(start[j], start[j + 1]) for j in range(len(sizes))]
    u, v = [], []
    for a, b in zip(layer[:-1], layer[1:]):
        big, small = (a, b) if len(a) >= len(b) else (b, a)
        pick = np.concatenate([g.permutation(len(small)), g.integers(0, len(small), len(big) - len(small))])
        u.append(big)
        v.append(small[pick])
        more = big[g.random(len(big)) < second]
        u.append(more)
        v.append(small[g.integers(0, len(small), len(more))])
    for j, k in (inside or {}).items():
        for _ in range(k):
            u.append(layer[j])
            v.append(layer[j][g.integers(0, len(layer[j]), len(layer[j]))])
    u, v = np.concatenate(u), np.concatenate(v)
    keep = u != v
    return int(start[-1]), u[keep], v[keep]


def _graph(parts, seed, isolated=0):
    """The parts side by side (one component each) and `isolated` empty rows, under shuffled labels; int32 CSR."""
    from sparsebase_amd import synth
    g = np.random.default_rng(seed)
    n, u, v = 0, [], []
    for sizes, kw in parts:
        cnt, pu, pv = _layered_edges(sizes, g, **kw)
        u.append(pu + n)
        v.append(pv + n)
        n += cnt
    n += isolated
    ids = g.permutation(n).astype(np.int64)
    return synth.csr_from_edges(n, *synth.symmetrize(ids[np.concatenate(u)], ids[np.concatenate(v)]))


def build_graph(name):
    from sparsebase_amd import synth
    if name == "layers":
        return _graph([([1] * 8 + [30, 9000, 33000, 60000, 5000, 300] + [1] * 8, {})], seed=11)
    if name == "lens":
        return _graph([([1, 1, 1, 200, 40000, 200, 1, 1, 1], {"inside": {4: 2}})], seed=12)
    if name == "lens_small":
        return _graph([([1, 1, 1, 200, 12000, 200, 1, 1, 1], {"inside": {4: 2}})], seed=13)
    if name == "star":
        return _graph([([1, 40000], {})], seed=14, isolated=3000)
    if name == "two_wide":
        return _graph([([1, 1, 1, 100, 9000, 100, 1, 1, 1], {}), ([1, 1, 1, 150, 10000, 150, 1, 1, 1], {})], seed=15)
    if name == "rmat16":
        return synth.rmat_symmetric(16, 8, seed=3)
    raise KeyError(name)


def graph_list(mode):
    """(graph, index type) pairs a mode's child runs; default and radix share one list (the profiler test compares them)."""
    if mode in ("radix_full_keys", "radix_ranked_all"):
        return [("layers", "int32"), ("layers", "int64"), ("lens", "int32"), ("star", "int32")]
    return [("layers", "int32"), ("layers", "int64"), ("lens", "int32"), ("lens_small", "int32"), ("lens_small", "int64"),
            ("star", "int32"), ("star", "int64"), ("two_wide", "int32"), ("rmat16", "int32")]


# ---- the child ----------------------------------------------------------------------------------------------------------
def child_main(mode):
    import torch
    from orc import Oracle
    from sparsebase_amd import ops
    orc = Oracle()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cases = []
    built = {}
    for name, dtype in graph_list(mode):
        if name not in built:
            built[name] = build_graph(name)
        rp, col = (a.astype(dtype) for a in built[name])
        cases.append((name, dtype, rp, col, orc.rcm_reorder(rp, col)))  # (the reference: computed once, reused below)
    torch.cuda.init()
    ops.handle_for(torch.device("cuda", 0))
    report = None
    t0 = time.perf_counter()
    for profiled in ((0, 1) if mode in PROFILED else (0,)):
        if profiled:
            ops.profile_enable(True)
        for name, dtype, rp, col, want in cases:
            sys.stderr.write("[graph] name=%s dtype=%s n=%d n_ranked=%d profiled=%d\n"
                             % (name, dtype, len(rp) - 1, int((np.diff(rp) > 0).sum()), profiled))
            sys.stderr.flush()
            got = ops.rcm_reorder(dev(rp), dev(col)).cpu().numpy()
            assert got.dtype == want.dtype and np.array_equal(got, want), \
                "%s / %s%s: the order differs from the reference's" % (name, dtype, " (profiled)" if profiled else "")
        if profiled:
            report = ops.profile_report()
            ops.profile_enable(False)
    took = time.perf_counter() - t0
    print("profile groups:", json.dumps(sorted(report) if report is not None else None))
    print("level-order child ok mode=%s graphs_seconds=%.2f" % (mode, took))


# ---- the parent ---------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^\[rcm level-path\] sweep=(cm|plain) level=(\d+) fsize=(\d+) nf=(\d+) route=([a-z_:]+) passes=(\d+) "
                  r"set_bits=([01]) mark_frontier=([01])$")
GRAPH = re.compile(r"^\[graph\] name=(\w+) dtype=(\w+) n=(\d+) n_ranked=(\d+) profiled=([01])$")


class Child:
    def __init__(self, mode):
        code = ("import sys; sys.path[:0] = [%r, %r]\n"
                "from test_rcm_level_order_gpu import child_main; child_main(%r)\n" % (ROOT, os.path.join(ROOT, "tests"), mode))
        env = dict(os.environ, SBX_DEBUG_RCM_LEVEL_PATHS="1", **MODES[mode])
        for name in {k for m in MODES.values() for k in m} - set(MODES[mode]):
            env.pop(name, None)  # (a mode is its own switches and no other mode's)
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        self.wall = time.perf_counter() - t0
        self.mode, self.stdout, self.stderr, self.returncode = mode, r.stdout, r.stderr, r.returncode
        self.levels = []  # one dict per traced level, with the graph it belongs to
        graph = None
        for line in r.stderr.splitlines():
            m = GRAPH.match(line)
            if m:
                graph = {"graph": m.group(1), "dtype": m.group(2), "n": int(m.group(3)), "n_ranked": int(m.group(4)),
                         "profiled": int(m.group(5))}
                continue
            if line.startswith("[rcm level-path]"):
                m = LINE.match(line)
                assert m and graph, "a trace line the parser does not know: %r" % line
                self.levels.append(dict(graph, sweep=m.group(1), level=int(m.group(2)), fsize=int(m.group(3)),
                                        nf=int(m.group(4)), route=m.group(5), passes=int(m.group(6)),
                                        set_bits=int(m.group(7)), mark_frontier=int(m.group(8)), text=line))
        groups = [l for l in r.stdout.splitlines() if l.startswith("profile groups:")]
        self.profile_groups = json.loads(groups[-1].split(":", 1)[1]) if groups else None
        print("level-order child %s: %.1f s wall; %s" % (mode, self.wall, r.stdout.strip().splitlines()[-1:] or ""))

    def trace(self):
        out, last = [], None
        for l in self.levels:
            head = "%s/%s n=%d n_ranked=%d%s" % (l["graph"], l["dtype"], l["n"], l["n_ranked"], " profiled" if l["profiled"] else "")
            if head != last:
                out.append("  " + head)
                last = head
            out.append("    " + l["text"])
        return "mode %s, trace:\n%s\n" % (self.mode, "\n".join(out))

    def seen(self, profiled=0, **want):
        """Traced levels (of the runs without the profiler) whose fields have these values; a callable is a predicate."""
        def ok(l):
            return all(v(l) if callable(v) else l[k] == v for k, v in want.items())
        return [l for l in self.levels if l["profiled"] == profiled and ok(l)]

    def need(self, what, **want):
        assert self.seen(**want), "mode %s: no level took %s\n%s" % (self.mode, what, self.trace())


_children = {}  # a mode's child runs once per session, whatever becomes of the assertions on it


def child(mode):
    if mode not in _children:
        _children[mode] = Child(mode)
    c = _children[mode]
    assert c.returncode == 0 and "level-order child ok" in c.stdout, c.stdout + c.stderr
    assert c.levels, "mode %s: SBX_DEBUG_RCM_LEVEL_PATHS printed nothing\n%s" % (mode, c.stderr)
    for l in c.levels:  # what holds on every route: the line is for a level above the one-workgroup sort's limit ...
        assert l["nf"] > LDS_SORT and l["fsize"] >= 1 and l["level"] >= 1, c.trace()
        # ... bits are set one by one exactly where no bitmap pass rebuilds them ...
        assert l["set_bits"] == (0 if l["nf"] >= max(REBUILD_BITS, l["n"] // 128) else 1), c.trace()
        # ... and the two families never mix within a process
        family = "count" if "SBX_RCM_COUNT_SORT" not in MODES[mode] and l["nf"] <= COUNT_SORT_MAX else "radix"
        assert l["route"].startswith(family + ":") or (family == "radix" and l["route"] == "emit_only"), c.trace()
    return c


def _cm_routes(c, **want):
    """The Cuthill-McKee sweeps' traced levels as a set (the plain sweeps' number may change when a grid barrier gives up)."""
    keys = ("graph", "level", "fsize", "nf", "route", "passes", "set_bits", "mark_frontier")
    got = {tuple(l[k] for k in keys) for l in c.seen(sweep="cm", **want)}
    assert got, c.trace()
    return got


def _counting_sort_routes(c):
    c.need("count:fresh_ranked in a Cuthill-McKee sweep", sweep="cm", route="count:fresh_ranked")
    c.need("count:scatter in a Cuthill-McKee sweep", sweep="cm", route="count:scatter")
    c.need("count:fresh_ranked below the bitmap pass", route="count:fresh_ranked", set_bits=1)
    c.need("count:fresh_ranked with the bitmap pass", route="count:fresh_ranked", set_bits=0)
    for passes in (1, 2):
        c.need("a counting sort of %d digit pass(es)" % passes, passes=passes)
    for mark in (0, 1):
        c.need("a level with mark_frontier=%d" % mark, mark_frontier=mark)
        c.need("a level with set_bits=1 and mark_frontier=%d" % mark, set_bits=1, mark_frontier=mark)
    for l in c.seen():  # 16 nf >= n_ranked is what separates the two routes of a Cuthill-McKee sweep
        if l["sweep"] == "cm":
            assert l["route"] == ("count:fresh_ranked" if 16 * l["nf"] >= l["n_ranked"] else "count:scatter"), c.trace()
    assert c.seen(dtype="int64"), c.trace()


def test_default_levels_take_the_counting_sort():
    _counting_sort_routes(child("default"))


def test_ordered_sweeps_take_the_counting_sort_too():
    c = child("ordered")
    _counting_sort_routes(c)
    c.need("count:fresh in a plain sweep", sweep="plain", route="count:fresh")
    c.need("count:scatter in a plain sweep", sweep="plain", route="count:scatter")
    for l in c.seen(sweep="plain"):
        assert l["route"] == ("count:scatter" if l["set_bits"] else "count:fresh"), c.trace()


def test_radix_routes_of_the_cuthill_mckee_sweep():
    c = child("radix")
    c.need("radix:fresh_ranked", sweep="cm", route="radix:fresh_ranked")
    c.need("radix:full with set_bits=1 (4097 ... 32767 vertices)", route="radix:full", set_bits=1,
           nf=lambda l: LDS_SORT < l["nf"] < REBUILD_BITS)
    c.need("radix:full with set_bits=0 (a bitmap pass and 3 nf < n_ranked)", route="radix:full", set_bits=0,
           nf=lambda l: 3 * l["nf"] < l["n_ranked"] and l["n_ranked"] > 3 * REBUILD_BITS)
    c.need("emit_only", route="emit_only", fsize=1, passes=0)
    for mark in (0, 1):
        c.need("a level with mark_frontier=%d" % mark, mark_frontier=mark)
        c.need("radix:full with set_bits=1 and mark_frontier=%d" % mark, route="radix:full", set_bits=1, mark_frontier=mark)
    c.need("radix:fresh_ranked with mark_frontier=1", route="radix:fresh_ranked", mark_frontier=1)
    for l in c.seen(sweep="cm"):
        ranked = l["set_bits"] == 0 and 3 * l["nf"] >= l["n_ranked"]
        assert l["route"] in (("radix:fresh_ranked", "emit_only") if ranked else ("radix:full",)), c.trace()
    for dtype in ("int32", "int64"):  # sbx_rcm.hip and sbx_rcm64.hip
        for route in ("radix:fresh_ranked", "radix:full", "emit_only"):
            c.need("%s with %s arrays" % (route, dtype), route=route, dtype=dtype)


def test_radix_routes_of_ordered_plain_sweeps():
    c = child("radix_ordered")
    c.need("radix:fresh in a plain sweep", sweep="plain", route="radix:fresh")
    c.need("radix:full in a plain sweep", sweep="plain", route="radix:full")
    for l in c.seen(sweep="plain"):
        assert l["route"] in (("radix:full",) if l["set_bits"] else ("radix:fresh", "emit_only")), c.trace()
    c.need("a plain sweep with int64 arrays", sweep="plain", dtype="int64")


def test_radix_full_keys_where_ranked_keys_would_run():
    c = child("radix_full_keys")
    c.need("radix:full with set_bits=0 on a level of at least n_ranked / 3", route="radix:full", set_bits=0,
           nf=lambda l: 3 * l["nf"] >= l["n_ranked"])
    c.need("the same with int64 arrays", route="radix:full", set_bits=0, dtype="int64", nf=lambda l: 3 * l["nf"] >= l["n_ranked"])
    assert not c.seen(route="radix:fresh_ranked"), c.trace()
    assert not [l for l in c.seen(sweep="cm") if l["route"] != "radix:full"], c.trace()


def test_radix_ranked_keys_on_every_bitmap_pass_level():
    c = child("radix_ranked_all")
    c.need("radix:fresh_ranked below n_ranked / 3", sweep="cm", route="radix:fresh_ranked", nf=lambda l: 3 * l["nf"] < l["n_ranked"])
    c.need("the same with int64 arrays", route="radix:fresh_ranked", dtype="int64", nf=lambda l: 3 * l["nf"] < l["n_ranked"])
    for l in c.seen(sweep="cm", set_bits=0):
        assert l["route"] == ("emit_only" if l["fsize"] == 1 else "radix:fresh_ranked"), c.trace()


def test_radix_pass_counts_and_index_widths_across_the_radix_modes():
    cs = [child(m) for m in RADIX_MODES]
    passes = {l["passes"] for c in cs for l in c.seen() if l["route"] != "emit_only"}
    everything = "".join(c.trace() for c in cs)
    assert 1 in passes and 2 in passes and max(passes) >= 3, everything
    for c in cs:  # the same graph takes the same routes whatever the width of its index arrays
        for name in {l["graph"] for l in c.seen(dtype="int64")}:
            assert _cm_routes(c, graph=name, dtype="int64") == _cm_routes(c, graph=name, dtype="int32"), c.trace()


def test_the_profiler_sees_the_radix_sort_only_with_the_counting_sort_off():
    """Not by the trace: under the handle's profiler the radix sort's kernels have groups of their own, and the RCM sorts
    by radix nowhere else at these sizes — none in the default child's report, both in the radix child's, same graphs."""
    d, r = child("default"), child("radix")
    assert graph_list("default") == graph_list("radix")
    assert d.profile_groups and r.profile_groups, (d.stdout, r.stdout)
    assert "level_order" in d.profile_groups and "level_order" in r.profile_groups, (d.profile_groups, r.profile_groups)
    assert not [g for g in d.profile_groups if g.startswith("radix")], d.profile_groups
    assert {"radix_hist", "radix_scatter"} <= set(r.profile_groups), r.profile_groups
    # (and the profiled calls took the routes of the unprofiled ones)
    for c in (d, r):
        assert _cm_routes(c, profiled=1) == _cm_routes(c), c.trace()
