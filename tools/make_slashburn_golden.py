"""Records tests/golden/slashburn.npz: inverse permutations of the REAL reference's SlashburnReorder
(reorder/slashburn_reorder.cc) for the graphs tests/test_slashburn_host.py checks its transcription against.

    python tools/make_slashburn_golden.py [--ref /path/to/reference]

The reference is compiled header-only in a temporary directory, with sparsebase/config.h derived from its own
config.h.in the way oracle/Makefile does, against a small driver whose text lives in this file.  The driver runs as
one process per call: the reference keeps greedy / hub_order in process globals that a call sets and never clears, so
every recorded call starts from a fresh process (the value the device computes).  Nothing compiled is kept.

Graphs: the reference test's 3-vertex graph and ash958 (958 x 292, the reference's examples/data) with k in {1, 10}
and all four flag combinations, and a dozen messy graphs (unsorted rows, duplicates, self loops, asymmetric patterns,
isolated vertices, several components, k >= n).
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "sparsebase/context/cpu_context.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/reorder/slashburn_reorder.h"
// stdin: n m nnz k greedy hub_order, row_ptr[n + 1], col[nnz]; stdout: inv[n]
int main() {
  int n, m, nnz, k, greedy, hub_order;
  if (scanf("%d %d %d %d %d %d", &n, &m, &nnz, &k, &greedy, &hub_order) != 6) return 2;
  std::vector<int> rp(n + 1), col(nnz > 0 ? nnz : 1), val(nnz > 0 ? nnz : 1, 1);
  for (int i = 0; i <= n; i++) if (scanf("%d", &rp[i]) != 1) return 2;
  for (int i = 0; i < nnz; i++) if (scanf("%d", &col[i]) != 1) return 2;
  // ignore_sort: GetReorderCSR sees the rows in their stored order, as the C ABI does
  sparsebase::format::CSR<int, int, int> csr(n, m, rp.data(), col.data(), val.data(), sparsebase::format::kNotOwned,
                                             true);
  sparsebase::context::CPUContext cpu;
  sparsebase::reorder::SlashburnReorder<int, int, int> sb(k, greedy != 0, hub_order != 0);
  int *inv = sb.GetReorder(&csr, {&cpu}, true);
  for (int i = 0; i < n; i++) printf("=%d\n", inv[i]);
  return 0;
}
"""


def build_driver(ref, tmp):
    cfg = os.path.join(tmp, "cfg", "sparsebase")
    os.makedirs(cfg)
    with open(os.path.join(ref, "src", "sparsebase", "config.h.in")) as f, open(os.path.join(cfg, "config.h"), "w") as o:
        for line in f:
            if line.startswith("#cmakedefine _HEADER_ONLY"):
                line = line.replace("#cmakedefine", "#define", 1)
            elif line.startswith("#cmakedefine "):
                line = "/* #undef %s */\n" % line[len("#cmakedefine "):].strip()
            o.write(line)
    src = os.path.join(tmp, "driver.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-fopenmp", "-I", os.path.join(tmp, "cfg"), "-I",
                           os.path.join(ref, "src"), src, "-o", exe])
    return exe


def run(exe, rp, col, m, k, greedy, hub_order):
    n = len(rp) - 1
    text = "%d %d %d %d %d %d\n%s\n%s\n" % (n, m, len(col), k, greedy, hub_order, " ".join(map(str, rp)),
                                           " ".join(map(str, col)))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    return np.array([int(x[1:]) for x in out.split("\n") if x.startswith("=")], np.int32)


def ash958(ref):
    rows, cols = [], []
    with open(os.path.join(ref, "examples", "data", "ash958.mtx")) as f:
        lines = [l for l in f if not l.startswith("%")]
    n, m, _ = map(int, lines[0].split())
    for l in lines[1:]:
        r, c = l.split()[:2]
        rows.append(int(r) - 1)
        cols.append(int(c) - 1)
    o = np.lexsort((cols, rows))
    rows, cols = np.array(rows)[o], np.array(cols)[o]
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp), cols, m


def messy_graphs():
    from test_slashburn_host import csr_from_pairs, random_messy_graph
    g = np.random.default_rng(20261016)
    out = []
    # unsorted rows with duplicates and self loops, asymmetric
    out.append(("unsorted_dups", *csr_from_pairs(6, [0, 0, 0, 2, 2, 2, 5, 5, 3], [3, 1, 3, 2, 5, 0, 1, 5, 3])))
    # a directed path: only S connects it
    out.append(("directed_path", *csr_from_pairs(8, list(range(7)), list(range(1, 8)))))
    # star with centre 0 stored one way, plus isolated vertices
    out.append(("star_one_way", *csr_from_pairs(12, [0] * 8, list(range(1, 9)))))
    # several components of equal size (tie rules)
    e = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (9, 10), (10, 8)]
    out.append(("equal_components", *csr_from_pairs(11, [a for a, b in e] + [b for a, b in e],
                                                     [b for a, b in e] + [a for a, b in e])))
    # two hubs joined by spokes of several sizes
    src, dst = [], []
    for v in range(2, 20):
        src += [0 if v % 2 else 1]
        dst += [v]
    src += [2, 4, 6, 7, 12, 13]
    dst += [3, 5, 7, 8, 13, 14]
    out.append(("two_hubs", *csr_from_pairs(20, src + dst, dst + src)))
    for i, (n, e, sym) in enumerate([(9, 20, False), (14, 30, True), (17, 45, False), (25, 60, True), (30, 70, False),
                                     (40, 120, True), (13, 8, False)]):
        out.append(("random_%d" % i, *random_messy_graph(g, n, e, symmetric=sym)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "slashburn.npz"))
    a = ap.parse_args()
    flags = [(g, h) for g in (0, 1) for h in (0, 1)]
    data, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(a.ref, tmp)
        graphs = [("ref3", np.array([0, 2, 3, 4]), np.array([1, 2, 0, 0]), 3, (1, 10)),
                  ("ash958", *ash958(a.ref), (1, 10))]
        for name, rp, col in messy_graphs():
            n = len(rp) - 1
            graphs.append((name, rp, col, n, sorted({1, 2, 3, -(-n * 5 // 100), n, n + 5})))
        for name, rp, col, m, ks in graphs:
            cases, invs = [], []
            for k in ks:
                for greedy, hub in flags:
                    cases.append((k, greedy, hub))
                    invs.append(run(exe, rp, col, m, k, greedy, hub))
            names.append(name)
            data[name + "/rp"] = np.asarray(rp, np.int32)
            data[name + "/col"] = np.asarray(col, np.int32)
            data[name + "/cases"] = np.asarray(cases, np.int32)
            data[name + "/inv"] = np.stack(invs)
            print(name, len(rp) - 1, len(col), len(cases))
    np.savez_compressed(a.out, names=np.array(names), **data)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
