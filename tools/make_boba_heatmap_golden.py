"""Records tests/golden/boba_heatmap.npz: outputs of the REAL reference's BOBAReorder (reorder/boba_reorder.cc) and
ReorderHeatmap (reorder/reorder_heatmap.cc) for the inputs tests/test_boba_host.py and tests/test_reorder_heatmap_host.py
check their restatements against.

    python tools/make_boba_heatmap_golden.py --ref /path/to/SparseBase

The reference is compiled header-only in a temporary directory, with sparsebase/config.h derived from its own
config.h.in the way oracle/Makefile does, against a small driver whose text lives in this file.  Nothing compiled is
kept.  BOBA is recorded in both modes; the parallel one runs with OMP_NUM_THREADS=1, where its unguarded minimum
(boba_reorder.cc:119-124) cannot race.  The heatmap's CSR is built from row-sorted entries (the reference's COO -> CSR
conversion assumes sorted rows).

Inputs: the reference tests' 3-vertex graph, ash958 (958 x 292, the reference's examples/data: nodes = max(n, m)
matters) and a dozen messy COOs (unsorted, duplicates, self loops, ids in [n, m), isolated vertices, nnz = 0).
Heatmaps (float) of ash958 and the messy graphs under the identity, degree and random orders, b in {1, 2, 3, 7, min(n, m)}.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "sparsebase/context/cpu_context.h"
#include "sparsebase/format/array.h"
#include "sparsebase/format/coo.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/reorder/boba_reorder.h"
#include "sparsebase/reorder/reorder_heatmap.h"
// stdin, until EOF, cases of either kind:
//   B n m nnz sequential row[nnz] col[nnz]                      -> "=inv" x max(n, m), then "."
//   H n m nnz b row_ptr[n + 1] col[nnz] order_r[n] order_c[m]   -> "=%a" x b * b, then "."
int main() {
  char kind;
  sparsebase::context::CPUContext cpu;
  while (scanf(" %c", &kind) == 1) {
    int n, m, nnz, p;
    if (scanf("%d %d %d %d", &n, &m, &nnz, &p) != 4) return 2;
    if (kind == 'B') {
      std::vector<int> row(nnz + 1), col(nnz + 1), val(nnz + 1, 1);
      for (int i = 0; i < nnz; i++) if (scanf("%d", &row[i]) != 1) return 2;
      for (int i = 0; i < nnz; i++) if (scanf("%d", &col[i]) != 1) return 2;
      sparsebase::format::COO<int, int, int> coo(n, m, nnz, row.data(), col.data(), val.data(),
                                                 sparsebase::format::kNotOwned, true);
      sparsebase::reorder::BOBAReorder<int, int, int> boba(p != 0);
      int *inv = boba.GetReorder(&coo, {&cpu}, true);
      for (int i = 0; i < (n > m ? n : m); i++) printf("=%d\n", inv[i]);
      delete[] inv;
    } else {
      std::vector<int> rp(n + 1), col(nnz + 1), val(nnz + 1, 1), orr(n + 1), orc(m + 1);
      for (int i = 0; i <= n; i++) if (scanf("%d", &rp[i]) != 1) return 2;
      for (int i = 0; i < nnz; i++) if (scanf("%d", &col[i]) != 1) return 2;
      for (int i = 0; i < n; i++) if (scanf("%d", &orr[i]) != 1) return 2;
      for (int i = 0; i < m; i++) if (scanf("%d", &orc[i]) != 1) return 2;
      sparsebase::format::CSR<int, int, int> csr(n, m, rp.data(), col.data(), val.data(),
                                                 sparsebase::format::kNotOwned, true);
      sparsebase::format::Array<int> ar(n, orr.data(), sparsebase::format::kNotOwned);
      sparsebase::format::Array<int> ac(m, orc.data(), sparsebase::format::kNotOwned);
      sparsebase::reorder::ReorderHeatmap<int, int, int, float> hm(p);
      auto *out = hm.Get(&csr, &ar, &ac, {&cpu}, true);
      const float *v = out->As<sparsebase::format::Array>()->get_vals();
      for (int i = 0; i < p * p; i++) printf("=%a\n", v[i]);
      delete out;
    }
    printf(".\n");
  }
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


def run_cases(exe, text, threads=None):
    env = dict(os.environ)
    if threads:
        env["OMP_NUM_THREADS"] = str(threads)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, env=env).stdout
    cases, cur = [], []
    for line in out.split("\n"):
        if line.startswith("="):
            cur.append(line[1:])
        elif line == ".":
            cases.append(cur)
            cur = []
    return cases


def ints(a):
    return " ".join(str(int(x)) for x in a)


def main():
    from test_boba_host import messy_coos
    from test_reorder_heatmap_host import csr_of, heat_shape, orders_for
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a SparseBase source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "boba_heatmap.npz"))
    a = ap.parse_args()
    from make_slashburn_golden import ash958
    rp, col, m = ash958(a.ref)
    n = len(rp) - 1
    ash_row = np.repeat(np.arange(n), np.diff(rp))
    graphs = [("ref3", np.array([0, 0, 1, 2]), np.array([1, 2, 0, 0]), 3, 3),
              ("ash958", ash_row, col, n, m)] + messy_coos()
    data, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(a.ref, tmp)
        for seq in (1, 0):
            text = "".join("B %d %d %d %d\n%s\n%s\n" % (gn, gm, len(r), seq, ints(r), ints(c))
                           for _, r, c, gn, gm in graphs)
            for (name, r, c, gn, gm), inv in zip(graphs, run_cases(exe, text, threads=1 if seq == 0 else None)):
                data["%s/boba_%s" % (name, "seq" if seq else "par")] = np.array(inv, np.int32)
        heat_cases = []
        for name, r, c, gn, gm in graphs[1:]:
            hn, hm = heat_shape(r, c, gn, gm)
            crp, ccol = csr_of(r, c, hn)
            bs = sorted({b for b in (1, 2, 3, 7, min(hn, hm)) if b <= min(hn, hm)})
            for oname, orr, orc in orders_for(crp, ccol, hn, hm, seed=len(heat_cases)):
                for b in bs:
                    heat_cases.append((name, oname, crp, ccol, hn, hm, orr, orc, b))
        text = "".join("H %d %d %d %d\n%s\n%s\n%s\n%s\n" % (gn, gm, len(ccol), b, ints(crp), ints(ccol), ints(orr), ints(orc))
                       for _, _, crp, ccol, gn, gm, orr, orc, b in heat_cases)
        outs = run_cases(exe, text)
    for name, r, c, gn, gm in graphs:
        names.append(name)
        data[name + "/row"] = np.asarray(r, np.int32)
        data[name + "/col"] = np.asarray(c, np.int32)
        data[name + "/shape"] = np.array([gn, gm], np.int64)
    hm = {}
    for (name, oname, crp, ccol, gn, gm, orr, orc, b), vals in zip(heat_cases, outs):
        key = "%s/heat/%s" % (name, oname)
        hm.setdefault(key, []).append((b, np.array([float.fromhex(v) for v in vals], np.float32)))
        data[key + "/order_r"] = np.asarray(orr, np.int32)
        data[key + "/order_c"] = np.asarray(orc, np.int32)
    for key, lst in hm.items():
        data[key + "/bs"] = np.array([b for b, _ in lst], np.int64)
        data[key + "/vals"] = np.concatenate([v for _, v in lst])
    np.savez_compressed(a.out, names=np.array(names), **data)
    print(a.out, os.path.getsize(a.out), "bytes,", len(graphs), "graphs,", len(heat_cases), "heatmaps")


if __name__ == "__main__":
    main()
