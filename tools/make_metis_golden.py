"""Records tests/golden/metis_graph.npz: what the REAL reference's MetisGraphReader (io/metis_graph_reader.cc) reads and
what its MetisGraphWriter (io/metis_graph_writer.cc) writes, for the cases tests/test_metis_host.py checks the
restatement against (and tests/test_metis_gpu.py the ABI).

    python tools/make_metis_golden.py --ref /path/to/SparseBase

The reference is compiled header-only in a temporary directory (sparsebase/config.h derived from its own config.h.in, as
tools/make_text_writers_golden.py does) against a small driver whose text lives in this file.  Nothing compiled is
kept.  Floating-point values travel as hex floats both ways, so the bits are the ones the reference holds.

Reader cases hold only files for which the reference is defined: exactly 2 * m neighbours, no malformed token, no
neighbour given twice with different weights.  Per case k the file holds in_k (the input file's bytes) and row_k / col_k /
val_k / vw_k (what the Graph holds; val and vw where they exist), and in `cases` (JSON) the value type, the index mode,
n_dim, ncon and the exception's message ("" if none).  Writer cases hold row_k / col_k / val_k / vw_k (the Graph given)
and file_k (the bytes written).
"""
import argparse
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>
#include "sparsebase/format/array.h"
#include "sparsebase/format/coo.h"
#include "sparsebase/io/metis_graph_reader.h"
#include "sparsebase/io/metis_graph_writer.h"
#include "sparsebase/object/object.h"
#include "sparsebase/utils/exception.h"
using namespace sparsebase;
static std::string word() { char b[256]; if (scanf("%255s", b) != 1) exit(2); return b; }
template <typename V> static void put(V v) {
  if constexpr (std::is_floating_point_v<V>) printf(" %a", (double)v); else printf(" %lld", (long long)v);
}
// R <vt> <zero> <path>:  prints  "G n_dim nnz ncon hasval hasvw", rows, cols, vals, vertex weights (one line each)
template <typename V> static void read_case(int zero, const char *path) {
  io::MetisGraphReader<int, int, V> reader(path, zero != 0);
  auto *g = reader.ReadGraph();
  auto *coo = g->get_connectivity()->template AsAbsolute<format::COO<int, int, V>>();
  const int n = (int)coo->get_dimensions()[0], nnz = (int)coo->get_num_nnz();
  bool hasval = false, hasvw = false;
  if constexpr (!std::is_same_v<V, void>) { hasval = coo->get_vals() != nullptr; hasvw = g->vertexWeights_ != nullptr; }
  printf("G %d %d %d %d %d\n", n, nnz, (int)g->ncon_, hasval ? 1 : 0, hasvw ? 1 : 0);
  for (int i = 0; i < nnz; i++) printf(" %d", coo->get_row()[i]);
  printf("\n");
  for (int i = 0; i < nnz; i++) printf(" %d", coo->get_col()[i]);
  printf("\n");
  if constexpr (!std::is_same_v<V, void>) {
    if (hasval) for (int i = 0; i < nnz; i++) put(coo->get_vals()[i]);
    printf("\n");
    if (hasvw) for (int v = 0; v < n; v++) for (int j = 0; j < (int)g->ncon_; j++) put(g->vertexWeights_[v]->get_vals()[j]);
    printf("\n");
  } else {
    printf("\n\n");
  }
}
// W <vt> <ew> <vw> <zero> <path>, stdin: n_dim nnz ncon hasval hasvw row[] col[] val[] vw[]
template <typename V> static void write_case(int ew, int vw, int zero, const char *path) {
  const int n = atoi(word().c_str()), nnz = atoi(word().c_str()), ncon = atoi(word().c_str());
  const int hasval = atoi(word().c_str()), hasvw = atoi(word().c_str());
  int *row = new int[nnz + 1], *col = new int[nnz + 1];
  for (int i = 0; i < nnz; i++) row[i] = atoi(word().c_str());
  for (int i = 0; i < nnz; i++) col[i] = atoi(word().c_str());
  if constexpr (std::is_same_v<V, void>) {
    object::Graph<int, int, void> g(new format::COO<int, int, void>(n, n, nnz, row, col, nullptr));
    io::MetisGraphWriter<int, int, void>(path, ew != 0, vw != 0, zero != 0).WriteGraph(&g);
  } else {
    V *val = nullptr;
    if (hasval) { val = new V[nnz + 1]; for (int i = 0; i < nnz; i++) val[i] = (V)strtod(word().c_str(), nullptr); }
    format::Array<V> **weights = nullptr;
    if (hasvw) {
      weights = new format::Array<V> *[n];
      for (int v = 0; v < n; v++) {
        V *w = new V[ncon + 1];
        for (int j = 0; j < ncon; j++) w[j] = (V)strtod(word().c_str(), nullptr);
        weights[v] = new format::Array<V>(ncon > 0 ? ncon : 1, w);
      }
    }
    object::Graph<int, int, V> g(new format::COO<int, int, V>(n, n, nnz, row, col, val), ncon, weights);
    io::MetisGraphWriter<int, int, V>(path, ew != 0, vw != 0, zero != 0).WriteGraph(&g);
  }
  printf("OK\n");
}
template <typename V> static void one(int argc, char **argv) {
  try {
    if (argv[1][0] == 'R') read_case<V>(atoi(argv[3]), argv[4]);
    else write_case<V>(atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), argv[6]);
  } catch (utils::Exception &e) {
    printf("EXC %s\n", e.what());
  }
}
int main(int argc, char **argv) {
  const char vt = argv[2][0];
  if (vt == 'v') one<void>(argc, argv);
  else if (vt == 'i') one<int>(argc, argv);
  else if (vt == 'f') one<float>(argc, argv);
  else one<double>(argc, argv);
  return 0;
}
"""

DTYPES = {"void": None, "int": np.int32, "float": np.float32, "double": np.float64}
VTYPES = ("int", "float", "double", "void")

# the two files of the reference's own tests (tiny_03 / tiny_04 of the METIS manual), kept as fixtures
TINY_03 = open(os.path.join(ROOT, "tests", "golden", "metis_tiny_03.graph"), "rb").read()
TINY_04 = open(os.path.join(ROOT, "tests", "golden", "metis_tiny_04.graph"), "rb").read()


def random_graph(g, n, p, isolated=()):
    """Symmetric adjacency lists (1-based neighbours, ascending) of a random graph; `isolated` vertices get no edge."""
    adj = [[] for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            if i not in isolated and j not in isolated and g.random() < p:
                adj[i].append(j + 1)
                adj[j].append(i + 1)
    return adj


def graph_text(adj, header_tail="", eweights=None, vweights=None, sep=" ", eol="\n", shuffle=None, last_eol=True,
               drop_trailing=0):
    """A METIS file of the adjacency lists: eweights {(i, j): token} for i < j (1-based), vweights per vertex a list of
    tokens; `shuffle` (a Generator) permutes every neighbour list; drop_trailing leaves the last (empty) lines out."""
    n, m = len(adj), sum(len(a) for a in adj) // 2
    lines = [f"{n} {m}{header_tail}"]
    rows = adj[:len(adj) - drop_trailing]
    for i, a in enumerate(rows):
        a = list(a)
        if shuffle is not None:
            shuffle.shuffle(a)
        toks = list(vweights[i]) if vweights is not None else []
        for j in a:
            toks.append(str(j))
            if eweights is not None:
                toks.append(eweights[(min(i + 1, j), max(i + 1, j))])
        lines.append(sep.join(toks))
    text = eol.join(lines) + (eol if last_eol else "")
    return text.encode()


def reader_inputs():
    g = np.random.default_rng(11)
    out = []
    add = lambda name, data, vts=VTYPES: out.extend((name, data, vt, zero) for vt in vts for zero in (False, True))
    add("tiny_03", TINY_03)
    add("tiny_04", TINY_04)
    adj = random_graph(g, 9, 0.4, isolated=(3, 8))
    ew = {(i + 1, j): str(int(g.integers(1, 50))) for i in range(9) for j in adj[i] if i + 1 < j}
    fw = dict(zip(sorted(ew), ["0.1", "1e-5", "123456.7", "2.5", "-3", "1E+3", "0.333333343", "7", "12.75", "1e10"] * 4))
    vw2 = [[str(int(g.integers(0, 9))), str(int(g.integers(0, 9)))] for _ in range(9)]
    vw3 = [[str(int(g.integers(0, 9))) for _ in range(3)] for _ in range(9)]
    plain = graph_text(adj)
    add("comments", b"% a comment\n%another\n" + plain.replace(b"\n", b"\n% between the lines 1 2 3\n", 3))
    add("fmt_0", graph_text(adj, " 0"))
    add("fmt_1", graph_text(adj, " 1", eweights=ew))
    add("fmt_001", graph_text(adj, " 001", eweights=ew))
    add("fmt_10_2", graph_text(adj, " 10 2", vweights=vw2))
    add("fmt_011", graph_text(adj, " 011", eweights=ew, vweights=[v[:1] for v in vw2]))
    add("fmt_11_3", graph_text(adj, " 11 3", eweights=ew, vweights=vw3))
    add("fmt_10_alone", graph_text(adj, " 10"))
    add("fmt_1_ncon", graph_text(adj, " 1 2", eweights=ew))
    add("blank_and_trailing", graph_text(adj, drop_trailing=1))         # vertex 4 is a blank line, vertex 9 has no line
    add("crlf_tabs", graph_text(adj, " 1", eweights=ew, sep="\t", eol="\r\n"))
    add("no_final_newline", graph_text(adj, last_eol=False))
    add("float_weights", graph_text(adj, " 1", eweights=fw), ("float", "double"))
    add("float_vertex_weights", graph_text(adj, " 11 2", eweights=fw, vweights=[["0.5", "1e-3"]] * 9), ("float", "double"))
    add("unsorted", graph_text(adj, " 1", eweights=ew, shuffle=g))
    for k, (n, p) in enumerate(((40, 0.1), (41, 0.2), (39, 0.05))):
        a = random_graph(g, n, p)
        w = {(i + 1, j): str(int(g.integers(-99, 99))) for i in range(n) for j in a[i] if i + 1 < j}
        vw = [[str(int(g.integers(0, 99)))] for _ in range(n)]
        add(f"random_{k}", graph_text(a, " 11", eweights=w, vweights=vw, shuffle=g if k else None), ("int", "double", "void"))
    return out


def writer_inputs():
    g = np.random.default_rng(12)
    out = []
    adj = random_graph(g, 10, 0.35, isolated=(0, 4, 9))                   # empty rows: the first, one inside, the last
    for vt in VTYPES:
        for zero in (False, True):
            base = 0 if zero else 1
            n_dim = 10 + base
            row = np.array([i + base for i in range(10) for _ in adj[i]], np.int32)
            col = np.array([j - 1 + base for i in range(10) for j in adj[i]], np.int32)
            dt = DTYPES[vt]
            if dt is None:
                out.append(dict(vtype=vt, zero=zero, ew=False, vw=False, n_dim=n_dim, ncon=0, row=row, col=col, val=None, vw_arr=None))
                continue
            if dt == np.int32:
                val = g.integers(-999, 999, len(row)).astype(dt)
                vwa = g.integers(0, 99, (n_dim, 3)).astype(dt)
            else:
                val = (g.integers(-999999, 999999, len(row)) / 1000.0 * 10.0 ** g.integers(-7, 9, len(row))).astype(dt)
                val[:5] = np.array([0.1, 1e-5, 123456.7, 1e10, 1.0 / 3.0], dt)
                vwa = (g.integers(0, 9999, (n_dim, 3)) / 100.0).astype(dt)
            for ew in (False, True):
                for vw in (False, True):
                    out.append(dict(vtype=vt, zero=zero, ew=ew, vw=vw, n_dim=n_dim, ncon=2, row=row, col=col, val=val,
                                    vw_arr=vwa[:, :2].copy()))
            if vt == "float":
                for ncon in (0, 1, 3):
                    out.append(dict(vtype=vt, zero=zero, ew=zero, vw=True, n_dim=n_dim, ncon=ncon, row=row, col=col,
                                    val=val, vw_arr=vwa[:, :ncon].copy()))
    return out


def _num(v):
    return float(v).hex() if isinstance(v, (np.floating, float)) else str(int(v))


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
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-fopenmp", "-I", os.path.join(tmp, "cfg"), "-I",
                           os.path.join(ref, "src"), src, "-o", exe])
    return exe


def _parse_numbers(line, dtype):
    toks = line.split()
    if dtype in (np.float32, np.float64):
        return np.array([float.fromhex(t) for t in toks], dtype)
    return np.array([int(t) for t in toks], dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a SparseBase source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "metis_graph.npz"))
    a = ap.parse_args()
    data, meta = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(a.ref, tmp)
        path = os.path.join(tmp, "case.graph")
        k = 0
        for name, text, vt, zero in reader_inputs():
            with open(path, "wb") as f:
                f.write(text)
            res = subprocess.run([exe, "R", vt, "1" if zero else "0", path], capture_output=True, text=True, check=True).stdout
            lines = res.split("\n")
            while lines and not lines[0].startswith("G "):  # (the reference logs its warnings to the same stream)
                lines.pop(0)
            assert lines, res
            head = lines[0].split()
            n_dim, nnz, ncon, hasval, hasvw = (int(x) for x in head[1:])
            dt = DTYPES[vt]
            data[f"in_{k}"] = np.frombuffer(text, np.uint8)
            data[f"row_{k}"] = _parse_numbers(lines[1], np.int32)
            data[f"col_{k}"] = _parse_numbers(lines[2], np.int32)
            assert len(data[f"row_{k}"]) == nnz
            if hasval:
                data[f"val_{k}"] = _parse_numbers(lines[3], dt)
            if hasvw:
                data[f"vw_{k}"] = _parse_numbers(lines[4], dt).reshape(n_dim, ncon)
            meta.append(dict(kind="read", name=name, vtype=vt, zero=zero, n_dim=n_dim, ncon=ncon, message=""))
            k += 1
        res = subprocess.run([exe, "R", "i", "0", os.path.join(tmp, "no_such.graph")], capture_output=True, text=True,
                             check=True).stdout.strip()
        assert res.startswith("EXC "), res
        data[f"in_{k}"] = np.zeros(0, np.uint8)
        meta.append(dict(kind="read_missing", name="missing_file", vtype="int", zero=False, n_dim=0, ncon=0, message=res[4:]))
        k += 1
        for c in writer_inputs():
            if os.path.exists(path):
                os.remove(path)
            hasval, hasvw = c["val"] is not None, c["vw_arr"] is not None
            text = "%d %d %d %d %d\n%s\n%s\n%s\n%s\n" % (
                c["n_dim"], len(c["row"]), c["ncon"], hasval, hasvw, " ".join(str(int(x)) for x in c["row"]),
                " ".join(str(int(x)) for x in c["col"]), " ".join(_num(x) for x in c["val"]) if hasval else "",
                " ".join(_num(x) for x in c["vw_arr"].ravel()) if hasvw else "")
            res = subprocess.run([exe, "W", c["vtype"], str(int(c["ew"])), str(int(c["vw"])), str(int(c["zero"])), path],
                                 input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")[-1]
            assert res == "OK", res
            data[f"file_{k}"] = np.frombuffer(open(path, "rb").read(), np.uint8)
            data[f"row_{k}"], data[f"col_{k}"] = c["row"], c["col"]
            if hasval:
                data[f"val_{k}"] = c["val"]
            if hasvw:
                data[f"vw_{k}"] = c["vw_arr"]
            meta.append(dict(kind="write", vtype=c["vtype"], zero=c["zero"], ew=c["ew"], vw=c["vw"], n_dim=c["n_dim"],
                             ncon=c["ncon"], message=""))
            k += 1
    data["cases"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(a.out, **data)
    print(a.out, os.path.getsize(a.out), "bytes,", len(meta), "cases")


if __name__ == "__main__":
    main()
