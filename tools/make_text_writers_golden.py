"""Records tests/golden/text_writers.npz: what the REAL reference's MTXWriter (io/mtx_writer.cc) and EdgeListWriter
(io/edge_list_writer.cc) write, and the messages they throw, for the cases tests/test_text_writers_host.py checks the
restatement and the transcription against (and tests/test_text_writers_gpu.py the ABI).

    python tools/make_text_writers_golden.py --ref /path/to/SparseBase

The reference is compiled header-only in a temporary directory (sparsebase/config.h derived from its own config.h.in,
as tools/make_boba_heatmap_golden.py does) against a small driver whose text lives in this file.  Nothing compiled is
kept.  Floating-point inputs travel as hex floats, so the driver sees the bits this file holds.

The file holds, per case k: row_k / col_k / val_k (the inputs that exist), file_k (the bytes of the file the reference
left, which after a throw is the banner alone or nothing) and in `cases` (JSON) the options, whether a file was left
and the exception's message ("" if none).  Undirected edge lists hold no duplicate whose surviving weight the
reference's std::sort would leave open: mirrored pairs carry equal weights.
"""
import argparse
import json
import os
import subprocess
import sys
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
#include "sparsebase/io/edge_list_writer.h"
#include "sparsebase/io/mtx_writer.h"
#include "sparsebase/utils/exception.h"
using namespace sparsebase;
static std::string word() { char b[256]; if (scanf("%255s", b) != 1) exit(2); return b; }
template <typename V> static void read_vals(std::vector<V> &v, int count) {
  for (int i = 0; i < count; i++) v[i] = (V)strtod(word().c_str(), nullptr);
}
// stdin, until EOF:  M <n> <m> <nnz> <hasvals> <object> <format> <field> <symmetry> row[] col[] val[]
//                    A <count> <object> <format> <field> <symmetry> val[]
//                    E <n> <m> <nnz> <hasvals> <directed> row[] col[] val[]
// stdout per case: "OK" or "EXC <message>"
template <typename V> static void one(char kind, const char *path) {
  try {
    if (kind == 'A') {
      int count = atoi(word().c_str());
      std::string o = word(), f = word(), fi = word(), s = word();
      if constexpr (std::is_same_v<V, void>) {
        io::MTXWriter<int, int, void> w(path, o, f, fi, s);
        format::Array<void> *arr = nullptr;
        w.WriteArray(arr);
      } else {
        std::vector<V> v(count + 1);
        read_vals(v, count);
        format::Array<V> arr(count, v.data(), format::kNotOwned);
        io::MTXWriter<int, int, V> w(path, o, f, fi, s);
        w.WriteArray(&arr);
      }
    } else {
      int n = atoi(word().c_str()), m = atoi(word().c_str()), nnz = atoi(word().c_str()), hasvals = atoi(word().c_str());
      std::string o, f, fi, s;
      int directed = 1;
      if (kind == 'M') { o = word(); f = word(); fi = word(); s = word(); }
      else directed = atoi(word().c_str());
      std::vector<int> row(nnz + 1), col(nnz + 1);
      for (int i = 0; i < nnz; i++) row[i] = atoi(word().c_str());
      for (int i = 0; i < nnz; i++) col[i] = atoi(word().c_str());
      if constexpr (std::is_same_v<V, void>) {
        format::COO<int, int, void> coo(n, m, nnz, row.data(), col.data(), nullptr, format::kNotOwned, true);
        if (kind == 'M') io::MTXWriter<int, int, void>(path, o, f, fi, s).WriteCOO(&coo);
        else io::EdgeListWriter<int, int, void>(path, directed != 0).WriteCOO(&coo);
      } else {
        std::vector<V> v(nnz + 1);
        if (hasvals) read_vals(v, nnz);
        format::COO<int, int, V> coo(n, m, nnz, row.data(), col.data(), hasvals ? v.data() : nullptr, format::kNotOwned, true);
        if (kind == 'M') io::MTXWriter<int, int, V>(path, o, f, fi, s).WriteCOO(&coo);
        else io::EdgeListWriter<int, int, V>(path, directed != 0).WriteCOO(&coo);
      }
    }
    printf("OK\n");
  } catch (utils::Exception &e) {
    printf("EXC %s\n", e.what());
  }
}
int main(int argc, char **argv) {
  char kind, vt;
  while (scanf(" %c %c", &kind, &vt) == 2) {
    if (vt == 'v') one<void>(kind, argv[1]);
    else if (vt == 'i') one<int>(kind, argv[1]);
    else if (vt == 'f') one<float>(kind, argv[1]);
    else one<double>(kind, argv[1]);
    fflush(stdout);
  }
  return 0;
}
"""

DTYPES = {"void": None, "int": np.int32, "float": np.float32, "double": np.float64}


def _vals_text(v):
    if v is None:
        return ""
    if v.dtype.kind == "f":
        return " ".join(float(x).hex() for x in v)
    return " ".join(str(int(x)) for x in v)


def case_text(c):
    code = c["vtype"][0]
    ints = lambda a: " ".join(str(int(x)) for x in a)
    if c["kind"] == "array":
        return "A %s %d %s %s %s %s\n%s\n" % (code, 0 if c["val"] is None else len(c["val"]), c["object"], c["format"],
                                             c["field"], c["symmetry"], _vals_text(c["val"]))
    head = "%d %d %d %d" % (c["n"], c["m"], len(c["row"]), 0 if c["val"] is None else 1)
    if c["kind"] == "mtx":
        head = "M %s %s %s %s %s %s" % (code, head, c["object"], c["format"], c["field"], c["symmetry"])
    else:
        head = "E %s %s %d" % (code, head, 1 if c["directed"] else 0)
    return "%s\n%s\n%s\n%s\n" % (head, ints(c["row"]), ints(c["col"]), _vals_text(c["val"]))


def cases():
    """The inputs: every format, field, symmetry and value type, the refusals, both kinds of edge list."""
    g = np.random.default_rng(7)
    out = []

    def vals(vtype, count, sym_pairs=None):
        dt = DTYPES[vtype]
        if dt is None:
            return None
        if dt == np.int32:
            return g.integers(-99999, 99999, count).astype(dt)
        mags = 10.0 ** g.integers(-7, 9, count)
        v = (g.integers(-999999, 999999, count) / 1000.0 * mags).astype(dt)
        v[:min(count, 6)] = np.array([0.1, 1e-5, 123456.7, 1e10, -2.5, 1.0 / 3.0], dt)[:min(count, 6)]
        return v

    def mtx(vtype, n, m, row, col, val, fmt="coordinate", field="real", sym="general", obj="matrix"):
        out.append(dict(kind="mtx", vtype=vtype, n=n, m=m, row=np.asarray(row, np.int32), col=np.asarray(col, np.int32),
                        val=val, object=obj, format=fmt, field=field, symmetry=sym))

    def general(vtype, n, m, nnz, **kw):
        row, col = g.integers(0, n, nnz), g.integers(0, m, nnz)
        mtx(vtype, n, m, row, col, vals(vtype, nnz), **kw)

    def symmetric(vtype, n, pairs, skew, diag, **kw):
        i, j = g.integers(0, n, pairs), g.integers(0, n, pairs)
        off = i != j
        i, j = i[off], j[off]
        w = vals(vtype, len(i))
        d = g.choice(n, diag, replace=False) if diag else np.zeros(0, np.int64)
        row, col = np.concatenate([i, j, d]), np.concatenate([j, i, d])
        val = None
        if w is not None:
            dv = np.zeros(len(d), w.dtype) if skew else vals(vtype, len(d))
            val = np.concatenate([w, -w if skew else w, dv])
        o = g.permutation(len(row))
        mtx(vtype, n, n, row[o], col[o], None if val is None else val[o], sym="skew-symmetric" if skew else "symmetric", **kw)

    general("float", 6, 5, 14)
    general("double", 7, 9, 20, field="double")
    general("int", 5, 5, 12, field="integer")
    general("void", 8, 6, 15, field="pattern")
    general("float", 6, 6, 10, field="pattern")            # values given, dropped
    symmetric("float", 9, 12, False, 4)
    symmetric("int", 7, 9, False, 3, field="integer")
    symmetric("void", 8, 10, False, 2, field="pattern")
    symmetric("float", 8, 10, True, 3)
    symmetric("double", 10, 14, True, 0, field="double")
    for vtype, field in (("float", "real"), ("void", "real"), ("int", "integer")):
        n, m = 4, 5
        cells = np.sort(g.choice(n * m, 9, replace=False))
        mtx(vtype, n, m, cells % n, cells // n, vals(vtype, 9), fmt="array", field=field)
    for vtype in ("float", "double", "int"):
        out.append(dict(kind="array", vtype=vtype, val=vals(vtype, 11), object="matrix", format="array",
                        field="integer" if vtype == "int" else "real", symmetry="general"))
    # the refusals
    for kw in (dict(obj="tensor"), dict(obj="vector"), dict(fmt="dense"), dict(field="rational"), dict(sym="triangular"),
               dict(fmt="array", field="pattern"), dict(fmt="array", sym="symmetric"), dict(sym="hermitian")):
        general("float", 4, 4, 6, **kw)
    general("void", 4, 4, 6, field="real")
    general("float", 4, 5, 6, sym="symmetric")             # not square
    mtx("float", 4, 4, [0, 1, 2], [1, 0, 3], np.array([1.5, 1.5, 2.0], np.float32), sym="symmetric")   # a mirror is missing
    mtx("float", 4, 4, [0, 1], [1, 0], np.array([1.5, 1.25], np.float32), sym="symmetric")              # another value
    mtx("float", 4, 4, [0, 1, 2], [1, 0, 2], np.array([1.5, -1.5, 3.0], np.float32), sym="skew-symmetric")  # diagonal != 0
    mtx("void", 4, 4, [0, 1], [1, 0], None, field="pattern", sym="skew-symmetric")                      # a pattern is never skew
    out.append(dict(kind="array", vtype="float", val=vals("float", 5), object="matrix", format="coordinate", field="real",
                    symmetry="general"))
    out.append(dict(kind="array", vtype="void", val=None, object="matrix", format="array", field="real", symmetry="general"))

    # edge lists
    def edges(vtype, n, row, col, val, directed):
        out.append(dict(kind="edges", vtype=vtype, n=n, m=n, row=np.asarray(row, np.int32), col=np.asarray(col, np.int32),
                        val=val, directed=directed))
    r, c = g.integers(0, 9, 16), g.integers(0, 9, 16)
    edges("void", 9, r, c, None, True)
    edges("float", 9, r, c, vals("float", 16), True)
    edges("float", 9, r, c, None, True)                   # a value type without values: unweighted
    i, j = g.integers(0, 8, 12), g.integers(0, 8, 12)
    edges("void", 8, np.concatenate([i, j, i[:4]]), np.concatenate([j, i, j[:4]]), None, False)  # mirrors and duplicates
    key = g.choice(64, 14, replace=False)                  # distinct pairs: equal weights on both directions
    i, j = key // 8, key % 8
    keep = i != j
    und = {}
    for a, b in zip(i[keep], j[keep]):
        und.setdefault((min(a, b), max(a, b)), None)
    pairs = np.array(sorted(und))
    w = vals("float", len(pairs))
    o = g.permutation(2 * len(pairs))
    edges("float", 8, np.concatenate([pairs[:, 0], pairs[:, 1]])[o], np.concatenate([pairs[:, 1], pairs[:, 0]])[o],
          np.concatenate([w, w])[o], False)
    key = g.choice(36, 10, replace=False)                  # no duplicates at all, integer weights, u < v only
    i, j = np.minimum(key // 6, key % 6), np.maximum(key // 6, key % 6) + 1
    uniq = sorted(set(zip(i.tolist(), j.tolist())))
    o = g.permutation(len(uniq))
    uu = np.array(uniq)[o]
    edges("int", 8, np.where(np.arange(len(uu)) % 2 == 0, uu[:, 0], uu[:, 1]), np.where(np.arange(len(uu)) % 2 == 0, uu[:, 1], uu[:, 0]),
          vals("int", len(uu)), False)
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a SparseBase source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "text_writers.npz"))
    a = ap.parse_args()
    cs = cases()
    data, meta = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(a.ref, tmp)
        path = os.path.join(tmp, "out.txt")
        for k, c in enumerate(cs):
            if os.path.exists(path):
                os.remove(path)
            res = subprocess.run([exe, path], input=case_text(c), capture_output=True, text=True, check=True).stdout
            res = res.rstrip("\n").split("\n")[-1]  # (the reference logs its warnings to the same stream; a message may end in a blank)
            assert res == "OK" or res.startswith("EXC "), res
            left = os.path.exists(path)
            data[f"file_{k}"] = np.frombuffer(open(path, "rb").read() if left else b"", np.uint8)
            for name in ("row", "col", "val"):
                if c.get(name) is not None:
                    data[f"{name}_{k}"] = c[name]
            m = {key: (v if not isinstance(v, np.generic) else v.item()) for key, v in c.items() if key not in ("row", "col", "val")}
            m.update(file_left=left, message="" if res == "OK" else res[4:])
            meta.append(m)
    data["cases"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(a.out, **data)
    print(a.out, os.path.getsize(a.out), "bytes,", len(cs), "cases,", sum(1 for m in meta if m["message"]), "refusals")


if __name__ == "__main__":
    main()
