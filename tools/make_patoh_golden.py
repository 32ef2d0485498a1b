"""Records tests/golden/patoh.npz: what the REAL reference's PatohReader (io/patoh_reader.cc) reads and what its
PatohWriter (io/patoh_writer.cc) writes, for the cases tests/test_patoh_host.py checks the restatement against (and
tests/test_patoh_gpu.py the ABI).

    python tools/make_patoh_golden.py --ref /path/to/SparseBase

The reference is compiled header-only in a temporary directory (sparsebase/config.h derived from its own config.h.in, as
tools/make_metis_golden.py does) against a small driver whose text lives in this file.  Nothing compiled is kept.  The
reference reads weights as int, so every number travels as a decimal integer.

Reader cases hold only files for which the reference is defined: exactly `nets` net lines and `pins` pins, no malformed
token, at most `cells` cell weights, no net line without a weight in a net-weighted file (the reference leaves that
weight uninitialised, so the "blank line in a net-weighted file" of the format's description is not recorded: the
library refuses it).  The file holds three arrays: `ints` (every integer array, end to end), `text` (every file's bytes) and
`cases` (JSON): per reader case the value type, n_, m_, the cells, base_type_ and constraint_num_, and as [offset, length]
into `text` its input file (`in`) and into `ints` xpin / pin / xnet / net / nw / cw (what the HyperGraph holds; the weights
where they exist).  Writer cases (<int, int, int>, the one tuple the reference writes) hold the arrays of the HyperGraph
given, the constructor's flags and `file` (the bytes written).  tests/patoh_restate.py: load_golden() unpacks it.
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
#include "sparsebase/format/array.h"
#include "sparsebase/format/csr.h"
#include "sparsebase/io/patoh_reader.h"
#include "sparsebase/io/patoh_writer.h"
#include "sparsebase/object/object.h"
#include "sparsebase/utils/exception.h"
using namespace sparsebase;
static int num() { char b[64]; if (scanf("%63s", b) != 1) exit(2); return atoi(b); }
// R <vt> <path>:  prints "H n m cells base constraints hasw", then xpin, pin, xnet, net, net weights, cell weights
template <typename V> static void read_case(const char *path) {
  io::PatohReader<int, int, V> reader(path);
  auto *g = reader.ReadHyperGraph();
  auto *csr = g->get_connectivity()->template AsAbsolute<format::CSR<int, int, V>>();
  const int n = (int)g->n_, m = (int)g->m_, cells = (int)csr->get_dimensions()[1];
  bool hasw = false;
  if constexpr (!std::is_same_v<V, void>) hasw = g->netWeights_ != nullptr && g->cellWeights_ != nullptr;
  printf("H %d %d %d %d %d %d\n", n, m, cells, (int)g->base_type_, (int)g->constraint_num_, hasw ? 1 : 0);
  for (int i = 0; i <= n; i++) printf(" %d", csr->get_row_ptr()[i]);
  printf("\n");
  for (int i = 0; i < m; i++) printf(" %d", csr->get_col()[i]);
  printf("\n");
  for (int i = 0; i <= cells; i++) printf(" %d", g->xNetCSR_->get_row_ptr()[i]);
  printf("\n");
  for (int i = 0; i < m; i++) printf(" %d", g->xNetCSR_->get_col()[i]);
  printf("\n");
  if constexpr (!std::is_same_v<V, void>) {
    if (hasw) for (int i = 0; i < n; i++) printf(" %lld", (long long)g->netWeights_->get_vals()[i]);
    printf("\n");
    if (hasw) for (int i = 0; i < cells; i++) printf(" %lld", (long long)g->cellWeights_->get_vals()[i]);
    printf("\n");
  } else {
    printf("\n\n");
  }
}
// W <zero> <ew> <vw> <path>, stdin: base cells nets pins constraints xpin[] pin[] xnet[] net[] nw[] cw[]
static void write_case(int zero, int ew, int vw, const char *path) {
  const int base = num(), cells = num(), nets = num(), pins = num(), constraints = num();
  int *xpin = new int[nets + 1], *pin = new int[pins + 1], *xnet = new int[cells + 1], *net = new int[pins + 1];
  int *nw = new int[nets + 1], *cw = new int[cells + 1];
  for (int i = 0; i <= nets; i++) xpin[i] = num();
  for (int i = 0; i < pins; i++) pin[i] = num();
  for (int i = 0; i <= cells; i++) xnet[i] = num();
  for (int i = 0; i < pins; i++) net[i] = num();
  for (int i = 0; i < nets; i++) nw[i] = num();
  for (int i = 0; i < cells; i++) cw[i] = num();
  object::HyperGraph<int, int, int> g(
      new format::CSR<int, int, int>(nets, cells, xpin, pin, nullptr, format::kNotOwned, true),
      new format::Array<int>(nets, nw), new format::Array<int>(cells, cw), base, constraints,
      new format::CSR<int, int, int>(cells, nets, xnet, net, nullptr, format::kNotOwned, true));
  io::PatohWriter<int, int, int>(path, zero != 0, ew != 0, vw != 0, constraints).WriteHyperGraph(&g);
  printf("OK\n");
}
int main(int argc, char **argv) {
  try {
    if (argv[1][0] == 'R') {
      const char vt = argv[2][0];
      if (vt == 'v') read_case<void>(argv[3]);
      else if (vt == 'i') read_case<int>(argv[3]);
      else if (vt == 'f') read_case<float>(argv[3]);
      else read_case<double>(argv[3]);
    } else {
      write_case(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), argv[5]);
    }
  } catch (utils::Exception &e) {
    printf("EXC %s\n", e.what());
  }
  return 0;
}
"""

DTYPES = {"void": None, "int": np.int32, "float": np.float32, "double": np.float64}
VTYPES = ("int", "float", "double", "void")
# the four files of the reference's own reader tests, kept as fixtures
OWN = ("patoh_unweighted", "patoh_net_weights", "patoh_cell_weights", "patoh_both_weights")


def random_hypergraph(g, nets, cells, empty=(), unused=()):
    """Per net a list of 0-based cells (unsorted, without duplicates); nets in `empty` get none, cells in `unused` no net."""
    pool = [c for c in range(cells) if c not in unused]
    return [[] if j in empty else [int(c) for c in g.choice(pool, size=int(g.integers(1, min(7, len(pool) + 1))), replace=False)]
            for j in range(nets)]


def file_text(nets, cells, base=0, scheme=0, constraints=None, nw=None, cw=None, sep=" ", eol="\n", last_eol=None,
              header=True):
    """A PaToH file of the nets (lists of 0-based cells): nw per net a weight, cw the cell weights (any number of them);
    last_eol None: a final newline exactly when no cell-weight line follows the nets."""
    head = [str(base), str(cells), str(len(nets)), str(sum(len(n) for n in nets))]
    if scheme or constraints is not None:
        head.append(str(scheme))
    if constraints is not None:
        head.append(str(constraints))
    lines = [" ".join(head)] if header else []
    for j, n in enumerate(nets):
        toks = [str(nw[j])] if scheme & 2 else []
        lines.append(sep.join(toks + [str(c + base) for c in n]))
    if scheme & 1 and cw is not None:
        lines.append(sep.join(str(w) for w in cw))
        last_eol = False if last_eol is None else last_eol
    else:
        last_eol = True if last_eol is None else last_eol
    return (eol.join(lines) + (eol if last_eol else "")).encode()


def reader_inputs():
    g = np.random.default_rng(21)
    out = []

    def add(name, data, scheme):
        for vt in VTYPES:
            if vt != "void" or scheme == 0:
                out.append((name, data, vt))

    for k, name in enumerate(OWN):
        add(name, open(os.path.join(ROOT, "tests", "golden", name + ".hypeg"), "rb").read(), (0, 2, 1, 3)[k])
    nets = random_hypergraph(g, 9, 8)
    nw = [int(x) for x in g.integers(1, 60, 9)]
    cw = [int(x) for x in g.integers(1, 99, 8)]
    for scheme in range(4):
        for base in (0, 1):
            add(f"scheme_{scheme}_base_{base}", file_text(nets, 8, base, scheme, None, nw, cw), scheme)
            add(f"scheme_{scheme}_base_{base}_con", file_text(nets, 8, base, scheme, 2, nw, cw), scheme)
    plain = file_text(nets, 8, 1, 3, None, nw, cw)
    add("comments", b"% a comment\n%another 1 2 3\n" + plain.replace(b"\n", b"\n% between the lines 1 2 3\n", 4), 3)
    add("comment_last", file_text(nets, 8, 0, 1, None, nw, None, last_eol=True) + b"% 1 2 3", 1)
    e = random_hypergraph(g, 9, 8, empty=(0, 4, 8))
    add("empty_nets", file_text(e, 8, 0, 0), 0)
    add("empty_nets_blank", file_text(e, 8, 1, 1, None, None, cw).replace(b"\n\n", b"\n \t\n"), 1)
    add("crlf_tabs", file_text(nets, 8, 1, 3, None, nw, cw, sep="\t", eol="\r\n"), 3)
    add("crlf_tabs_plain", file_text(e, 8, 0, 0, sep="\t", eol="\r\n"), 0)
    add("weighted_ends_in_newline", file_text(nets, 8, 0, 1, None, nw, None, last_eol=True), 1)
    add("net_weighted_no_newline", file_text(nets, 8, 0, 2, None, nw, None, last_eol=False), 2)
    add("plain_no_newline", file_text(nets, 8, 1, 0, last_eol=False), 0)
    add("few_cell_weights", file_text(nets, 8, 1, 3, None, nw, cw[:5]), 3)
    d = [n + n[:2] for n in nets]
    add("duplicate_pins", file_text(d, 8, 1, 2, None, nw, None), 2)
    u = random_hypergraph(g, 9, 8, unused=(0, 3, 7))
    add("unused_cells", file_text(u, 8, 0, 3, None, nw, cw), 3)
    add("negative_weights", file_text(nets, 8, 0, 3, None, [-x for x in nw], [x - 50 for x in cw]), 3)
    for k, (n, c, scheme) in enumerate(((40, 31, 3), (41, 64, 0), (39, 17, 2))):
        r = random_hypergraph(g, n, c, empty=(5,) if scheme == 0 else ())
        add(f"random_{k}", file_text(r, c, k & 1, scheme, None, [int(x) for x in g.integers(1, 999, n)],
                                     [int(x) for x in g.integers(1, 999, c)]), scheme)
    return out


def writer_inputs():
    g = np.random.default_rng(22)
    nets = random_hypergraph(g, 10, 9, unused=(2,))
    out = []
    for base in (0, 1):
        xpin = np.cumsum([0] + [len(n) for n in nets]).astype(np.int32)
        pin = np.array([c + base for n in nets for c in n], np.int32)
        order = np.argsort(pin - base, kind="stable")
        net = (np.searchsorted(xpin, order, side="right") - 1 + base).astype(np.int32)
        xnet = np.concatenate([[0], np.cumsum(np.bincount(pin - base, minlength=9))]).astype(np.int32)
        nw = g.integers(1, 999, 10).astype(np.int32)
        cw = g.integers(-50, 50, 9).astype(np.int32)
        for zero in (False, True):
            for ew in (False, True):
                for vw in (False, True):
                    for constraints in (1, 2):
                        out.append(dict(base=base, zero=zero, ew=ew, vw=vw, constraints=constraints, cells=9, xpin=xpin,
                                        pin=pin, xnet=xnet, net=net, nw=nw, cw=cw))
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


def _ints(line, dtype=np.int32):
    return np.array([int(t) for t in line.split()], np.int64).astype(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a SparseBase source tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "patoh.npz"))
    a = ap.parse_args()
    ints, text, meta = [], [], []  # (two arrays for all cases: an array of its own per case and name costs more than it holds)

    def keep(pool, arr):
        off = sum(len(x) for x in pool)
        pool.append(arr)
        return [off, len(arr)]

    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(a.ref, tmp)
        path = os.path.join(tmp, "case.hypeg")
        for name, data, vt in reader_inputs():
            with open(path, "wb") as f:
                f.write(data)
            res = subprocess.run([exe, "R", vt, path], capture_output=True, text=True, check=True).stdout
            lines = res.split("\n")
            while lines and not lines[0].startswith("H "):
                lines.pop(0)
            assert lines, (name, res)
            n, m, cells, base, constraints, hasw = (int(x) for x in lines[0].split()[1:])
            c = dict(kind="read", name=name, vtype=vt, n=n, m=m, cells=cells, base=base, constraints=constraints)
            c["in"] = keep(text, np.frombuffer(data, np.uint8))
            for key, line in zip(("xpin", "pin", "xnet", "net", "nw", "cw"), lines[1:7]):
                if key in ("nw", "cw") and not hasw:
                    continue
                c[key] = keep(ints, _ints(line, np.int64))
            assert c["pin"][1] == m and c["xpin"][1] == n + 1, name
            meta.append(c)
        for w in writer_inputs():
            if os.path.exists(path):
                os.remove(path)
            join = lambda arr: " ".join(str(int(x)) for x in arr)
            stdin = "%d %d %d %d %d\n%s\n%s\n%s\n%s\n%s\n%s\n" % (
                w["base"], w["cells"], len(w["xpin"]) - 1, len(w["pin"]), w["constraints"], join(w["xpin"]), join(w["pin"]),
                join(w["xnet"]), join(w["net"]), join(w["nw"]), join(w["cw"]))
            res = subprocess.run([exe, "W", str(int(w["zero"])), str(int(w["ew"])), str(int(w["vw"])), path], input=stdin,
                                 capture_output=True, text=True, check=True).stdout.strip().split("\n")[-1]
            assert res == "OK", res
            c = dict(kind="write", vtype="int", base=w["base"], zero=w["zero"], ew=w["ew"], vw=w["vw"],
                     constraints=w["constraints"], cells=w["cells"])
            c["file"] = keep(text, np.frombuffer(open(path, "rb").read(), np.uint8))
            for key in ("xpin", "pin", "xnet", "net", "nw", "cw"):
                c[key] = keep(ints, w[key].astype(np.int64))
            meta.append(c)
    np.savez_compressed(a.out, ints=np.concatenate(ints), text=np.concatenate(text),
                        cases=np.frombuffer(json.dumps(meta).encode(), np.uint8))
    print(a.out, os.path.getsize(a.out), "bytes,", len(meta), "cases")


if __name__ == "__main__":
    main()
