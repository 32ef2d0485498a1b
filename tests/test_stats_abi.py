"""CPU tests of the boundary of include/sbx_stats.h, and of the three headers together: the header, the library's
`sbxstat_` exports and capi.STATS_PROTOTYPES name the same functions; every exported C symbol that begins with `sbx` is
declared in one of the three headers (the `sbx_` checks of tests/test_abi.py and tests/test_text_abi.py do not see the
`sbxstat_` prefix); headers and tables are pairwise disjoint; every entry point has a held-back-stream case and a row in
the synchronous table of tests/test_stats_stream_order_gpu.py."""
import itertools
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
HEADERS = ("sbx.h", "sbx_text.h", "sbx_stats.h")


@pytest.fixture(scope="module")
def lib_path():
    from sparsebase_amd import build
    return build.build()


def _functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sbx[a-z0-9]*_[a-z0-9_]+)\s*\(", text)))


def _exports(lib_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    return set(re.findall(r"\bT (sbx[a-z0-9_]*)$", out, flags=re.M))  # (unmangled names only: the C symbols)


def test_header_table_and_exports_agree(lib_path):
    from sparsebase_amd import capi
    declared = _functions("sbx_stats.h")
    assert declared and all(f.startswith("sbxstat_") for f in declared)
    assert sorted(capi.STATS_PROTOTYPES) == declared
    assert sorted(f for f in _exports(lib_path) if f.startswith("sbxstat_")) == declared
    lib = capi.load()
    for name, (argtypes, restype) in capi.STATS_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype == restype


def test_every_sbx_export_is_declared_in_one_of_the_three_headers(lib_path):
    declared = set().union(*(_functions(h) for h in HEADERS))
    exported = _exports(lib_path)
    assert exported and not sorted(exported - declared), sorted(exported - declared)
    assert not sorted(declared - exported), sorted(declared - exported)


def test_headers_and_tables_are_pairwise_disjoint():
    from sparsebase_amd import capi
    tables = (capi.PROTOTYPES, capi.TEXT_PROTOTYPES, capi.STATS_PROTOTYPES)
    for (ha, ta), (hb, tb) in itertools.combinations(zip(HEADERS, tables), 2):
        assert not set(_functions(ha)) & set(_functions(hb)), (ha, hb)
        assert not set(ta) & set(tb), (ha, hb)
    for header, table in zip(HEADERS, tables):
        assert sorted(table) == _functions(header), header
    text = open(os.path.join(ROOT, "include", "sbx_stats.h")).read()
    assert '#include "sbx.h"' in text and re.search(r"#define SBX_STATS_VERSION 100\b", text)


def test_struct_layout_matches_the_header():
    import ctypes as C
    from sparsebase_amd import capi
    text = open(os.path.join(ROOT, "include", "sbx_stats.h")).read()
    body = re.search(r"typedef struct sbxstat_degrees \{(.*?)\} sbxstat_degrees;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int64_t|uint64_t|double)\s+([a-z_, ]+);", body):
        fields += [(n.strip(), {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}[ctype]) for n in names.split(",")]
    assert fields == list(capi.StatDegrees._fields_) and C.sizeof(capi.StatDegrees) == 80
    assert (capi.STAT_MEDIAN, capi.STAT_LOG) == tuple(int(re.search(rf"#define {n}\s+0x([0-9a-f]+)u", text).group(1), 16)
                                                      for n in ("SBXSTAT_MEDIAN", "SBXSTAT_LOG"))


def test_every_stats_entry_point_has_a_stream_order_case():
    torch = pytest.importorskip("torch")  # noqa: F841  (the stream-order modules import it)
    from sparsebase_amd import capi
    import test_stats_stream_order_gpu as so
    targets = {entry for _, entry, _, _ in so.CASES}
    assert targets == set(capi.STATS_PROTOTYPES)
    assert set(so.SYNCHRONOUS) == set(capi.STATS_PROTOTYPES) and all(so.SYNCHRONOUS.values())
