"""CPU tests of the boundary of include/sbmt.h, the thirteenth header: the header, the library's `sbmt_` exports and
capi.MT_PROTOTYPES name the same two functions with the same ctypes signatures; they share no name with the other twelve
headers and tables; the header includes sbx.h alone and carries a version of its own, and the other versions are where
they were; both entry points have a held-back-stream case for every index tuple and a row in the synchronous table of
tests/test_mt_stream_order_gpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OTHER_HEADERS = ("sbx.h", "sbx_text.h", "sbx_stats.h", "sbio.h", "sbgr.h", "sbhg.h", "sbfx.h", "sbsym.h", "sbmv.h", "sbmm.h",
                 "sbdd.h", "sbsm.h")
NAMES = ["sbmt_csr_spmm_t", "sbmt_csr_transpose_plan"]
PARAMETERS = {"sbmt_csr_transpose_plan": ["h", "it", "n", "m", "nnz", "row_ptr", "col", "col_ptr_out", "row_out", "perm_out"],
              "sbmt_csr_spmm_t": ["h", "it", "vt", "n", "m", "nnz", "k", "col_ptr", "row", "perm", "val", "x", "ldx", "y",
                                  "ldy"]}


@pytest.fixture(scope="module")
def lib_path():
    from sparsebase_amd import build
    return build.build()


def _text(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def _functions(header):
    return sorted(set(re.findall(r"\b(sb[a-z]*_[a-z0-9_]+)\s*\(", _text(header))))


def _exports(lib_path, prefix):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    return sorted(set(re.findall(rf"\bT ({prefix}[a-z0-9_]*)$", out, flags=re.M)))  # (unmangled names only: the C symbols)


def test_header_table_and_exports_agree(lib_path):
    from sparsebase_amd import capi
    assert _functions("sbmt.h") == NAMES
    assert sorted(capi.MT_PROTOTYPES) == NAMES
    assert _exports(lib_path, "sbmt_") == NAMES
    lib = capi.load()
    for name, (argtypes, restype) in capi.MT_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype == restype


_CTYPE = {"sbx_handle_t": C.c_void_p, "sbx_index_type": C.c_int, "sbx_value_type": C.c_int, "int64_t": C.c_int64,
          "const void *": C.c_void_p, "void *": C.c_void_p}


def test_signatures_match_the_header():
    """Parameter by parameter: the C types of the header's declarations against the ctypes of the table."""
    from sparsebase_amd import capi
    text = _text("sbmt.h")
    for name, (argtypes, restype) in capi.MT_PROTOTYPES.items():
        m = re.search(rf"\b(\w+)\s+{name}\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert m.group(1) == "int" and restype == C.c_int
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(2).split(",")]
        assert [re.sub(r"^.*?(\w+)$", r"\1", p) for p in params] == PARAMETERS[name]
        ctypes_of = [_CTYPE[re.sub(r"\s*\w+$", "", p).strip()] for p in params]  # (the type is what precedes the name)
        assert ctypes_of == argtypes, (name, params)
    assert "vt" not in PARAMETERS["sbmt_csr_transpose_plan"] and "val" not in PARAMETERS["sbmt_csr_transpose_plan"]  # (a plan
    # never sees a value)


def test_disjoint_from_the_other_twelve_headers_and_tables():
    from sparsebase_amd import capi
    mine = set(_functions("sbmt.h"))
    tables = (capi.PROTOTYPES, capi.TEXT_PROTOTYPES, capi.STATS_PROTOTYPES, capi.IO_PROTOTYPES, capi.GRAPH_PROTOTYPES,
              capi.HYPERGRAPH_PROTOTYPES, capi.EXTRACT_PROTOTYPES, capi.SYM_PROTOTYPES, capi.MV_PROTOTYPES,
              capi.MM_PROTOTYPES, capi.DD_PROTOTYPES, capi.SM_PROTOTYPES)
    assert len(tables) == len(OTHER_HEADERS)
    for header, table in zip(OTHER_HEADERS, tables):
        assert not mine & set(_functions(header)), header
        assert not set(capi.MT_PROTOTYPES) & set(table), header
        assert not any(name.startswith("sbmt_") for name in table), header
    assert not any(name.startswith("sbx") for name in capi.MT_PROTOTYPES)  # (the `sbx` prefix is closed)


def test_header_includes_sbx_h_alone_and_the_thirteen_versions():
    text = open(os.path.join(ROOT, "include", "sbmt.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["sbx.h"]
    assert re.search(r"#define SBMT_VERSION 100\b", text)
    inc = lambda h: open(os.path.join(ROOT, "include", h)).read()
    assert re.search(r"#define SBX_VERSION 102\b", inc("sbx.h"))
    assert re.search(r"#define SBIO_VERSION 100\b", inc("sbio.h"))
    assert re.search(r"#define SBX_TEXT_VERSION 100\b", inc("sbx_text.h"))
    assert re.search(r"#define SBX_STATS_VERSION 100\b", inc("sbx_stats.h"))
    assert re.search(r"#define SBGR_VERSION 100\b", inc("sbgr.h"))
    assert re.search(r"#define SBHG_VERSION 100\b", inc("sbhg.h"))
    assert re.search(r"#define SBFX_VERSION 100\b", inc("sbfx.h"))
    assert re.search(r"#define SBSYM_VERSION 100\b", inc("sbsym.h"))
    assert re.search(r"#define SBMV_VERSION 100\b", inc("sbmv.h"))
    assert re.search(r"#define SBMM_VERSION 100\b", inc("sbmm.h"))
    assert re.search(r"#define SBDD_VERSION 100\b", inc("sbdd.h"))
    assert re.search(r"#define SBSM_VERSION 100\b", inc("sbsm.h"))
    assert _functions("sbmm.h") == ["sbmm_csr_spmm"]  # (the product's own header is as it was: one function)


def test_both_entry_points_have_a_stream_order_case_for_every_tuple():
    torch = pytest.importorskip("torch")  # noqa: F841  (the stream-order modules import it)
    from sparsebase_amd import capi
    import test_mt_stream_order_gpu as so
    targets = {entry for _, entry, _, _ in so.CASES}
    assert targets == set(capi.MT_PROTOTYPES)
    assert so.SYNCHRONOUS == {"sbmt_csr_transpose_plan": True, "sbmt_csr_spmm_t": False}
    for entry in targets:
        assert any(e == entry and "other" in modes for _, e, _, modes in so.CASES), entry
        for tup in ("i32", "i64", "i32_n64"):  # every index tuple
            assert any(e == entry and f"-{tup}-" in cid + "-" for cid, e, _, modes in so.CASES), (entry, tup)
