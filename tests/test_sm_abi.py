"""CPU tests of the boundary of include/sbsm.h, the twelfth header: the header, the library's `sbsm_` exports and
capi.SM_PROTOTYPES name the same two functions with the same ctypes signatures; they share no name with the other eleven
headers and tables; the header includes sbx.h alone and carries a version of its own, and the other versions are where
they were; both entry points have a held-back-stream case for every index tuple and a row in the synchronous table of
tests/test_sm_stream_order_gpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OTHER_HEADERS = ("sbx.h", "sbx_text.h", "sbx_stats.h", "sbio.h", "sbgr.h", "sbhg.h", "sbfx.h", "sbsym.h", "sbmv.h", "sbmm.h",
                 "sbdd.h")
NAMES = ["sbsm_csr_row_softmax", "sbsm_csr_row_softmax_backward"]
PARAMETERS = {"sbsm_csr_row_softmax": ["h", "it", "vt", "n", "nnz", "row_ptr", "val", "out"],
              "sbsm_csr_row_softmax_backward": ["h", "it", "vt", "n", "nnz", "row_ptr", "s", "g", "dz"]}


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
    assert _functions("sbsm.h") == NAMES
    assert sorted(capi.SM_PROTOTYPES) == NAMES
    assert _exports(lib_path, "sbsm_") == NAMES
    lib = capi.load()
    for name, (argtypes, restype) in capi.SM_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype == restype


_CTYPE = {"sbx_handle_t": C.c_void_p, "sbx_index_type": C.c_int, "sbx_value_type": C.c_int, "int64_t": C.c_int64,
          "const void *": C.c_void_p, "void *": C.c_void_p}


def test_signatures_match_the_header():
    """Parameter by parameter: the C types of the header's declarations against the ctypes of the table."""
    from sparsebase_amd import capi
    text = _text("sbsm.h")
    for name, (argtypes, restype) in capi.SM_PROTOTYPES.items():
        m = re.search(rf"\b(\w+)\s+{name}\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert m.group(1) == "int" and restype == C.c_int
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(2).split(",")]
        assert [re.sub(r"^.*?(\w+)$", r"\1", p) for p in params] == PARAMETERS[name]
        ctypes_of = [_CTYPE[re.sub(r"\s*\w+$", "", p).strip()] for p in params]  # (the type is what precedes the name)
        assert ctypes_of == argtypes, (name, params)
        assert "col" not in PARAMETERS[name] and "m" not in PARAMETERS[name]  # (the operation never looks at a column)


def test_disjoint_from_the_other_eleven_headers_and_tables():
    from sparsebase_amd import capi
    mine = set(_functions("sbsm.h"))
    tables = (capi.PROTOTYPES, capi.TEXT_PROTOTYPES, capi.STATS_PROTOTYPES, capi.IO_PROTOTYPES, capi.GRAPH_PROTOTYPES,
              capi.HYPERGRAPH_PROTOTYPES, capi.EXTRACT_PROTOTYPES, capi.SYM_PROTOTYPES, capi.MV_PROTOTYPES,
              capi.MM_PROTOTYPES, capi.DD_PROTOTYPES)
    assert len(tables) == len(OTHER_HEADERS)
    for header, table in zip(OTHER_HEADERS, tables):
        assert not mine & set(_functions(header)), header
        assert not set(capi.SM_PROTOTYPES) & set(table), header
        assert not any(name.startswith("sbsm_") for name in table), header
    assert not any(name.startswith("sbx") for name in capi.SM_PROTOTYPES)  # (the `sbx` prefix is closed)


def test_header_includes_sbx_h_alone_and_the_twelve_versions():
    text = open(os.path.join(ROOT, "include", "sbsm.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["sbx.h"]
    assert re.search(r"#define SBSM_VERSION 100\b", text)
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


def test_both_entry_points_have_a_stream_order_case_for_every_tuple():
    torch = pytest.importorskip("torch")  # noqa: F841  (the stream-order modules import it)
    from sparsebase_amd import capi
    import test_sm_stream_order_gpu as so
    targets = {entry for _, entry, _, _ in so.CASES}
    assert targets == set(capi.SM_PROTOTYPES)
    assert so.SYNCHRONOUS == {"sbsm_csr_row_softmax": False, "sbsm_csr_row_softmax_backward": False}
    for entry in targets:
        assert any(e == entry and "other" in modes for _, e, _, modes in so.CASES), entry
        for tup in ("i32", "i64", "i32_n64"):  # every index tuple
            assert any(e == entry and f"-{tup}-" in cid + "-" for cid, e, _, modes in so.CASES), (entry, tup)
