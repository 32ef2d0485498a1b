"""CPU tests of the boundary of include/sbio.h, the fourth header: the header, the library's `sbio_` exports and
capi.IO_PROTOTYPES name the same functions with the same ctypes signatures; they share no name with the other three
headers and tables; the header includes sbx.h and carries a version of its own; every entry point has a
held-back-stream case and a row in the synchronous table of tests/test_io_stream_order_gpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OTHER_HEADERS = ("sbx.h", "sbx_text.h", "sbx_stats.h")


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
    declared = _functions("sbio.h")
    assert len(declared) == 3 and all(f.startswith("sbio_") for f in declared)
    assert sorted(capi.IO_PROTOTYPES) == declared
    assert _exports(lib_path, "sbio_") == declared
    lib = capi.load()
    for name, (argtypes, restype) in capi.IO_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype == restype


_CTYPE = {"sbx_handle_t": C.c_void_p, "sbx_index_type": C.c_int, "sbx_value_type": C.c_int, "int64_t": C.c_int64,
          "int": C.c_int, "unsigned": C.c_uint, "const void *": C.c_void_p, "void *": C.c_void_p,
          "int64_t *": C.POINTER(C.c_int64)}


def test_signatures_match_the_header():
    """Parameter by parameter: the C types of the header's declarations against the ctypes of the table."""
    from sparsebase_amd import capi
    text = _text("sbio.h")
    for name, (argtypes, restype) in capi.IO_PROTOTYPES.items():
        m = re.search(rf"\b(\w+)\s+{name}\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert m.group(1) == "int" and restype == C.c_int
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(2).split(",")]
        ctypes_of = [_CTYPE[re.sub(r"\s*\w+$", "", p).strip()] for p in params]  # (the type is what precedes the name)
        assert ctypes_of == argtypes, (name, params)


def test_disjoint_from_the_other_three_headers_and_tables():
    from sparsebase_amd import capi
    mine = set(_functions("sbio.h"))
    for header, table in zip(OTHER_HEADERS, (capi.PROTOTYPES, capi.TEXT_PROTOTYPES, capi.STATS_PROTOTYPES)):
        assert not mine & set(_functions(header)), header
        assert not set(capi.IO_PROTOTYPES) & set(table), header
        assert not any(name.startswith("sbio_") for name in table), header


def test_header_includes_sbx_h_and_has_its_own_version():
    text = open(os.path.join(ROOT, "include", "sbio.h")).read()
    assert '#include "sbx.h"' in text and re.search(r"#define SBIO_VERSION 100\b", text)
    assert not any(f'#include "{h}"' in text for h in OTHER_HEADERS[1:])
    sbx = open(os.path.join(ROOT, "include", "sbx.h")).read()
    assert re.search(r"#define SBX_VERSION 102\b", sbx)  # (the other versions stay where they were)


def test_every_io_entry_point_has_a_stream_order_case():
    torch = pytest.importorskip("torch")  # noqa: F841  (the stream-order modules import it)
    from sparsebase_amd import capi
    import test_io_stream_order_gpu as so
    targets = {entry for _, entry, _, _ in so.CASES}
    assert targets == set(capi.IO_PROTOTYPES)
    assert set(so.SYNCHRONOUS) == set(capi.IO_PROTOTYPES) and all(so.SYNCHRONOUS.values())
    assert any("other" in modes for _, _, _, modes in so.CASES)
