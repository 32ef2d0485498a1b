"""CPU tests of the text-output ABI's boundary: include/sbx_text.h, the library's exports and capi.TEXT_PROTOTYPES name
the same functions; the header declares nothing include/sbx.h declares; every entry point has a held-back-stream case
and a row in the synchronous table of tests/test_text_stream_order_gpu.py."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def lib_path():
    from sparsebase_amd import build
    return build.build()


def _functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sbx_[a-z0-9_]+)\s*\(", text)))


def test_header_table_and_exports_agree(lib_path):
    from sparsebase_amd import capi
    declared = _functions("sbx_text.h")
    assert declared and sorted(capi.TEXT_PROTOTYPES) == declared
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    exported = set(re.findall(r"\bT (sbx_[a-z0-9_]+)", out))
    assert not [f for f in declared if f not in exported]
    # nothing is exported that neither header declares
    assert exported == set(declared) | set(_functions("sbx.h"))
    lib = capi.load()
    for name, (argtypes, restype) in capi.TEXT_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype == restype


def test_text_header_adds_to_sbx_h_only():
    assert not set(_functions("sbx_text.h")) & set(_functions("sbx.h"))
    from sparsebase_amd import capi
    assert not set(capi.TEXT_PROTOTYPES) & set(capi.PROTOTYPES)
    text = open(os.path.join(ROOT, "include", "sbx_text.h")).read()
    assert '#include "sbx.h"' in text and re.search(r"#define SBX_TEXT_VERSION 100\b", text)


def test_every_text_entry_point_has_a_stream_order_case():
    torch = pytest.importorskip("torch")  # noqa: F841  (the stream-order modules import it)
    from sparsebase_amd import capi
    import test_text_stream_order_gpu as so
    targets = {entry for _, entry, _, _ in so.CASES}
    assert targets == set(capi.TEXT_PROTOTYPES)
    assert set(so.SYNCHRONOUS) == set(capi.TEXT_PROTOTYPES)
