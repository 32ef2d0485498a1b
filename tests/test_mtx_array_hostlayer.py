"""Runs the host layer's array-format reader test program (sparsebase_amd/host/tests/test_mtx_array.cc): MTXReader on
array files (ReadCOO / ReadCSR / ReadHIPCOO, the refusals), ReadArray / ReadHIPArray, the IOBase facade and the round
trips through MTXWriter."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_layer import built, run  # noqa: E402,F401  (the fixture by name)


@pytest.mark.gpu
def test_mtx_array_program_gpu(built, tmp_path):
    out = run(os.path.join(built, "test_mtx_array"), str(tmp_path), timeout=300)
    assert "0 failures" in out and "FAIL" not in out, out
    assert out.count("[ OK ]") >= 8, out
