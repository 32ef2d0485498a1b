"""Runs the host layer's PaToH test program (sparsebase_amd/host/tests/test_patoh.cc): the reference's PatohReader tests
over the four files they write, the writer's bytes for every flag, base and chunk size, empty nets, the refusals,
object::HyperGraph, and a round trip write -> read for three type tuples.  One attempt: a crashed or hung GPU process is
not started again."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_layer import built, run  # noqa: E402,F401  (the fixture by name)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.gpu
def test_patoh_program_gpu(built, tmp_path):
    out = run(os.path.join(built, "test_patoh"), str(tmp_path), GOLDEN, timeout=300, attempts=1)
    assert "0 failures" in out and "FAIL" not in out, out
    assert out.count("[ OK ]") >= 7, out
