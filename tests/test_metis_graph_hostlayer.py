"""Runs the host layer's METIS graph test program (sparsebase_amd/host/tests/test_metis_graph.cc): the reference's
MetisGraphReader and MetisGraphWriter tests transcribed, the writer's bytes, the refusals, object::Graph, and a round
trip read -> RCM -> permute -> write -> read.  One attempt: a crashed or hung GPU process is not started again."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_layer import built, run  # noqa: E402,F401  (the fixture by name)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.gpu
def test_metis_graph_program_gpu(built, tmp_path):
    out = run(os.path.join(built, "test_metis_graph"), str(tmp_path), GOLDEN, timeout=300, attempts=1)
    assert "0 failures" in out and "FAIL" not in out, out
    assert out.count("[ OK ]") >= 6, out
