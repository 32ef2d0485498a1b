"""Builds the host layer and runs its transposed-product test program (sparsebase_amd/host/tests/test_spmm_t.cc) on a
matrix the program writes itself: a kernels::TransposePlan built from a host CSR and from an HIPCSR, kernels::SpMMTransposed
host-staged and device-resident against a plain loop for k = 1, 3, 64 and 130 (exact integers), one plan reused for two
value arrays, a rectangle whose plan is spelled out, the operand-size, device-mismatch and bad-column exceptions, and
experiment::SpMMTransposed through ConcreteExperiment with and without a plan in its parameter."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_layer import built, run  # noqa: E402,F401  (the fixture by name)


@pytest.mark.gpu
def test_spmm_t_program_gpu(built, tmp_path):
    out = run(os.path.join(built, "test_spmm_t"), str(tmp_path / "graph.mtx"), timeout=300, attempts=1)
    assert "0 failures" in out and "FAIL" not in out, out
    assert out.count("[ OK ]") == 4, out
