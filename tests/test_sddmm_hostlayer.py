"""Builds the host layer and runs its SDDMM test program (sparsebase_amd/host/tests/test_sddmm.cc) on a matrix the program
writes itself: kernels::SDDMM host-staged against device-resident against a plain loop for k = 1, 3, 64 and 130, the
operand-size and device-mismatch exceptions, and experiment::SDDMM through ConcreteExperiment with Pass and with
RCMReorder on the device."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_layer import built, run  # noqa: E402,F401  (the fixture by name)


@pytest.mark.gpu
def test_sddmm_program_gpu(built, tmp_path):
    out = run(os.path.join(built, "test_sddmm"), str(tmp_path / "symmetric.mtx"), timeout=300, attempts=1)
    assert "0 failures" in out and "FAIL" not in out, out
    assert out.count("[ OK ]") == 5, out
