"""Builds the host layer and runs its row-softmax test program (sparsebase_amd/host/tests/test_row_softmax.cc) on a matrix
the program writes itself: kernels::RowSoftmax and kernels::RowSoftmaxBackward host-staged against device-resident
against a plain loop in long double, the operand-size and device-mismatch exceptions, and experiment::RowSoftmax through
ConcreteExperiment with Pass and with RCMReorder on the device."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_layer import built, run  # noqa: E402,F401  (the fixture by name)


def test_the_program_holds_the_restatement_s_constant():
    """The program's bound is that of tests/softmax_restate.py: its copy of EXP_ULPS is the same number."""
    import softmax_restate as sm
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "sparsebase_amd", "host", "tests", "test_row_softmax.cc")).read()
    assert [int(x) for x in re.findall(r"constexpr long double EXP_ULPS = (\d+);", text)] == [sm.EXP_ULPS]


@pytest.mark.gpu
def test_row_softmax_program_gpu(built, tmp_path):
    out = run(os.path.join(built, "test_row_softmax"), str(tmp_path / "symmetric.mtx"), timeout=300, attempts=1)
    assert "0 failures" in out and "FAIL" not in out, out
    assert out.count("[ OK ]") == 5, out
