"""The host layer's degree-statistic features and feature::OffDiagBlockNNZ on the MI355X: the C++ program
sparsebase_amd/host/tests/test_degree_features.cc walks every class through its interface, on a host format and its HIP
twin, against constants taken from tests/golden/degree_stats.npz."""
import os

import pytest

from test_host_layer import built, run  # noqa: F401  (the host programs' fixture and runner)

pytestmark = pytest.mark.gpu


def test_cpp_api(built):  # noqa: F811
    out = run(os.path.join(built, "test_degree_features"))
    assert "0 failures" in out and "FAIL" not in out, out
