"""Runs the host layer's experiment test program (sparsebase_amd/host/tests/test_experiment.cc) on ash958.mtx, written
from tests/golden/ash958.npz as tests/test_host_layer.py::test_examples_gpu does: what the reference's two experiment
suites assert, restated, then SpMV through the harness host-staged against device-resident against a plain loop, the
LoadHIPCSR -> ReorderHIP<RCMReorder> -> SpMV pipeline, duplicate ids and kernels/spmv.h.  Then the example_experiment
binary on a symmetric grid graph as a Matrix Market file and as an edge list: the result lines of `original` agree
between the host-staged and the device-resident kernel, file by file."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_layer import built, run, write_mtx  # noqa: E402,F401  (the fixture by name)


@pytest.mark.gpu
def test_experiment_program_gpu(built, tmp_path, golden_dir):
    z = np.load(os.path.join(golden_dir, "ash958.npz"))
    n, m, _ = (int(x) for x in z["dims"])
    mtx = str(tmp_path / "ash958.mtx")
    write_mtx(mtx, n, m, z["file_row"], z["file_col"])
    out = run(os.path.join(built, "test_experiment"), mtx, timeout=300)
    assert "0 failures" in out and "FAIL" not in out, out
    assert out.count("[ OK ]") == 11, out


@pytest.mark.gpu
def test_example_experiment_gpu(built, tmp_path):
    from sparsebase_amd import synth
    rp, col = synth.grid_graph(16, 32, shuffle_seed=3)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    mtx, edges = str(tmp_path / "grid.mtx"), str(tmp_path / "grid.edges")
    write_mtx(mtx, n, n, rows, col)
    with open(edges, "w") as f:
        for r, c in zip(rows, col):
            if r < c:  # (the reader adds the reverse edges)
                f.write(f"{r} {c}\n")
    out = run(os.path.join(built, "example_experiment"), mtx, edges)
    lines = [(key, body.split()) for key, body in re.findall(r"^(-\S+,\S+,hip-\S+,\d+): (.*)$", out, flags=re.M)]
    results = {key: " ".join(body) for key, body in lines if len(body) == 8}  # (a result line prints eight values,
    times = [body[0] for key, body in lines if len(body) == 1]                # a run-time line one per Run)
    assert len(results) == 16 and len(times) == 16, out
    for path in (mtx, edges):
        for i in range(2):
            staged, resident = results[f"-{path},original,hip-staged,{i}"], results[f"-{path},original,hip-resident,{i}"]
            assert staged == resident and len(staged.split()) == 8, (path, i, staged, resident)
            assert results[f"-{path},RCM,hip-staged,{i}"] == results[f"-{path},RCM,hip-resident,{i}"]
    # the same matrix from both files, the vectors differ by seed: the results of one file do not repeat the other's
    assert results[f"-{mtx},original,hip-staged,0"] != results[f"-{edges},original,hip-staged,0"]
    for name in ("format", "processed_format"):
        assert any(line.startswith(f"{name},-{mtx}") for line in out.splitlines())
    assert all(float(t) > 0 for t in times)
