"""Runs the host layer's text-writer test program (sparsebase_amd/host/tests/test_text_writers.cc) and the text_tool
example: .mtx -> RCM -> permute -> .mtx / edge list, read back to the same permuted matrix bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_layer import built, run  # noqa: E402,F401  (the fixture by name)


@pytest.mark.gpu
def test_text_writers_program_gpu(built, tmp_path):
    out = run(os.path.join(built, "test_text_writers"), str(tmp_path), timeout=300)
    assert "0 failures" in out and "FAIL" not in out, out
    assert out.count("[ OK ]") >= 8, out


@pytest.mark.gpu
def test_text_tool_round_trip_gpu(built, tmp_path):
    import torch
    from sparsebase_amd import ops, synth
    rp, col = synth.grid_graph(24, 40, shuffle_seed=5)
    n = len(rp) - 1
    row = np.repeat(np.arange(n), np.diff(rp)).astype(np.int32)
    col = col.astype(np.int32)[np.lexsort((col, row))]  # (rows sorted, as the reader leaves them)
    g = np.random.default_rng(3)
    val = (g.random(len(col)) * 10.0 ** g.integers(-6, 6, len(col))).astype(np.float32)
    src, dst, edges = (str(tmp_path / x) for x in ("in.mtx", "out.mtx", "out.edges"))
    with open(src, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, len(col)))
        for r, c, v in zip(row, col, val):
            f.write("%d %d %.9g\n" % (r + 1, c + 1, float(v)))
    out = run(os.path.join(built, "text_tool"), src, dst, edges)
    assert f"Number of vertices: {n}" in out and "wrote" in out
    # what the file must hold: the library's own RCM + permute of the same matrix
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rp32 = rp.astype(np.int32)
    order = ops.rcm_reorder(d(rp32), d(col))
    prp, pcol, pval = ops.permute_csr(n, n, d(rp32), d(col), d(val), order, order)
    prow, pcol, pval = ops.csr_to_coo(n, n, prp, pcol, pval)
    want = (prow.cpu().numpy(), pcol.cpu().numpy(), pval.cpu().numpy())
    # read back with the library's reader
    text = open(dst, "rb").read()
    banner, size, body = text.split(b"\n", 2)
    assert banner == b"%%MatrixMarket matrix coordinate real general" and size == b"%d %d %d" % (n, n, len(col))
    r, c, v = ops.mtx_parse_coordinate(d(np.frombuffer(body, np.uint8)), n, n, len(col), 3, value_dtype=torch.float32)
    assert np.array_equal(r.cpu().numpy(), want[0]) and np.array_equal(c.cpu().numpy(), want[1])
    assert v.cpu().numpy().tobytes() == want[2].tobytes()
    n2, m2, r, c, v = ops.edge_list_parse(d(np.frombuffer(open(edges, "rb").read(), np.uint8)), weighted=True,
                                          read_undirected=False, value_dtype=torch.float32)
    assert np.array_equal(r.cpu().numpy(), want[0]) and np.array_equal(c.cpu().numpy(), want[1])
    assert v.cpu().numpy().tobytes() == want[2].tobytes()
