"""Runs the host layer's symmetrize test program (sparsebase_amd/host/tests/test_symmetrize.cc): utils::MissingMirrors,
IsStructurallySymmetric and Symmetrize on a host CSR and an HIPCSR, the rectangular refusal, RCMReorder with and without
RCMReorderParams::symmetrize.  Then the text_tool example with a leading --symmetrize on a small unsymmetric file: the
matrix written is the ORIGINAL permuted by the order of A + A^T, the order the Python path gives; without the flag the
same file still ends in the refusal."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_host_layer import built, run  # noqa: E402,F401  (the fixture by name)


@pytest.mark.gpu
def test_symmetrize_program_gpu(built):
    out = run(os.path.join(built, "test_symmetrize"), timeout=300)
    assert "0 failures" in out and "FAIL" not in out, out
    assert out.count("[ OK ]") == 8, out


@pytest.mark.gpu
def test_text_tool_symmetrize_gpu(built, tmp_path):
    import torch
    from sparsebase_amd import ops, synth
    # a directed chain k -> k - 1 on the first 100 vertices, a random digraph on the others
    g = np.random.default_rng(8)
    n = 220
    src = np.concatenate([np.arange(1, 100), g.integers(100, n, 400)])
    dst = np.concatenate([np.arange(0, 99), g.integers(100, n, 400)])
    rp, col = synth.csr_from_edges(n, src, dst, np.int32)  # (deduplicated, rows sorted)
    row = np.repeat(np.arange(n), np.diff(rp)).astype(np.int32)
    val = (g.random(len(col)) * 10.0 ** g.integers(-4, 4, len(col))).astype(np.float32)
    src_path, dst_path = str(tmp_path / "in.mtx"), str(tmp_path / "out.mtx")
    with open(src_path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (n, n, len(col)))
        for r, c, v in zip(row, col, val):
            f.write("%d %d %.9g\n" % (r + 1, c + 1, float(v)))
    # without the flag: the refusal, as before
    p = subprocess.run([os.path.join(built, "text_tool"), src_path, dst_path], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "text_tool: " in p.stderr and "symmetric" in p.stderr, (p.returncode, p.stdout, p.stderr)
    assert not os.path.exists(dst_path)
    out = run(os.path.join(built, "text_tool"), "--symmetrize", src_path, dst_path)
    assert f"Number of vertices: {n}" in out and f"Number of edges: {len(col)}" in out and "wrote" in out
    # the Python path's order of A + A^T, and the ORIGINAL matrix permuted by it
    d = lambda a: torch.from_numpy(np.array(a)).cuda()  # (a copy: synth hands out read-only arrays)
    order = ops.rcm_reorder(d(rp), d(col), symmetrize=True)
    assert np.array_equal(np.sort(order.cpu().numpy()), np.arange(n))
    prp, pcol, pval = ops.permute_csr(n, n, d(rp), d(col), d(val), order, order)
    prow, pcol, pval = ops.csr_to_coo(n, n, prp, pcol, pval)
    text = open(dst_path, "rb").read()
    banner, size, body = text.split(b"\n", 2)
    assert banner == b"%%MatrixMarket matrix coordinate real general" and size == b"%d %d %d" % (n, n, len(col))
    r, c, v = ops.mtx_parse_coordinate(d(np.frombuffer(body, np.uint8)), n, n, len(col), 3, value_dtype=torch.float32)
    assert np.array_equal(r.cpu().numpy(), prow.cpu().numpy()) and np.array_equal(c.cpu().numpy(), pcol.cpu().numpy())
    assert v.cpu().numpy().tobytes() == pval.cpu().numpy().tobytes()
    # numpy's word on it: the file is the input with both indices renamed by one permutation
    o = order.cpu().numpy().astype(np.int64)
    key_in = np.sort(o[row] * n + o[col])
    assert np.array_equal(key_in, np.sort(r.cpu().numpy().astype(np.int64) * n + c.cpu().numpy()))
