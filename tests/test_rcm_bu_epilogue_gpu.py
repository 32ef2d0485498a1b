"""The epilogue of RCM's bottom-up levels (sbx_rcm.hip: stage_end_block, ubu_chain_end).  The four kernels of a
bottom-up level run as 1024-thread workgroups, two per CU; a workgroup adds its degree sum to the level's counter and
its scanned entries to edges_bu — and to edges_bu ALONE: the host reports edges_scanned = edges + edges_bu — and in a
chain (and only there) the last workgroup out of an election moves the chain on.  What can go wrong there is a
workgroup without candidates that the election does not count, an election word that is not back at zero for the next link, a wave's
share that the sixteen-wave sum drops, or a share of the statistics that is lost or counted twice.

The graphs are the wheels of test_rcm_bu_blocks_gpu: the smallest inputs that reach bottom-up levels in the unordered
sweeps (n of two thousand: two or three blocks of bitmap words for a grid of 512 workgroups, so nearly every workgroup
has nothing) and in the Cuthill-McKee sweep (`big`).  Orders are compared bit for bit with the oracle; the statistics
with tests/golden/rcm_bu_epilogue_stats.json, which tools/record_rcm_stats.py recorded on the commit before the
epilogue changed (three runs per case, all equal, no case left out).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_rcm_bu_blocks_gpu import case, graph, want  # noqa: F401  (case: the graphs' definition, for the reader)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rcm_bu_epilogue_stats.json")
FIELDS = ("edges_scanned", "edges_scanned_bottom_up", "bfs_levels", "bfs_sweeps")
SPARSE = ["n=2047", "n=2048", "n=2049"]                    # most workgroups have nothing
LAUNCHES = ["big", "empty_blocks", "second_wheel_behind"]  # the ordered sweep's levels, empty blocks, labels


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["stats"]


def run(ops, torch, name, bits):
    rp, col, _ = graph(name, bits)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got, stats = ops.rcm_reorder(d(rp), d(col), return_stats=True)
    return got.cpu().numpy(), stats


def check_recorded(name, bits, stats):
    rec = recorded()
    key = "%s/%d" % (name, bits)
    assert key in rec, "no record for %s" % key
    assert {f: stats[f] for f in FIELDS} == rec[key], (key, stats)


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import ops
    return ops, torch


@pytest.mark.gpu
def test_the_record_holds_every_case():
    rec = recorded()
    for name in SPARSE + LAUNCHES:
        for bits in (32, 64):
            assert set(rec["%s/%d" % (name, bits)]) == set(FIELDS)
    assert all(v["edges_scanned_bottom_up"] > 0 for v in rec.values())


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", SPARSE)
def test_most_workgroups_have_nothing(gpu, name, bits):
    got, stats = run(*gpu, name, bits)
    assert got.dtype == (np.int32 if bits == 32 else np.int64)
    assert np.array_equal(got, want(name)), (name, bits)
    assert 0 < stats["edges_scanned_bottom_up"] <= stats["edges_scanned"], stats
    check_recorded(name, bits, stats)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", LAUNCHES)
def test_every_kind_of_launch(gpu, name, bits):
    got, stats = run(*gpu, name, bits)
    assert np.array_equal(got, want(name)), (name, bits)
    assert 0 < stats["edges_scanned_bottom_up"] <= stats["edges_scanned"], stats
    check_recorded(name, bits, stats)


@pytest.mark.gpu
def test_no_state_left_behind(gpu, monkeypatch):
    """big, n=2049, big on one handle: the scratch the small graph's launches run on is full of the big one's, and
    the chains' election word (uc_done) has been through the links of both graphs' sweeps."""
    ops, torch = gpu
    monkeypatch.setattr(ops, "_handles", {})  # a handle nobody has used
    fresh_order, fresh_stats = run(ops, torch, "n=2049", 32)
    monkeypatch.setattr(ops, "_handles", {})  # and another one for the three calls
    first = run(ops, torch, "big", 32)
    second = run(ops, torch, "n=2049", 32)
    third = run(ops, torch, "big", 32)
    assert np.array_equal(first[0], want("big")) and np.array_equal(fresh_order, want("n=2049"))
    assert np.array_equal(third[0], first[0]) and third[1] == first[1], (first[1], third[1])
    assert np.array_equal(second[0], fresh_order) and second[1] == fresh_stats, (fresh_stats, second[1])


def run_plain():
    """`big` in this process (the child of the test below), both index widths."""
    import torch
    from sparsebase_amd import ops
    for bits in (32, 64):
        got, stats = run(ops, torch, "big", bits)
        assert np.array_equal(got, want("big")), bits
        check_recorded("big", bits, stats)
    print("bu epilogue plain ok")


@pytest.mark.gpu
def test_the_kernels_without_the_block_front_end_in_a_child():
    """SBX_RCM_BU_BLOCKS=0 (read once per process) launches the kernels with a lane per vertex, which end in the same
    epilogue; they scan the same candidates, so the recorded statistics hold for them too."""
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_rcm_bu_epilogue_gpu as t\nt.run_plain()\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SBX_RCM_BU_BLOCKS="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "bu epilogue plain ok" in r.stdout, r.stdout + r.stderr
