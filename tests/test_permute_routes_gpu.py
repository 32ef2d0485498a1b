"""Which kernels a permute runs, not only what it returns: the parity tests compare results, and a driver that sent every
row down the radix path would still pass them.  Each case takes the launch counts of the profiler's permute groups
(ops.profile_enable / ops.profile_report) around ONE call, asserts the difference and the result against the oracle.
With the profiler on the sort stage does not fork; the stream side is tests/test_stream_order_gpu.py's.
"""
import numpy as np
import pytest

from sparsebase_amd import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GROUPS = ("permute_prep", "permute_tile", "permute_block", "permute_long")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def csr(lens, m, seed):
    """Rows of the given lengths, each with distinct sorted columns below m; values 0, 1, 2, ..."""
    g = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(g.choice(m, int(l), replace=False)) for l in lens]).astype(np.int32)
    return rp, col, np.arange(len(col), dtype=np.float32)


def short_lens(count, most, seed):
    return [int(x) for x in np.random.default_rng(seed).integers(0, most + 1, count)]


def counted(call):
    """(result of call(), launches it added per group) — the profiler is off again whatever happens."""
    from sparsebase_amd import ops
    ops.profile_enable(True)
    try:
        before = ops.profile_report()
        got = call()
        torch.cuda.synchronize()
        after = ops.profile_report()
    finally:
        ops.profile_enable(False)
    return got, tuple(after.get(k, (0, 0, 0))[1] - before.get(k, (0, 0, 0))[1] for k in GROUPS)


def permute_case(oracle, rp, col, val, row_map, col_map):
    from sparsebase_amd import ops
    n, m = len(rp) - 1, 4096 if col.max() < 4096 else 65536
    ro = synth.random_permutation(n, 11)
    co = {None: None, "random": synth.random_permutation(m, 12), "identity": np.arange(m, dtype=np.int32)}[col_map]
    got, counts = counted(lambda: ops.permute_csr(n, m, dev(rp), dev(col), dev(val), dev(ro), dev(co)))
    for g, w in zip(got, oracle.permute_csr(rp, col, val, ro, co)):
        assert np.array_equal(g.cpu().numpy(), w)
    return counts


D_LENS = short_lens(25, 100, 5) + [200, 400, 900, 1500, 3000, 6000] + short_lens(25, 100, 6)
F_LENS = short_lens(20, 100, 7) + [20000] + short_lens(20, 100, 8)


def test_rowwise_sorted_rows_are_copied(oracle):
    # A: k_rowwise_prep, three classification kernels, k_tile_rows | k_permute_copy
    rp, col, val = csr(short_lens(200, 100, 1), 4096, 2)
    assert permute_case(oracle, rp, col, val, "random", None) == (5, 1, 0, 0)


def test_rowwise_unsorted_row_redoes_through_the_tile_kernels(oracle):
    # B: A's launches, then the redo: classification again, k_tile_first | k_permute_copy, k_permute_tile and its
    # radix twin | - | k_fix_dup_runs
    rp, col, val = csr(short_lens(200, 100, 1), 4096, 2)
    r = int(np.argmax(np.diff(rp) >= 2))
    col[rp[r]], col[rp[r + 1] - 1] = col[rp[r + 1] - 1], col[rp[r]]
    assert permute_case(oracle, rp, col, val, "random", None) == (9, 3, 0, 1)


def test_relabelled_short_rows_take_tile2(oracle):
    # C: two map kernels, k_rowwise_prep, k_fill_index, three classification kernels | k_permute_tile2 | - | k_fix_dup_runs
    rp, col, val = csr(short_lens(300, 128, 3), 4096, 4)
    assert permute_case(oracle, rp, col, val, "random", "random") == (7, 1, 0, 1)


def test_six_row_classes(oracle):
    # D: as C | k_permute_tile2 | five k_rows_quad, k_permute_block_rows (the 512-slot class), k_permute_rows_radix |
    # k_fix_dup_runs
    rp, col, val = csr(D_LENS, 65536, 9)
    assert permute_case(oracle, rp, col, val, "random", "random") == (7, 1, 7, 1)


def test_eight_byte_values_have_no_8192_slot_class(oracle):
    # E: D with float64 values: five classes and k_permute_rows_radix; the 6000-entry row is long
    rp, col, val = csr(D_LENS, 65536, 9)
    counts = permute_case(oracle, rp, col, val.astype(np.float64), "random", "random")
    assert counts[:3] == (7, 1, 6) and counts[3] > 1


def test_long_row_goes_through_the_segment_path(oracle):
    # F: k_long_seg_offsets, _gather, _hist, _scan, _partition, two k_rows_quad, k_permute_rows_radix, k_fix_dup_runs:
    # nothing handed to the global radix sort
    rp, col, val = csr(F_LENS, 65536, 10)
    assert permute_case(oracle, rp, col, val, "random", "random") == (7, 1, 0, 9)


def test_segment_path_declines_an_ordered_long_row(oracle):
    # G: F, and k_long_lengths, k_long_gather, k_long_scatter for the row the identity column map leaves in order
    rp, col, val = csr(F_LENS, 65536, 10)
    assert permute_case(oracle, rp, col, val, "random", "identity") == (7, 1, 0, 12)


def test_constructor_sort_takes_the_global_radix_path(oracle):
    # H: k_rowwise_prep, three classification kernels, k_tile_first | k_permute_tile and its radix twin | - |
    # k_long_lengths, k_long_gather, k_long_scatter, k_fix_dup_runs (the radix sort's kernels count in groups of their own)
    from sparsebase_amd import ops
    rp, col, val = csr(F_LENS, 65536, 10)
    r = int(np.argmax(np.diff(rp)))
    col[rp[r]:rp[r + 1]] = np.random.default_rng(13).permutation(col[rp[r]:rp[r + 1]])
    n, m, dc, dv = len(rp) - 1, 65536, dev(col), dev(val)
    _, counts = counted(lambda: ops.csr_sort_rows_(n, m, dev(rp), dc, dv))
    want_c, want_v = oracle.csr_sort_rows(rp, col, val, m=m)
    assert np.array_equal(dc.cpu().numpy(), want_c) and np.array_equal(dv.cpu().numpy(), want_v)
    assert counts == (5, 2, 0, 4)
