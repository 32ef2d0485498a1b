"""Which kernels a Gray call runs, not only what it returns: the parity tests compare results, and a driver that sent
every matrix down the tile kernels would still pass them.  Each case takes the launch count of the profiler's `gray`
group (ops.profile_enable / ops.profile_report) around ONE call and asserts that count and the result against the oracle.
The key stage's routes are the ones sbx_gray.hip's header names; the ordering stage's forms are sbx_gray_order.hip's
(its calls count the key stage's launches too; the scans and radix sorts count in groups of their own).
"""
import numpy as np
import pytest

from sparsebase_amd import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def counted(call):
    """(result of call(), launches it added to the gray group) — the profiler is off again whatever happens."""
    from sparsebase_amd import ops
    ops.profile_enable(True)
    try:
        before = ops.profile_report()
        got = call()
        torch.cuda.synchronize()
        after = ops.profile_report()
    finally:
        ops.profile_enable(False)
    return got, after.get("gray", (0, 0, 0))[1] - before.get("gray", (0, 0, 0))[1]


def rows(lens, m, seed):
    from test_gpu_parity import _mixed_rows
    return _mixed_rows(np.random.default_rng(seed), len(lens), m, lens)


def keys_case(oracle, rp, col, m, res, thr, wide=False):
    """Launches of one ops.gray_row_keys call whose degrees, keys and band counters equal the oracle's."""
    from sparsebase_amd import ops
    idt = np.int64 if wide else np.int32
    (deg, key, counts), launches = counted(lambda: ops.gray_row_keys(m, dev(rp.astype(idt)), dev(col.astype(idt)), res, thr))
    wdeg, wkey, wcounts = oracle.gray_row_keys(rp, col, m, res, thr)
    assert deg.dtype == (torch.int64 if wide else torch.int32)
    assert np.array_equal(deg.cpu().numpy(), wdeg)
    assert np.array_equal(key.cpu().numpy().view(np.uint64), wkey)
    assert list(counts) == wcounts.tolist()
    print("gray_row_keys launches:", launches)
    return launches


def banded_lens(special):
    """lens of test_gray_row_keys_banded_with_a_few_medium_rows, with the given rows above GR_SHORT_MAX entries"""
    lens = np.random.default_rng(5).integers(1, 40, 6000)
    for r, l in special:
        lens[r] = l
    return lens


def power_law_lens(res, thr, m):
    """lens of test_gray_row_keys_power_law_path"""
    g = np.random.default_rng(1000 + res + thr)
    n = 3000
    lens = g.integers(0, 65, n)
    lens[g.integers(0, n, 400)] = g.integers(65, 1025, 400)
    lens[g.integers(0, n, 60)] = g.integers(1025, 9000, 60)
    lens[[5, 6, 7]] = (40000, 1024, 1025)
    lens[[100, 101, 102, 103]] = (64, 65, 0, 33)
    lens[n - 1] = 1027
    return np.minimum(lens, m)


# ----------------------------------------------------------------------------- the key stage
def test_banded_kernel_alone(oracle):
    # A: k_gray_rows_short met no row above GR_SHORT_MAX entries
    rp, col = synth.banded_symmetric(4096, 40, 9, 1)
    assert keys_case(oracle, rp, col, 4096, 32, 10) == 1


def test_banded_kernel_then_medium_and_long_leftovers(oracle):
    # B: k_gray_rows_short | k_gray_list_medium, k_gray_rows_medium, k_gray_units_finish | k_gray_long_rows, k_gray_long_finish
    lens = banded_lens(((50, 100), (900, 65), (1700, 1024), (2500, 1025), (3300, 5000), (4100, 8192), (4900, 8193), (5700, 30000)))
    rp, col = rows(lens, 32 * 4096, 5)
    assert keys_case(oracle, rp, col, 32 * 4096, 32, 10) == 6


def test_banded_kernel_then_long_leftovers_only(oracle):
    # C: no row of 65 .. 8192 entries: k_gray_rows_short | k_gray_long_rows, k_gray_long_finish
    lens = banded_lens(((4900, 8193), (5700, 30000)))
    assert not np.any((lens > 64) & (lens <= 8192))
    rp, col = rows(lens, 32 * 4096, 5)
    assert keys_case(oracle, rp, col, 32 * 4096, 32, 10) == 3


def test_power_law_kernels_tiny_and_listed(oracle):
    # D: k_gray_rows_short (stopped) | k_gray_rows_tiny, k_gray_rows_listed, k_gray_rows_medium, k_gray_units_finish, k_gray_fold
    m = 32 * 1024
    rp, col = rows(power_law_lens(32, 10, m), m, 1010)
    assert keys_case(oracle, rp, col, m, 32, 10) == 6


def test_power_law_kernels_balanced(oracle):
    # E: a resolution of at most GR_TINY with the threshold below it: k_gray_rows_balanced instead of tiny + listed
    m = 14 * 1024
    rp, col = rows(power_law_lens(14, 3, m), m, 1017)
    assert keys_case(oracle, rp, col, m, 14, 3) == 5


def test_low_resolution_takes_the_tile_kernels(oracle):
    # F: resolution 8 needs 9 counter levels: k_gray_prep, k_gray_tile, k_gray_finish
    lens = np.random.default_rng(108).integers(0, 65, 600)
    rp, col = rows(lens, 8 * 40, 109)
    assert keys_case(oracle, rp, col, 8 * 40, 8, 7) == 3


def test_power_law_kernels_on_64_bit_arrays(oracle):
    # G: D through the file's second compilation
    m = 32 * 1024
    rp, col = rows(power_law_lens(32, 10, m), m, 1010)
    assert keys_case(oracle, rp, col, m, 32, 10, wide=True) == 6


def test_long_row_list_overflow_starts_over_with_the_tile_kernels(oracle):
    # H: more than GR_LONG_LIST rows above GR_MED_MAX entries: k_gray_rows_short | k_gray_prep, k_gray_tile, k_gray_finish
    heavy, m = 4100, 16384
    lens = np.concatenate([[3, 0, 17], np.full(heavy, 8193), [1, 40]])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([[1, 5, 9], np.arange(100, 117), np.tile(np.arange(8193), heavy), [16383], np.arange(0, 16384 - 200, 400)[:40]]).astype(np.int32)
    assert len(col) == rp[-1]
    assert keys_case(oracle, rp, col, m, 32, 10) == 4


# ----------------------------------------------------------------------------- the ordering stage
def order_case(oracle, rp, col, m, res, thr, grp, wide=False):
    """Launches of one ops.gray_reorder call whose result equals the stable model's row for row."""
    from sparsebase_amd import ops
    from test_gpu_parity import _gray_stable_model
    idt = np.int64 if wide else np.int32
    inv, launches = counted(lambda: ops.gray_reorder(m, dev(rp.astype(idt)), dev(col.astype(idt)), res, thr, grp))
    assert inv.dtype == (torch.int64 if wide else torch.int32)
    deg, key, counts = oracle.gray_row_keys(rp, col, m, res, thr)
    model, _ = _gray_stable_model(deg, key, counts, min(res, m), thr, grp)
    assert np.array_equal(inv.cpu().numpy().astype(np.int64), model)
    print("gray_reorder launches:", launches)
    return launches


def test_one_sort_with_the_row_id_in_the_key(oracle):
    # I: 3 + 32 + 4 criterion bits and 13 id bits: the key stage's six, then k_go_present, k_go_sections, k_go_composite
    # (no payload, no emit kernel: the sort's last pass writes the inverse permutation)
    rp, col = synth.rmat_symmetric(13, 8, seed=5)
    assert order_case(oracle, rp, col, len(rp) - 1, 32, 10, 4) == 9


def test_one_sort_with_a_payload(oracle):
    # J: 48 + class + degree bits fit 64, but not with the id bits: the same, and k_go_emit
    m = 48 * 1000
    rp, col = rows(power_law_lens(48, 10, m), m, 1058)
    assert order_case(oracle, rp, col, m, 48, 10, 4) == 10


def test_three_sorts_at_resolution_64(oracle):
    # K: the key stage's six, then k_go_degree_keys, k_go_sections, k_go_signed_keys, k_go_class_keys, k_go_emit
    rp, col = synth.rmat_symmetric(13, 8, seed=5)
    assert order_case(oracle, rp, col, len(rp) - 1, 64, 10, 4) == 11


def test_one_sort_on_64_bit_arrays_widens_the_result(oracle):
    # L: I, and k_go_widen behind the sort
    rp, col = synth.rmat_symmetric(13, 8, seed=5)
    assert order_case(oracle, rp, col, len(rp) - 1, 32, 10, 4, wide=True) == 10
