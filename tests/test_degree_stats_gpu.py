"""sbxstat_degree_stats on the MI355X (ops.degree_stats): every integer field equals the restatement of
test_degree_stats_host.py exactly; sum_log is within (n + 2) 2^-53 relative of the fsum value (one rounding per
logarithm, here counted as two, and at most n - 1 per addition chain) and has the same bits in two calls and on two
handles.

The shapes are the smallest at which the kernels can go wrong: a tile of the pass is 4096 degrees (256 threads, four
steps of four consecutive degrees: 16-byte loads), a pass has at most SBXSTAT_MAX_GRID = 512 workgroups, the select
takes 12-bit digits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sparsebase_amd import capi, ops
from test_degree_stats_host import degree_stats

pytestmark = pytest.mark.gpu

WORDS = {"w32": torch.int32, "w64": torch.int64}
TILE = 4096
INT_FIELDS = ("count", "sum", "min", "max", "zeros", "sumsq", "median_lo", "median_hi")


def _ptr(deg, start=0):
    return np.concatenate([[start], start + np.cumsum(np.asarray(deg, np.int64))]).astype(np.int64)


def _dev(ptr, word):
    assert word == "w64" or np.max(ptr) < 2 ** 31, "the offsets do not fit 32-bit words"
    return torch.as_tensor(np.asarray(ptr, np.int64)).to(WORDS[word]).cuda()


def _check(ptr, words=tuple(WORDS), want=None, **kw):
    want = want or degree_stats(ptr)
    n = want["count"]
    for word in words:
        got = ops.degree_stats(_dev(ptr, word), **kw)
        for k in INT_FIELDS:
            w = want[k] if kw.get("median", True) or not k.startswith("median") else -1
            assert got[k] == w, f"{word} {k}: {got[k]} != {w}"
        if kw.get("log", True):
            assert abs(got["sum_log"] - want["sum_log"]) <= (n + 2) * 2.0 ** -53 * abs(want["sum_log"]), (word, got["sum_log"], want["sum_log"])
        else:
            assert got["sum_log"] == 0.0
    return want


def _power_law(n, seed, cap=2 ** 20):
    g = np.random.default_rng(seed)
    return np.minimum(g.pareto(1.1, n).astype(np.int64) + (g.random(n) < 0.7), cap)


@pytest.mark.parametrize("word", list(WORDS))
def test_sizes_around_a_wave_a_workgroup_and_a_tile(word):
    g = np.random.default_rng(1)
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1):
        _check(_ptr(g.integers(0, 21, n)), (word,))


@functools.lru_cache(None)
def _big(n, seed):
    ptr = _ptr(_power_law(n, seed))
    return ptr, degree_stats(ptr)


@pytest.mark.parametrize("word", list(WORDS))
def test_more_tiles_than_one_workgroup_takes_2_20_plus_3(word):
    ptr, want = _big(2 ** 20 + 3, 2)
    _check(ptr, (word,), want=want)


def test_more_tiles_than_workgroups():
    ptr, want = _big(513 * TILE + 5, 3)  # (a grid stride: 514 tiles for at most 512 workgroups)
    _check(ptr, ("w32",), want=want)


@pytest.mark.parametrize("kind", ["all_equal", "all_zero", "one_hub", "power_law"])
def test_distributions(kind):
    n = 5001
    deg = {"all_equal": np.full(n, 7), "all_zero": np.zeros(n), "power_law": _power_law(n, 4)}.get(kind)
    if deg is None:
        deg = np.ones(n)
        deg[1234] = 2 ** 27
    st = _check(_ptr(deg))
    if kind == "all_zero":
        assert st["zeros"] == n and st["sum_log"] == 0.0


def test_median_ranks_part_at_the_top_digit():
    g = np.random.default_rng(5)
    st = _check(_ptr(g.permutation(np.repeat([4095, 4096], 3000))))
    assert (st["median_lo"], st["median_hi"]) == (4095, 4096)


def test_median_ranks_part_at_the_last_digit():
    g = np.random.default_rng(6)
    for count, words in ((2500, ("w64",)), (50, ("w32", "w64"))):  # (2500 of each do not fit 32-bit offsets)
        st = _check(_ptr(g.permutation(np.repeat([2 ** 24 + 5, 2 ** 24 + 6], count))), words)
        assert (st["median_lo"], st["median_hi"]) == (2 ** 24 + 5, 2 ** 24 + 6)
    # and in the middle one of three
    for count, words in ((2500, ("w64",)), (10, ("w32", "w64"))):
        st = _check(_ptr(g.permutation(np.repeat([(5 << 24) + (7 << 12) + 9, (5 << 24) + (8 << 12) + 9], count))), words)
        assert st["median_hi"] - st["median_lo"] == 1 << 12


@pytest.mark.parametrize("bits,word", [(20, "w32"), (20, "w64"), (30, "w32"), (30, "w64"), (40, "w64"), (52, "w64")])
def test_two_three_four_and_five_digit_passes(bits, word):
    g = np.random.default_rng(bits)
    if word == "w32" and bits == 30:  # (the sum has to fit the word)
        deg = g.integers(0, 100, 3001)
        deg[1000] = 2 ** 30 - 1
    else:
        n = 2047 if word == "w32" else 3001
        deg = g.integers(0, 2 ** bits, n)
        deg[n // 3] = 2 ** bits - 1
    st = _check(_ptr(deg), (word,))
    assert st["max"] == 2 ** bits - 1 and (bits < 40 or st["sumsq"] >> 64)


def test_six_digit_passes():
    st = _check(_ptr([2 ** 60 + 3, 0, 2 ** 61, 2 ** 60 + 1, 7, 2 ** 60 + 2]), ("w64",))
    assert (st["median_lo"], st["median_hi"]) == (2 ** 60 + 1, 2 ** 60 + 2) and st["sumsq"] >> 64
    g = np.random.default_rng(7)
    deg = g.integers(0, 50, 4097)
    deg[[5, 4000]] = [2 ** 61 + 12345, 2 ** 60]
    _check(_ptr(deg), ("w64",))


def test_first_offset_not_zero_and_unaligned_array():
    g = np.random.default_rng(8)
    ptr = _ptr(g.integers(0, 9, 10000), start=777)
    want = _check(ptr)
    for word in WORDS:  # a view one word into an allocation: no 16-byte loads
        buf = torch.empty(len(ptr) + 1, dtype=WORDS[word], device="cuda")
        buf[1:] = _dev(ptr, word)
        got = ops.degree_stats(buf[1:])
        assert all(got[k] == want[k] for k in INT_FIELDS)


def test_flags_off():
    g = np.random.default_rng(9)
    ptr = _ptr(g.integers(1, 30, 9000))
    _check(ptr, median=False, log=True)
    _check(ptr, median=True, log=False)
    _check(ptr, median=False, log=False)


def test_bad_arguments():
    for word in WORDS:
        with pytest.raises(capi.SbxError) as e:
            ops.degree_stats(_dev([0, 5, 4, 9], word))
        assert e.value.status == 1
        with pytest.raises(capi.SbxError) as e:
            ops.degree_stats(_dev([0], word))
        assert e.value.status == 1
    big = _ptr(np.random.default_rng(10).integers(0, 5, 70000))
    big[40000:] -= big[40000] - big[39999] + 1  # one step down in the middle
    with pytest.raises(capi.SbxError) as e:
        ops.degree_stats(_dev(big, "w64"))
    assert e.value.status == 1


def test_sum_log_has_the_same_bits_in_two_calls_and_on_two_handles():
    ptr = _ptr(_power_law(300000, 11) + 1)
    for word in WORDS:
        t = _dev(ptr, word)
        a, b = ops.degree_stats(t), ops.degree_stats(t)
        assert np.float64(a["sum_log"]).tobytes() == np.float64(b["sum_log"]).tobytes()
        other = ops.Handle(torch.cuda.current_device())
        try:
            other.bind_stream()
            out = capi.StatDegrees()
            other.check(other.lib.sbxstat_degree_stats(other.h, capi.SBX_I32 if word == "w32" else capi.SBX_I64, t.numel() - 1,
                                                       C.c_void_p(t.data_ptr()), capi.STAT_LOG, C.byref(out)))
        finally:
            other.lib.sbx_destroy(other.h)
        assert np.float64(out.sum_log).tobytes() == np.float64(a["sum_log"]).tobytes()
        assert (out.median_lo, out.median_hi) == (-1, -1) and out.max == a["max"]
