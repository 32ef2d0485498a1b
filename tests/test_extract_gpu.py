"""The fused feature entry points of include/sbfx.h on the GPU: sbfx_csr_degrees_degree_distribution and
sbfx_csr_bandwidth_profile through ops.csr_degrees_degree_distribution / ops.csr_bandwidth_profile.

Every result is compared bit for bit with two things: a numpy restatement written here, and what the entry points they
are fused from return on the same arrays (sbx_csr_degrees, sbx_csr_degree_distribution, sbx_csr_bandwidth,
sbx_csr_profile, which other tests hold to the reference).  Shapes are the smallest at which the kernels take another
path: one row, a wave more or less, a workgroup more or less, the grid cap of 8192 x 256 rows passed; tiles of 2048
entries with one entry more or less, rows longer than a tile, empty rows on a tile boundary; pointers that are only
4-byte (8-byte for 64-bit words) aligned."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (offsets, ids): SBX_I32, SBX_I64, SBX_I32_N64
TUPLES = {"i32": (np.int32, np.int32), "i64": (np.int64, np.int64), "i32_n64": (np.int64, np.int32)}
GUARD = 0x5A


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import ops
    return ops


def _tdt(dt):
    return torch.from_numpy(np.zeros(0, dt)).dtype


def _view(a, lead=1):
    """`a` on the device as a view that starts `lead` elements into a larger buffer: its pointer is aligned to the
    element and to nothing more.  Returns (view, buffer); the buffer's other bytes are GUARD."""
    buf = torch.full(((len(a) + lead + 1) * a.itemsize,), GUARD, dtype=torch.uint8, device="cuda").view(_tdt(a.dtype))
    view = buf[lead:lead + len(a)]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (buf.data_ptr() + lead * a.itemsize) % 16 and view.data_ptr() % 16 != 0
    return view, buf


def _out_view(count, dt, lead=1):
    buf = torch.full(((count + lead + 1) * np.dtype(dt).itemsize,), GUARD, dtype=torch.uint8, device="cuda").view(_tdt(dt))
    return buf[lead:lead + count], buf


def _guards_intact(buf, count, lead=1):
    raw = buf.view(torch.uint8).cpu().numpy()
    size = raw.size // (count + lead + 1)
    return bool((raw[:lead * size] == GUARD).all() and (raw[(lead + count) * size:] == GUARD).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


# ------------------------------------------------------------------------------------------ degrees + distribution
N_LIST = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, (1 << 21) + 3)  # the last: beyond 8192 workgroups of 256 rows


def _row_ptr(n, ot, seed):
    """Degrees 0 .. 4 with a fifth of the rows empty and one hub of 1000."""
    g = np.random.default_rng(seed)
    deg = g.integers(0, 5, n)
    deg[g.random(n) < 0.2] = 0
    deg[n // 2] = 1000
    return np.concatenate([[0], np.cumsum(deg)]).astype(ot)


def _check_degrees_distribution(ops, rp, idt, fdt):
    n, nnz = len(rp) - 1, int(rp[-1])
    d_rp, _ = _view(rp)
    d_deg, deg_buf = _out_view(n, idt)
    d_dist, dist_buf = _out_view(n, fdt)
    got = ops.csr_degrees_degree_distribution(d_rp, nnz, out=(d_deg, d_dist))
    assert got[0] is d_deg and got[1] is d_dist
    deg, dist = d_deg.cpu().numpy(), d_dist.cpu().numpy()
    assert _guards_intact(deg_buf, n) and _guards_intact(dist_buf, n), "written outside the outputs"
    # the two entry points it is fused from
    p_deg = ops.csr_degrees(d_rp, id_dtype=_tdt(idt)).cpu().numpy()
    p_dist = ops.csr_degree_distribution(d_rp, nnz, dtype=_tdt(fdt)).cpu().numpy()
    assert deg.dtype == p_deg.dtype and _bits(deg) == _bits(p_deg)
    assert dist.dtype == p_dist.dtype and _bits(dist) == _bits(p_dist)
    return deg, dist


@pytest.mark.parametrize("fdt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("tup", list(TUPLES))
def test_degrees_degree_distribution(ops, tup, fdt):
    ot, idt = TUPLES[tup]
    for n in N_LIST:
        rp = _row_ptr(n, ot, n)
        deg, dist = _check_degrees_distribution(ops, rp, idt, fdt)
        want = np.diff(rp.astype(np.int64))
        assert np.array_equal(deg, want.astype(idt)), n
        assert _bits(dist) == _bits(want.astype(fdt) / fdt(rp[-1])), n  # (one conversion and one division per row)
    # without the view, out=None: tensors of the call's own
    rp = _row_ptr(257, ot, 7)
    deg, dist = ops.csr_degrees_degree_distribution(torch.from_numpy(rp).cuda(), int(rp[-1]), dtype=_tdt(fdt),
                                                    id_dtype=_tdt(idt))
    assert deg.dtype == _tdt(idt) and dist.dtype == _tdt(fdt)
    assert np.array_equal(deg.cpu().numpy(), np.diff(rp).astype(idt))
    assert _bits(dist.cpu().numpy()) == _bits(np.diff(rp).astype(fdt) / fdt(rp[-1]))


# offset arrays that only claim their entries (no col is read): degrees and an nnz that no float holds exactly
CLAIMED = {"i32": [0, (1 << 24) + 1, (1 << 24) + 4, (1 << 31) - 1],
           "i32_n64": [0, (1 << 24) + 1, (1 << 24) + 4, (1 << 31) - 1],
           "i64": [0, (1 << 53) + 1, (1 << 53) + 2, 1 << 62]}


@pytest.mark.parametrize("fdt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("tup", list(TUPLES))
def test_degrees_degree_distribution_int_to_float_rounding(ops, tup, fdt):
    ot, idt = TUPLES[tup]
    rp = np.array(CLAIMED[tup], ot)
    deg, dist = _check_degrees_distribution(ops, rp, idt, fdt)
    want = np.diff(rp)
    assert np.array_equal(deg, want.astype(idt))
    assert _bits(dist) == _bits(want.astype(fdt) / fdt(rp[-1]))


@pytest.mark.parametrize("fdt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("tup", list(TUPLES))
def test_degrees_degree_distribution_without_nonzeros(ops, tup, fdt):
    """Every distribution value is 0 / 0: compared with sbx_csr_degree_distribution alone, as raw bits (the host's NaN
    need not carry the device's sign)."""
    ot, idt = TUPLES[tup]
    deg, dist = _check_degrees_distribution(ops, np.zeros(6, ot), idt, fdt)
    assert not deg.any() and np.isnan(dist).all()


def test_degrees_degree_distribution_refusals(ops):
    from sparsebase_amd import capi
    rp = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.csr_degrees_degree_distribution(rp, 0, out=(torch.empty(3, dtype=torch.int32, device="cuda"),
                                                        torch.empty(3, dtype=torch.float16, device="cuda")))
    hd = ops.handle_for(rp.device)
    p = lambda t: t.data_ptr()
    out = torch.empty(3, dtype=torch.float32, device="cuda")
    deg = torch.empty(3, dtype=torch.int32, device="cuda")
    lib = hd.lib.sbfx_csr_degrees_degree_distribution
    assert lib(hd.h, capi.SBX_I32, 3, 0, p(rp), 2, p(deg), p(out)) == 1      # feature_bytes
    assert lib(hd.h, capi.SBX_I32, 3, 0, p(rp), 4, None, p(out)) == 1        # both outputs are required
    assert lib(hd.h, capi.SBX_I32, 3, 0, p(rp), 4, p(deg), None) == 1
    assert lib(hd.h, capi.SBX_I32, -1, 0, p(rp), 4, p(deg), p(out)) == 1
    assert lib(hd.h, capi.SBX_I32, 0, 0, p(rp), 4, None, None) == 0          # no rows: nothing to write


# ------------------------------------------------------------------------------------------ bandwidth + profile
def _restate(rp, col):
    """max |i - j| + 1 (0 without nonzeros); the sum over the rows of i - min(i, smallest column)."""
    rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int64)
    if len(col) == 0:
        return 0, 0
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    filled = np.nonzero(np.diff(rp))[0]
    rowmin = np.minimum.reduceat(col, rp[filled])
    return int(np.abs(rows - col).max()) + 1, int(np.maximum(filled - rowmin, 0).sum())


def _csr(lens, ncols, seed, col_of=None):
    """Sorted rows of the given lengths with distinct columns below ncols (or col_of(row, length))."""
    g = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = [np.sort(g.choice(ncols, int(l), replace=False)) if col_of is None else np.asarray(col_of(i, int(l)), np.int64)
            for i, l in enumerate(lens)]
    return rp, (np.concatenate(cols) if len(cols) else np.zeros(0)).astype(np.int64)


def _lens_with_total(n, total, seed):
    g = np.random.default_rng(seed)
    lens = np.bincount(g.integers(0, n, total), minlength=n)
    lens[g.integers(0, n, n // 5)] = 0
    lens[0] += total - lens.sum()
    return lens


def _bp_cases():
    cases = {"empty": (np.zeros(5, np.int64), np.zeros(0, np.int64)),
             "one_entry": (np.array([0, 0, 1, 1], np.int64), np.array([0], np.int64))}
    for total in (2047, 2048, 2049, 4096, 3 * 2048 + 1):  # a tile is 2048 entries
        cases[f"nnz{total}"] = _csr(_lens_with_total(500, total, total), 4000, total)
    cases["row_of_three_tiles_between_empty_rows"] = _csr([0, 0, 3, 0, 5000, 0, 0, 2, 0], 6000, 1)
    # rows 2 .. 301 are empty and share entry 2048, the first of the second tile, with row 302
    cases["empty_rows_on_a_tile_boundary"] = _csr([1024, 1024] + [0] * 300 + [10, 5], 3000, 2)
    cases["empty_first_and_last_rows"] = _csr([0, 0, 7, 3, 0, 9, 0], 40, 3)
    cases["above_the_diagonal"] = _csr([3] * 700, 0, 4, col_of=lambda i, l: i + 1 + np.arange(l) * 2)
    return cases


BP_CASES = _bp_cases()


def _check_bandwidth_profile(ops, tup, rp, col, view=False):
    ot, idt = TUPLES[tup]
    d_rp = torch.from_numpy(rp.astype(ot)).cuda()
    d_col = _view(col.astype(idt))[0] if view else torch.from_numpy(col.astype(idt)).cuda()
    got = ops.csr_bandwidth_profile(d_rp, d_col)
    parents = (ops.csr_bandwidth(d_rp, d_col), ops.csr_profile(d_rp, d_col))
    assert got == parents, (got, parents)
    assert got == _restate(rp, col), (got, _restate(rp, col))
    return got


@pytest.mark.parametrize("name", list(BP_CASES))
@pytest.mark.parametrize("tup", list(TUPLES))
def test_bandwidth_profile(ops, tup, name):
    rp, col = BP_CASES[name]
    got = _check_bandwidth_profile(ops, tup, rp, col)
    if name == "above_the_diagonal":
        assert got[1] == 0
    if len(col):  # a col pointer that is aligned to its element and no more: the scalar loads of sbx_load_items8
        assert _check_bandwidth_profile(ops, tup, rp, col, view=True) == got


@pytest.mark.parametrize("tup", list(TUPLES))
def test_bandwidth_profile_of_unsorted_rows(ops, tup):
    """One row reversed, one rotated: the pass raises its flag and the profile comes from the smallest column of every
    row.  The bandwidth is the sorted matrix's, the profile sbx_csr_profile's."""
    rp, col = BP_CASES["nnz4096"]
    sorted_result = _check_bandwidth_profile(ops, tup, rp, col)
    long_rows = np.nonzero(np.diff(rp) >= 3)[0]
    a, b = long_rows[1], long_rows[-2]
    for which in ("reversed", "rotated", "both"):
        c = col.copy()
        if which != "rotated":
            c[rp[a]:rp[a + 1]] = c[rp[a]:rp[a + 1]][::-1]
        if which != "reversed":
            c[rp[b]:rp[b + 1]] = np.roll(c[rp[b]:rp[b + 1]], 1)
        assert _check_bandwidth_profile(ops, tup, rp, c) == sorted_result, which
        assert _check_bandwidth_profile(ops, tup, rp, c, view=True) == sorted_result, which


def test_bandwidth_profile_i64_columns_beyond_32_bits(ops):
    base = 1 << 32
    rp, col = _csr([3, 0, 2500, 1, 4], 0, 5, col_of=lambda i, l: base + i * 7 + np.arange(l) * 3)
    bw, pr = _check_bandwidth_profile(ops, "i64", rp, col)
    assert bw > base and pr == 0  # (the largest distance is a column's: n < 2^31)
    _check_bandwidth_profile(ops, "i64", rp, col, view=True)


def test_bandwidth_profile_refusals(ops):
    rp = torch.zeros(4, dtype=torch.int64, device="cuda")
    col = torch.zeros(0, dtype=torch.int32, device="cuda")
    assert ops.csr_bandwidth_profile(rp, col) == (0, 0)  # SBX_I32_N64 without nonzeros
    from sparsebase_amd import capi
    hd = ops.handle_for(rp.device)
    import ctypes as C
    bw, pr = C.c_int64(7), C.c_int64(7)
    lib = hd.lib.sbfx_csr_bandwidth_profile
    assert lib(hd.h, capi.SBX_I64, 3, 0, rp.data_ptr(), None, C.byref(bw), None) == 1
    assert lib(hd.h, capi.SBX_I64, 3, 5, rp.data_ptr(), None, C.byref(bw), C.byref(pr)) == 1
    assert lib(hd.h, capi.SBX_I32_N64, 3, 1 << 31, rp.data_ptr(), rp.data_ptr(), C.byref(bw), C.byref(pr)) == 5
    assert lib(hd.h, capi.SBX_I32, 1 << 31, 1, rp.data_ptr(), rp.data_ptr(), C.byref(bw), C.byref(pr)) == 1


def test_the_fused_call_launches_no_more_than_either_parent(ops):
    """With the handle's profile counters on, on a sorted matrix: the `feature` launches of the fused call against those
    of sbx_csr_bandwidth and of sbx_csr_profile, all counted here."""
    rp, col = BP_CASES["nnz6145"]
    d_rp, d_col = torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(col.astype(np.int32)).cuda()

    def launches(fn):
        ops.profile_enable(True)
        try:
            fn()
            return ops.profile_report().get("feature", (0.0, 0, 0))[1]
        finally:
            ops.profile_enable(False)
    fused = launches(lambda: ops.csr_bandwidth_profile(d_rp, d_col))
    bandwidth = launches(lambda: ops.csr_bandwidth(d_rp, d_col))
    profile = launches(lambda: ops.csr_profile(d_rp, d_col))
    assert fused > 0 and bandwidth > 0 and profile > 0
    assert fused <= bandwidth and fused <= profile, (fused, bandwidth, profile)
    # and the degree pair: one launch for two
    one = launches(lambda: ops.csr_degrees_degree_distribution(d_rp, len(col)))
    two = launches(lambda: (ops.csr_degrees(d_rp), ops.csr_degree_distribution(d_rp, len(col))))
    assert 0 < one < two, (one, two)
