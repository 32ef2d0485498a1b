"""GPU tests of include/sbmv.h through ops.csr_spmv and ops.csr_check, for every value type and every index tuple,
against tests/spmv_restate.py.

  1. exact cases       values and x are integers in [-8, 8]: every partial sum of a row is exact in float32 up to 2^17
                       entries per row, so y equals the restatement bit for bit whatever the order of the sum
  2. the rounding bound  |y_i - yhat_i| <= gamma(k, u) S_i + gamma(k, u_wide) S_i for k rounded products summed in any
                       order (with or without fused multiply-add): nothing here is a measured tolerance
  3. determinism       two calls and a second handle on another stream: identical bytes
  4. pattern           val=None equals val=ones
  5. column guard      columns m, m + 1 and -1 contribute nothing; x is a slice inside a larger tensor
  6. sbmv_csr_check    accepts every shape of 1, refuses five malformed inputs with the position in the message
  7. with RCM          spmv(P A P^T, P x)[order[i]] == spmv(A, x)[i]

The kernels' tile is MV_TILE = 2048 entries (sbx_spmv.hip), below the staircase's 8193: no wider shape is needed.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmv_restate as mv  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TUPLES = {"i32": (np.int32, np.int32), "i64": (np.int64, np.int64), "i32_n64": (np.int64, np.int32)}  # (offsets, ids)
VTS = {"f32": np.float32, "f64": np.float64, "i32": np.int32, "i64": np.int64}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import ops
    return ops


def _from_lengths(lengths, m, seed):
    rp = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])
    return len(lengths), m, rp, np.random.default_rng(seed).integers(0, m, rp[-1])


def _hub(where):
    g = np.random.default_rng(61)
    lengths = g.integers(0, 5, 3000).tolist()
    lengths.insert({"first": 0, "middle": 1500, "last": 3000}[where], 70000)
    return _from_lengths(lengths, 5000, 62)


def _staircase():
    """Row i has i entries for i = 0 ... 1100, then the rows around the tile's multiples with empty rows between: every
    row length and every alignment of a row against a tile boundary up to there occurs."""
    lengths = list(range(1101))
    for k in (2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193):
        lengths += [0, k]
    return _from_lengths(lengths + [0], 3000, 63)


def _power_law():
    from sparsebase_amd import synth
    rp, col = synth.rmat_symmetric(13, 16, seed=64, idx_dtype=np.int64)
    return len(rp) - 1, len(rp) - 1, rp, col


SHAPES = {
    "n0": lambda: (0, 5, np.zeros(1, np.int64), np.zeros(0, np.int64)),
    "nnz0": lambda: (5, 4, np.zeros(6, np.int64), np.zeros(0, np.int64)),
    "one": lambda: (1, 1, np.array([0, 1]), np.array([0])),
    "staircase": _staircase,
    "hub_first": lambda: _hub("first"),
    "hub_middle": lambda: _hub("middle"),
    "hub_last": lambda: _hub("last"),
    "ones": lambda: _from_lengths([1] * 20000, 20000, 65),
    "wide": lambda: _from_lengths(np.random.default_rng(66).integers(100, 300, 300), 70000, 67),
    "tall": lambda: _from_lengths(np.random.default_rng(68).integers(0, 3, 70000), 300, 69),
    "dups": lambda: _from_lengths(np.random.default_rng(70).integers(0, 40, 500), 7, 71),
    "power_law": _power_law,
}


@functools.lru_cache(None)
def shape(name):
    n, m, rp, col = SHAPES[name]()
    return n, m, np.asarray(rp, np.int64), np.asarray(col, np.int64)


@functools.lru_cache(None)
def small_ints(name, vt):
    """(val, x): integers in [-8, 8] in the value type."""
    n, m, rp, col = shape(name)
    g = np.random.default_rng(72)
    return g.integers(-8, 9, len(col)).astype(VTS[vt]), g.integers(-8, 9, m).astype(VTS[vt])


@functools.lru_cache(None)
def exact_want(name, vt, pattern=False):
    n, m, rp, col = shape(name)
    val, x = small_ints(name, vt)
    val = None if pattern else val
    if vt in ("i32", "i64"):
        return mv.spmv_int(rp, col, x, val, m)
    y, _, _ = mv.spmv_wide(rp, col, x, val, m, wide=np.float64)
    return y.astype(VTS[vt])  # (integers below 2^23: exact in both formats)


def dev(a, dt=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a if dt is None else a.astype(dt))).cuda()


def prefilled(n, vt):
    dtype = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "i64": torch.int64}[vt]
    return torch.full((n,), float("nan") if vt in ("f32", "f64") else -1, dtype=dtype, device="cuda")


def same_bits(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def first_difference(got, want):
    got = got.cpu().numpy()
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{got.dtype}{got.shape} for {want.dtype}{want.shape}"
    width = got.itemsize
    bad = np.nonzero((got.view(np.uint8).reshape(-1, width) != want.view(np.uint8).reshape(-1, width)).any(axis=1))[0]
    return f"{len(bad)} of {len(want)} rows differ, first {bad[:5]}: {got[bad[:5]]} for {want[bad[:5]]}"


CASES = [(t, v, s) for t in TUPLES for v in VTS for s in SHAPES]


@pytest.mark.parametrize("tup,vt,name", CASES, ids=["-".join(c) for c in CASES])
def test_exact(ops, tup, vt, name):
    n, m, rp, col = shape(name)
    ot, idt = TUPLES[tup]
    val, x = small_ints(name, vt)
    want = exact_want(name, vt)
    y = prefilled(n, vt)
    got = ops.csr_spmv(dev(rp, ot), dev(col, idt), dev(x), val=dev(val), m=m, out=y)
    assert got is y
    assert same_bits(y, want), first_difference(y, want)  # (NaN or -1 left: a row that was not written)
    ops.csr_check(dev(rp, ot), dev(col, idt), m)  # 6: every shape here is well-formed


# ---- 2
BOUND_SHAPES = ("staircase", "hub_first", "hub_middle", "hub_last")


def _wide_for(vt, nnz):
    """f32: float64.  f64: np.longdouble where its epsilon is below 2^-60, else exact fractions on the shapes of at most
    2000 entries (None: this platform has no wider sum for this shape)."""
    if vt == "f32":
        return np.float64
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        return np.longdouble
    return "fraction" if nnz <= 2000 else None


@functools.lru_cache(None)
def uniform_data(name, vt, k):
    n, m, rp, col = shape(name)
    g = np.random.default_rng(100 + k)

    def draw(count):  # uniform in (-1, 1), kept 2^-20 away from 0 (no product is subnormal), times 10^k
        u = g.uniform(-1.0, 1.0, count)
        u = np.where(np.abs(u) < 2.0 ** -20, 2.0 ** -20, u)
        return (u * 10.0 ** k).astype(VTS[vt])
    val, x = draw(len(col)), draw(m)
    wide = _wide_for(vt, len(col))
    return val, x, (None if wide is None else mv.spmv_wide(rp, col, x, val, m, wide=wide))


@pytest.mark.parametrize("name", BOUND_SHAPES)
@pytest.mark.parametrize("vt", ["f32", "f64"])
@pytest.mark.parametrize("tup", list(TUPLES))
def test_rounding_bound(ops, tup, vt, name):
    n, m, rp, col = shape(name)
    ot, idt = TUPLES[tup]
    u = 2.0 ** -24 if vt == "f32" else 2.0 ** -53
    length = np.diff(rp)
    drp, dcol = dev(rp, ot), dev(col, idt)
    checked = 0
    for k in range(-3, 4):
        val, x, wide = uniform_data(name, vt, k)
        if wide is None:
            continue
        yhat, S, u_wide = wide
        y = ops.csr_spmv(drp, dcol, dev(x), val=dev(val), m=m, out=prefilled(n, vt)).cpu().numpy().astype(np.longdouble)
        bound = (mv.gamma(length, u) + mv.gamma(length, u_wide)) * S.astype(np.longdouble)
        err = np.abs(y - yhat.astype(np.longdouble))
        worst = int(np.argmax(err - bound))
        print(f"{name} {vt} {tup} k={k}: largest error / bound = {float(np.max(err[bound > 0] / bound[bound > 0])):.3g}")
        assert (err <= bound).all(), f"k={k}: row {worst} of {length[worst]} entries: error {err[worst]} over the bound {bound[worst]}"
        checked += 1
    assert checked or vt == "f64"  # (f64 without a wider format: only the shapes of at most 2000 entries)


# ---- 3
@pytest.mark.parametrize("name", ["hub_middle", "power_law"])
@pytest.mark.parametrize("vt", ["f32", "f64"])
def test_determinism(ops, vt, name):
    from sparsebase_amd import capi
    n, m, rp, col = shape(name)
    val, x, _ = uniform_data(name, vt, 0) if name in BOUND_SHAPES else _power_law_uniform(vt)
    drp, dcol, dval, dx = dev(rp, np.int32), dev(col, np.int32), dev(val), dev(x)
    y1 = ops.csr_spmv(drp, dcol, dx, val=dval).cpu().numpy()
    y2 = ops.csr_spmv(drp, dcol, dx, val=dval).cpu().numpy()
    torch.cuda.synchronize()
    lib, h, s = capi.load(), C.c_void_p(), torch.cuda.Stream()
    assert lib.sbx_create(torch.cuda.current_device(), C.byref(h)) == 0
    try:
        assert lib.sbx_set_stream(h, C.c_void_p(s.cuda_stream)) == 0
        y3 = prefilled(n, vt)
        torch.cuda.synchronize()
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = lib.sbmv_csr_spmv(h, capi.SBX_I32, capi.V_F32 if vt == "f32" else capi.V_F64, n, m, len(col), p(drp), p(dcol),
                               p(dval), p(dx), p(y3))
        assert rc == 0, lib.sbx_last_error(h).decode()
        s.synchronize()
    finally:
        lib.sbx_sync(h)
        lib.sbx_destroy(h)
    assert same_bits(y2, y1) and same_bits(y3, y1)


@functools.lru_cache(None)
def _power_law_uniform(vt):
    n, m, rp, col = shape("power_law")
    g = np.random.default_rng(73)
    return g.uniform(-1, 1, len(col)).astype(VTS[vt]), g.uniform(-1, 1, m).astype(VTS[vt]), None


# ---- 4
@pytest.mark.parametrize("tup,vt,name", [c for c in CASES if c[2] in ("staircase", "hub_middle", "dups", "power_law")],
                         ids=["-".join(c) for c in CASES if c[2] in ("staircase", "hub_middle", "dups", "power_law")])
def test_pattern(ops, tup, vt, name):
    n, m, rp, col = shape(name)
    ot, idt = TUPLES[tup]
    _, x = small_ints(name, vt)
    drp, dcol, dx = dev(rp, ot), dev(col, idt), dev(x)
    got = ops.csr_spmv(drp, dcol, dx, out=prefilled(n, vt))
    ones = ops.csr_spmv(drp, dcol, dx, val=torch.ones(len(col), dtype=dx.dtype, device="cuda"), out=prefilled(n, vt))
    want = exact_want(name, vt, pattern=True)
    assert same_bits(got, want), first_difference(got, want)
    assert same_bits(ones, want), first_difference(ones, want)


# ---- 5
@pytest.mark.parametrize("tup", list(TUPLES))
@pytest.mark.parametrize("vt", list(VTS))
def test_column_guard(ops, tup, vt):
    n, m, rp, col = shape("power_law")
    ot, idt = TUPLES[tup]
    val, x = small_ints("power_law", vt)
    g = np.random.default_rng(74)
    col = col.copy()
    pick = g.choice(len(col), 3000, replace=False)
    col[pick] = np.array([m, m + 1, -1])[g.integers(0, 3, len(pick))]
    col[[0, len(col) - 1]] = m, -1
    want = mv.spmv_int(rp, col, x, val, m) if vt in ("i32", "i64") else mv.spmv_wide(rp, col, x, val, m)[0].astype(VTS[vt])
    # x begins 16 elements inside a larger tensor and ends 16 before its end: an unguarded column reads 1000, not a fault
    big = torch.full((m + 32,), 1000, dtype=dev(x).dtype, device="cuda")
    big[16:16 + m] = dev(x)
    got = ops.csr_spmv(dev(rp, ot), dev(col, idt), big[16:16 + m], val=dev(val), m=m, out=prefilled(n, vt))
    assert same_bits(got, want), first_difference(got, want)


# ---- 6
def _refused(ops, rp, col, m, tup):
    from sparsebase_amd import capi
    ot, idt = TUPLES[tup]
    with pytest.raises(capi.SbxError) as e:
        ops.csr_check(dev(rp, ot), dev(col, idt), m)
    assert e.value.status == 1
    return str(e.value)


@pytest.mark.parametrize("tup", list(TUPLES))
def test_check_refuses(ops, tup):
    n, m, rp, col = shape("staircase")
    bad = rp.copy()
    bad[0] = 1
    assert "row_ptr[0] is 1" in _refused(ops, bad, col, m, tup)
    bad = rp.copy()
    bad[700] = bad[701] + 1  # rows 699 / 700: row_ptr[700] > row_ptr[701] is the first decreasing pair
    assert "decreases at row 700 " in _refused(ops, bad, col, m, tup)
    bad = rp.copy()
    bad[n] += 5
    assert f"row_ptr[{n}] is {rp[n] + 5}, not nnz = {rp[n]}" in _refused(ops, bad, col, m, tup)
    for value in (-1, m):
        bad = col.copy()
        bad[[123456, 400000]] = value
        assert f"position 123456 lies outside [0, {m})" in _refused(ops, rp, bad, m, tup)
    ot, idt = TUPLES[tup]
    ops.csr_check(dev(np.zeros(1, np.int64), ot), dev(np.zeros(0, np.int64), idt), 5)  # n = 0


# ---- 7
def test_with_rcm_and_permute(ops):
    n, m, rp, col = shape("power_law")
    val, x = small_ints("power_law", "f32")
    drp, dcol, dval, dx = dev(rp, np.int32), dev(col, np.int32), dev(val), dev(x)
    y = ops.csr_spmv(drp, dcol, dx, val=dval)
    assert same_bits(y, exact_want("power_law", "f32"))
    order = ops.rcm_reorder(drp, dcol, symmetrize=True)
    brp, bcol, bval = ops.permute_csr(n, n, drp, dcol, dval, order, order)
    xp = torch.empty_like(dx)
    xp[order.long()] = dx
    yp = ops.csr_spmv(brp, bcol, xp, val=bval)
    assert torch.equal(yp[order.long()], y)
