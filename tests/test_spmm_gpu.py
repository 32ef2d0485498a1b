"""GPU tests of include/sbmm.h through ops.csr_spmm, for every value type and every index tuple, against
tests/spmm_restate.py.  The shapes are those of tests/test_spmv_gpu.py, imported.

  1. exact cases       values and X are integers in [-8, 8]: every partial sum of a row is exact in float32 (70 000 * 64
                       < 2^23), so Y equals the restatement bit for bit whatever the order of the sum; Y is pre-filled
                       with NaN or -1, so an element that was not written shows
  2. leading dimensions and alignment   X and Y are column slices [:, 3:3 + k] of wider tensors (ldx = k + 5,
                       ldy = k + 7, an odd element offset): Y's slice is exact, every sentinel outside it untouched
  2b. aligned leading dimensions   the 16-byte aligned slices [:, 0:k] of tensors of 2 k columns: the 16-byte forms at
                       ldx, ldy != k, the padding untouched
  3. the rounding bound  |Y - Yhat| <= gamma(len, u) S + gamma(len, u_wide) S elementwise, for len rounded products summed
                       in any order (with or without fused multiply-add): nothing here is a measured tolerance
  4. determinism       two calls and a second handle on another stream: identical bytes; one vector replicated into all
                       k columns of X: all k columns of Y bitwise equal (a tail path that sums in another order shows)
  5. pattern           val=None equals val=ones, bitwise
  6. column guard      columns m, m + 1 and -1 contribute nothing; X is a slice of exactly m rows between rows of NaN
  7. refusals          every case of the header, with its status and the argument's name in the message
  8. with RCM          spmm(P A P^T, P X)[order[i], :] == spmm(A, X)[i, :]

The kernel's constants (sbx_spmm.hip) and the k that stands on either side of each:
  - MM_SPAN = 2048 entries per wave: the tile of the SpMV, so the staircase's 2047 ... 8193 rows cover it.
  - 64 lanes per wave, one column per lane where the 16-byte form does not apply (every odd k, and every k of section
    2): one group of lanes up to k = 64, two blocks of columns from k = 65 (64 | 65), three from 129 (128 | 129), five
    from 257 (256 | 257); the groups-of-lanes form below 33 lanes and the one-group form from 33 (32 | 33).
  - 16 bytes per lane (4 columns of f32 / i32, 2 of f64 / i64) where X, Y, ldx, ldy and k allow it (every k % 4 == 0
    here in section 1): 32 lanes at k = 128, 33 at 132 (128 | 132: groups-of-lanes | one group); 64 lanes at k = 256,
    two blocks of columns from 260 (256 | 260); 12 and 20 give 3 and 5 lanes per group, groups that do not divide the
    wave (lanes left over, a span that does not divide into the groups' runs).  For the 8-byte types (2 columns per
    lane) those boundaries are 64 | 66 (32 | 33 lanes) and 128 | 130 (64 lanes | two blocks of columns).  The other index
    tuples and value types run K_OTHER, the issue's list (of which 8 and 64 are groups-of-lanes forms at 16 bytes and the
    odd k one column per lane), plus K_EDGE = 66, 130, 132, 260, all aligned: the far side of every one of these four
    boundaries, so that the one-group form at 16 bytes per lane and its second block of columns run for every index
    tuple and every value type; sections 2b and 4 run them too.
  - k = 1 at unit strides goes to the SpMV's kernels; k = 1 of section 2 does not.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmm_restate as mm  # noqa: E402
import spmv_restate as mv  # noqa: E402
from test_spmv_gpu import (BOUND_SHAPES, SHAPES, TUPLES, VTS, _wide_for, dev, first_difference, ops, same_bits,  # noqa: E402,F401
                           shape)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K_BASE = [1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513]
K_ALL = sorted(set(K_BASE + [12, 20, 132, 260]))
K_OTHER = [1, 3, 8, 33, 64, 129]
K_EDGE = [66, 130, 132, 260]  # the far sides of 64 | 66, 128 | 130 (8-byte values) and 128 | 132, 256 | 260 (4-byte values)
K_MAX = max(K_ALL)
TORCH_DT = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "i64": torch.int64}


@functools.lru_cache(None)
def small_ints(name):
    """(val, X): integers in [-8, 8]; X has K_MAX columns, a test takes the first k."""
    n, m, rp, col = shape(name)
    g = np.random.default_rng(172)
    return g.integers(-8, 9, len(col)), g.integers(-8, 9, (m, K_MAX))


@functools.lru_cache(None)
def exact_ref(name, pattern=False):
    """The restatement's n x K_MAX product in int64, computed once: its first k columns are the product with X[:, :k]."""
    n, m, rp, col = shape(name)
    val, X = small_ints(name)
    ref = mm.spmm_int(rp, col, X.reshape(-1), K_MAX, None if pattern else val, m=m)
    assert np.abs(ref).max(initial=0) < 2 ** 23  # exact in float32 in any order
    return ref


def operands(name, vt, k):
    val, X = small_ints(name)
    return val.astype(VTS[vt]), np.ascontiguousarray(X[:, :k]).astype(VTS[vt])


def prefilled(n, k, vt, width=None):
    return torch.full((n, k if width is None else width), float("nan") if vt in ("f32", "f64") else -1, dtype=TORCH_DT[vt],
                      device="cuda")


def differs(got, want):
    got = got.cpu().numpy()
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{got.dtype}{got.shape} for {want.dtype}{want.shape}"
    bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
    return f"{len(bad)} of {want.size} elements differ, first (row, column) {bad[:5].tolist()}: " \
           f"{[got[tuple(b)] for b in bad[:5]]} for {[want[tuple(b)] for b in bad[:5]]}"


# ---- 1
EXACT = [("i32", "f32", s, k) for s in SHAPES for k in K_ALL] + \
        [(t, v, s, k) for t in TUPLES for v in VTS if (t, v) != ("i32", "f32")
         for s in ("staircase", "hub_middle", "power_law") for k in K_OTHER + K_EDGE]


@pytest.mark.parametrize("tup,vt,name,k", EXACT, ids=[f"{t}-{v}-{s}-k{k}" for t, v, s, k in EXACT])
def test_exact(ops, tup, vt, name, k):
    n, m, rp, col = shape(name)
    ot, idt = TUPLES[tup]
    val, X = operands(name, vt, k)
    want = np.ascontiguousarray(exact_ref(name)[:, :k]).astype(VTS[vt])
    y = prefilled(n, k, vt)
    got = ops.csr_spmm(dev(rp, ot), dev(col, idt), dev(X), val=dev(val), m=m, out=y)
    assert got is y
    assert same_bits(y, want), differs(y, want)  # (NaN or -1 left: an element that was not written)


# ---- 2
@pytest.mark.parametrize("k", [1, 4, 7, 64, 68, 130])
@pytest.mark.parametrize("vt", ["f32", "i64"])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "nnz0"])
def test_leading_dimensions_and_alignment(ops, name, vt, k):
    n, m, rp, col = shape(name)
    val, X = operands(name, vt, k)
    want = np.ascontiguousarray(exact_ref(name)[:, :k]).astype(VTS[vt])
    xw = prefilled(m, k, vt, k + 5)
    xw[:, 3:3 + k] = dev(X)
    yw = prefilled(n, k, vt, k + 7)
    sentinel = yw.clone()
    xs, ys = xw[:, 3:3 + k], yw[:, 3:3 + k]
    assert xs.stride(0) == k + 5 and ys.stride(0) == k + 7 and xs.data_ptr() % 16 != 0 and ys.data_ptr() % 16 != 0
    got = ops.csr_spmm(dev(rp, np.int32), dev(col, np.int32), xs, val=dev(val), m=m, out=ys)
    assert got is ys
    assert same_bits(ys.contiguous(), want), differs(ys.contiguous(), want)
    outside = torch.ones_like(yw, dtype=torch.bool)
    outside[:, 3:3 + k] = False
    assert same_bits(yw[outside], sentinel[outside].cpu().numpy()), "the padding of Y was written"


# ---- 2b
@pytest.mark.parametrize("k", [8, 64, 66, 132])
@pytest.mark.parametrize("tup,vt", [("i32", "f32"), ("i64", "f64"), ("i32_n64", "i64")])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "nnz0"])
def test_aligned_leading_dimensions(ops, name, tup, vt, k):
    """X and Y are the 16-byte aligned slices [:, 0:k] of tensors of 2 k columns: the 16-bytes-per-lane forms (groups of
    lanes at k = 8 and 64, one group at k = 132, and at 66 for the 8-byte types) at leading dimensions other than k."""
    n, m, rp, col = shape(name)
    ot, idt = TUPLES[tup]
    val, X = operands(name, vt, k)
    want = np.ascontiguousarray(exact_ref(name)[:, :k]).astype(VTS[vt])
    xw = prefilled(m, k, vt, 2 * k)
    xw[:, :k] = dev(X)
    yw = prefilled(n, k, vt, 2 * k)
    sentinel = yw.clone()
    xs, ys = xw[:, :k], yw[:, :k]
    assert xs.data_ptr() % 16 == 0 and ys.data_ptr() % 16 == 0 and (2 * k * xs.element_size()) % 16 == 0
    assert (xs.stride(0) == 2 * k or m <= 1) and (ys.stride(0) == 2 * k or n <= 1)
    got = ops.csr_spmm(dev(rp, ot), dev(col, idt), xs, val=dev(val), m=m, out=ys)
    assert got is ys
    assert same_bits(ys.contiguous(), want), differs(ys.contiguous(), want)
    assert same_bits(yw[:, k:].contiguous(), sentinel[:, k:].cpu().numpy()), "the padding of Y was written"


# ---- 3
K_BOUND = (3, 64, 129)


@functools.lru_cache(None)
def uniform_data(name, vt):
    """(val, X of max(K_BOUND) columns, the wide product or None): uniform in (-1, 1), kept 2^-20 away from 0."""
    n, m, rp, col = shape(name)
    g = np.random.default_rng(173)

    def draw(size):
        u = g.uniform(-1.0, 1.0, size)
        return np.where(np.abs(u) < 2.0 ** -20, 2.0 ** -20, u).astype(VTS[vt])
    val, X = draw(len(col)), draw((m, max(K_BOUND)))
    wide = _wide_for(vt, len(col))
    return val, X, (None if wide is None else mm.spmm_wide(rp, col, X.reshape(-1), max(K_BOUND), val, m=m, wide=wide))


@pytest.mark.parametrize("k", K_BOUND)
@pytest.mark.parametrize("name", BOUND_SHAPES)
@pytest.mark.parametrize("vt", ["f32", "f64"])
def test_rounding_bound(ops, vt, name, k):
    n, m, rp, col = shape(name)
    u = 2.0 ** -24 if vt == "f32" else 2.0 ** -53
    length = np.diff(rp)[:, None]
    val, X, wide = uniform_data(name, vt)
    if wide is None:  # (f64 on a platform without a wider format: only the shapes of at most 2000 entries)
        return
    yhat, S, u_wide = (wide[0][:, :k], wide[1][:, :k], wide[2])
    y = ops.csr_spmm(dev(rp, np.int32), dev(col, np.int32), dev(np.ascontiguousarray(X[:, :k])), val=dev(val), m=m,
                     out=prefilled(n, k, vt)).cpu().numpy().astype(np.longdouble)
    bound = (mv.gamma(length, u) + mv.gamma(length, u_wide)) * S.astype(np.longdouble)
    err = np.abs(y - yhat.astype(np.longdouble))
    worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
    print(f"{name} {vt} k={k}: largest error / bound = {float(np.max(err[bound > 0] / bound[bound > 0])):.3g}")
    assert (err <= bound).all(), f"element {worst} of a row of {length[worst[0], 0]} entries: error {err[worst]} over the bound {bound[worst]}"


# ---- 4
@functools.lru_cache(None)
def _uniform(name, vt, k):
    n, m, rp, col = shape(name)
    g = np.random.default_rng(174)
    return g.uniform(-1, 1, len(col)).astype(VTS[vt]), g.uniform(-1, 1, (m, k)).astype(VTS[vt])


@pytest.mark.parametrize("k", [8, 129, 130])
@pytest.mark.parametrize("name", ["hub_middle", "power_law"])
@pytest.mark.parametrize("vt", ["f32", "f64"])
def test_determinism(ops, vt, name, k):
    from sparsebase_amd import capi
    n, m, rp, col = shape(name)
    val, X = _uniform(name, vt, k)
    drp, dcol, dval, dx = dev(rp, np.int32), dev(col, np.int32), dev(val), dev(X)
    y1 = ops.csr_spmm(drp, dcol, dx, val=dval).cpu().numpy()
    y2 = ops.csr_spmm(drp, dcol, dx, val=dval).cpu().numpy()
    torch.cuda.synchronize()
    lib, h, s = capi.load(), C.c_void_p(), torch.cuda.Stream()
    assert lib.sbx_create(torch.cuda.current_device(), C.byref(h)) == 0
    try:
        assert lib.sbx_set_stream(h, C.c_void_p(s.cuda_stream)) == 0
        y3 = prefilled(n, k, vt)
        torch.cuda.synchronize()
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = lib.sbmm_csr_spmm(h, capi.SBX_I32, capi.V_F32 if vt == "f32" else capi.V_F64, n, m, len(col), k, p(drp), p(dcol),
                               p(dval), p(dx), k, p(y3), k)
        assert rc == 0, lib.sbx_last_error(h).decode()
        s.synchronize()
    finally:
        lib.sbx_sync(h)
        lib.sbx_destroy(h)
    assert not np.isnan(y1).any()
    assert same_bits(y2, y1) and same_bits(y3, y1)


@pytest.mark.parametrize("k", [5, 64, 66, 132, 257, 260])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "power_law"])
@pytest.mark.parametrize("vt", ["f32", "f64"])
def test_columns_agree(ops, vt, name, k):
    n, m, rp, col = shape(name)
    val, X = _uniform(name, vt, 1)
    X = np.ascontiguousarray(np.repeat(X, k, axis=1))
    y = ops.csr_spmm(dev(rp, np.int32), dev(col, np.int32), dev(X), val=dev(val), m=m, out=prefilled(n, k, vt)).cpu().numpy()
    assert not np.isnan(y).any()
    width = y.itemsize
    cols = np.ascontiguousarray(y.T).view(np.uint8).reshape(k, n * width)
    odd = [j for j in range(1, k) if not np.array_equal(cols[j], cols[0])]
    assert not odd, f"columns {odd[:8]} of Y differ from column 0 for equal columns of X"


# ---- 5
@pytest.mark.parametrize("k", [3, 64, 129])
@pytest.mark.parametrize("tup,vt", [("i32", "f32"), ("i64", "f64"), ("i32_n64", "i32"), ("i32", "i64")])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "dups", "power_law"])
def test_pattern(ops, name, tup, vt, k):
    n, m, rp, col = shape(name)
    ot, idt = TUPLES[tup]
    _, X = operands(name, vt, k)
    drp, dcol, dx = dev(rp, ot), dev(col, idt), dev(X)
    got = ops.csr_spmm(drp, dcol, dx, out=prefilled(n, k, vt))
    ones = ops.csr_spmm(drp, dcol, dx, val=torch.ones(len(col), dtype=dx.dtype, device="cuda"), out=prefilled(n, k, vt))
    want = np.ascontiguousarray(exact_ref(name, pattern=True)[:, :k]).astype(VTS[vt])
    assert same_bits(got, want), differs(got, want)
    assert same_bits(ones, want), differs(ones, want)


# ---- 6
@pytest.mark.parametrize("k", [3, 64])
@pytest.mark.parametrize("tup", list(TUPLES))
@pytest.mark.parametrize("vt", list(VTS))
def test_column_guard(ops, vt, tup, k):
    n, m, rp, col = shape("power_law")
    ot, idt = TUPLES[tup]
    val, X = operands("power_law", vt, k)
    g = np.random.default_rng(175)
    col = col.copy()
    pick = g.choice(len(col), 3000, replace=False)
    col[pick] = np.array([m, m + 1, -1])[g.integers(0, 3, len(pick))]
    col[[0, len(col) - 1]] = m, -1
    want = mm.spmm_int(rp, col, X.astype(np.int64).reshape(-1), k, val.astype(np.int64), m=m).astype(VTS[vt])
    # X begins 16 rows inside a larger tensor and ends 16 before its end: an unguarded column reads NaN (1000), not a fault
    big = torch.full((m + 32, k), float("nan") if vt in ("f32", "f64") else 1000, dtype=TORCH_DT[vt], device="cuda")
    big[16:16 + m] = dev(X)
    got = ops.csr_spmm(dev(rp, ot), dev(col, idt), big[16:16 + m], val=dev(val), m=m, out=prefilled(n, k, vt))
    assert same_bits(got, want), differs(got, want)


# ---- 7
def test_refusals(ops):
    from sparsebase_amd import capi
    hd = ops.handle_for(torch.device("cuda", torch.cuda.current_device()))
    lib = hd.lib
    n, m, k = 4, 3, 2
    rp, col = dev(np.array([0, 1, 2, 2, 3], np.int32)), dev(np.array([0, 2, 1], np.int32))
    val = torch.ones(3, dtype=torch.float32, device="cuda")
    X = torch.ones((m, k), dtype=torch.float32, device="cuda")
    Y = prefilled(n, k, "f32")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ok = dict(it=capi.SBX_I32, vt=capi.V_F32, n=n, m=m, nnz=3, k=k, rp=rp, col=col, val=val, x=X, ldx=k, y=Y, ldy=k)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.sbmm_csr_spmm(hd.h, a["it"], a["vt"], a["n"], a["m"], a["nnz"], a["k"], p(a["rp"]), p(a["col"]), p(a["val"]),
                               p(a["x"]), a["ldx"], p(a["y"]), a["ldy"])
        return rc, lib.sbx_last_error(hd.h).decode()

    BAD, UNSUPPORTED = 1, 5
    for kw, status, word in [
            (dict(n=-1), BAD, "n is negative"), (dict(m=-1), BAD, "m is negative"), (dict(nnz=-1), BAD, "nnz is negative"),
            (dict(k=-1), BAD, "k is negative"), (dict(ldx=k - 1), BAD, "ldx"), (dict(ldy=k - 1), BAD, "ldy"),
            (dict(n=0), BAD, "nnz > 0 with n == 0"), (dict(rp=None), BAD, "row_ptr"), (dict(col=None), BAD, "col"),
            (dict(x=None), BAD, "x is NULL"), (dict(y=None), BAD, "y is NULL"), (dict(vt=capi.V_NONE), BAD, "value type"),
            (dict(vt=77), BAD, "value type"), (dict(it=9), BAD, "index type"),
            (dict(nnz=1 << 42), UNSUPPORTED, "nnz")]:
        rc, msg = call(**kw)
        assert rc == status and "sbmm_csr_spmm" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(Y).all(), "a refused call wrote to Y"
    # k > 2^20 on a 1 x 1 matrix with buffers of the full legal size: nothing could fault even without the refusal
    kk = (1 << 20) + 1
    bx, by = torch.ones((1, kk), dtype=torch.float32, device="cuda"), prefilled(1, kk, "f32")
    rc, msg = call(n=1, m=1, nnz=1, k=kk, rp=dev(np.array([0, 1], np.int32)), col=dev(np.array([0], np.int32)),
                   val=val[:1], x=bx, ldx=kk, y=by, ldy=kk)
    assert rc == UNSUPPORTED and "sbmm_csr_spmm" in msg and "k = " in msg, (rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(by).all()
    # k == 0 and n == 0 succeed and write nothing
    assert call(k=0, ldx=0, ldy=0)[0] == 0 and call(k=0)[0] == 0
    assert call(n=0, nnz=0, rp=dev(np.zeros(1, np.int32)))[0] == 0
    torch.cuda.synchronize()
    assert torch.isnan(Y).all()
    rc, msg = call()
    torch.cuda.synchronize()
    assert rc == 0 and Y.cpu().tolist() == [[1, 1], [1, 1], [0, 0], [1, 1]]


def test_the_tensor_layer_refuses(ops):
    rp, col = dev(np.array([0, 1], np.int32)), dev(np.array([0], np.int32))
    X = torch.ones((1, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        ops.csr_spmm(rp, col, X.cpu())
    with pytest.raises(ValueError):
        ops.csr_spmm(rp, col, torch.ones((4, 2), dtype=torch.float32, device="cuda").t()[:1])  # stride(1) != 1
    with pytest.raises(ValueError):
        ops.csr_spmm(rp, col, X, out=torch.ones((4, 2), dtype=torch.float32, device="cuda").t()[:1])
    with pytest.raises(ValueError):
        ops.csr_spmm(rp, col, X[0])  # 1-D


# ---- 8
def test_with_rcm_and_permute(ops):
    n, m, rp, col = shape("power_law")
    k = 16
    val, X = operands("power_law", "f32", k)
    drp, dcol, dval, dx = dev(rp, np.int32), dev(col, np.int32), dev(val), dev(X)
    y = ops.csr_spmm(drp, dcol, dx, val=dval)
    want = np.ascontiguousarray(exact_ref("power_law")[:, :k]).astype(np.float32)
    assert same_bits(y, want), differs(y, want)
    order = ops.rcm_reorder(drp, dcol, symmetrize=True)
    brp, bcol, bval = ops.permute_csr(n, n, drp, dcol, dval, order, order)
    xp = torch.empty_like(dx)
    xp[order.long()] = dx
    yp = ops.csr_spmm(brp, bcol, xp, val=bval)
    assert torch.equal(yp[order.long()], y)
