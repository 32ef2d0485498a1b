"""GPU tests of include/sbdd.h through ops.csr_sddmm, for every value type and every index tuple, against
tests/sddmm_restate.py.  The shapes are those of tests/test_spmv_gpu.py, imported: rows on either side of the 2048-entry
span, hub_* (one row over 35 spans), ones, tall, dups, n0, nnz0, one.

  1. exact cases       val, U, V are integers in [-8, 8]: |val| k 64 <= 8 * 513 * 64 < 2^23, so every partial sum is exact
                       in float32 in any order and out equals the restatement bit for bit; the final product is done in
                       the value type, so -0 agrees; out is pre-filled with NaN or -1, so an unwritten element shows
  2. leading dimensions and alignment   U and V are odd column slices [:, 3:3 + k] of wider tensors (the one-column
                       form), and the 16-byte aligned slices [:, 0:k] of tensors of 2 k columns (the 16-byte form)
  3. the rounding bound  |out - outhat| <= gamma(k + 1, u) S + gamma(k + 1, u_wide) S elementwise: k rounded products
                       summed in any order, with or without fused multiply-add, then one product; derived, not measured
  4. determinism and position independence   two calls and a second handle on another stream: identical bytes; on `dups`
                       entries with equal (row, column, value) have equal bits; one (row, column, value) first in a hub
                       row of one matrix and alone in its row in another, at another position: equal bits
  5. pattern           val=None equals val=ones, bitwise
  6. column guard      columns m, m + 1 and -1 give +0; V is a slice of exactly m rows between rows of NaN, U of n rows
  7. k == 0            +0 into a NaN-filled out; nnz0 and n0 write nothing
  8. refusals          every case of the header, with its status and the argument's name in the message; the ValueErrors
                       of the tensor layer
  9. with RCM and permute   sddmm(P A P^T; P U, P V) at a permuted entry equals sddmm(A; U, V) at its origin, bitwise, on
                       random floats: ops.permute_csr carries arange(nnz) as the value payload
 10. with SpMM         out.sum() of sddmm(A; W, X) equals (W * csr_spmm(A, X)).sum(), exactly, on small integers

The kernel's constants (sbx_sddmm.hip) and the k that stands on either side of each:
  - DD_SPAN = 2048 entries per wave in batches of 512 (8 per lane): the staircase's 2047 ... 8193 rows and the hubs
    cover span and batch ends; `one`, `dups` and the staircase's short rows a last batch that is not full.
  - one column per lane (every odd k, and every k of section 2's odd slices): a group of G = 1, 2, 4, 8, 16, 32 lanes per
    entry up to k = 1, 2, 4, 8, 16, 32 (1 | 2, 2 | 3, 4 | 5, 8 | 9, 16 | 17, 32 | 33), the groups that are padded with
    zeros at 3, 5, 9, 15, 17, 31; the wide form (one group of 64, entries broadcast through scalar registers) from 33;
    two blocks of columns from 65 (64 | 65), three from 129 (128 | 129), five from 257 (256 | 257), nine at 513.
  - 16 bytes per lane (4 columns of f32 / i32, 2 of f64 / i64) where U, V, ldu, ldv and k allow it (every k % 4 == 0 of
    section 1): G = 1 at k = 4 (no exchange at all), 2 at 8, 4 at 12 (padded) and 16, 8 at 20 (padded) and 32, 16 at 36
    (32 | 36) and 64, 32 at 68 (64 | 68) and 128, the wide form at 132 (128 | 132) and 256, two blocks from 260
    (256 | 260).  For the 8-byte types those boundaries are 64 | 66 (32 | 33 lanes) and 128 | 130 (64 lanes | two blocks).
    K_SDDMM = 9, 36, 68 are this kernel's own boundaries beside the k lists of tests/test_spmm_gpu.py.  The other index
    tuples and value types run K_OTHER plus K_EDGE = 66, 130, 132, 260, as there.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sddmm_restate as dd  # noqa: E402
import spmv_restate as mv  # noqa: E402
from test_spmv_gpu import (BOUND_SHAPES, SHAPES, TUPLES, VTS, _wide_for, dev, ops, same_bits, shape)  # noqa: E402,F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K_BASE = [1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513]
K_SDDMM = [9, 36, 68]
K_ALL = sorted(set(K_BASE + [12, 20, 132, 260] + K_SDDMM))
K_OTHER = [1, 3, 8, 33, 64, 129]
K_EDGE = [66, 130, 132, 260]
K_MAX = max(K_ALL)
TORCH_DT = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "i64": torch.int64}
FLOATS = ("f32", "f64")


@functools.lru_cache(None)
def small_ints(name):
    """(val, U, V): integers in [-8, 8]; U and V have K_MAX columns, a test takes the first k."""
    n, m, rp, col = shape(name)
    g = np.random.default_rng(181)
    return (g.integers(-8, 9, len(col)), g.integers(-8, 9, (n, K_MAX)).astype(np.int32),
            g.integers(-8, 9, (m, K_MAX)).astype(np.int32))


@functools.lru_cache(None)
def exact_dots(name):
    """{k: the nnz dots in int64} for every k of the lists, from one pass of the restatement."""
    n, m, rp, col = shape(name)
    _, U, V = small_ints(name)
    dots = dd.int_prefix(rp, col, U.astype(np.int64), V.astype(np.int64), sorted(set(K_ALL + K_OTHER + K_EDGE + [7, 130])), m=m)
    assert all(np.abs(d).max(initial=0) * 8 < 2 ** 23 for d in dots.values())  # exact in float32 in any order
    return dots


def exact_want(name, vt, k, pattern=False, val=None):
    """The restatement's out in the value type: the dot, then the one product val * dot done in that type (-0 agrees)."""
    dot = exact_dots(name)[k].astype(VTS[vt])
    if pattern:
        return dot
    w = (small_ints(name)[0] if val is None else val).astype(VTS[vt])
    return (w * dot).astype(VTS[vt])


def operands(name, vt, k):
    val, U, V = small_ints(name)
    return val.astype(VTS[vt]), np.ascontiguousarray(U[:, :k]).astype(VTS[vt]), np.ascontiguousarray(V[:, :k]).astype(VTS[vt])


def filled(shape_, vt):
    return torch.full(shape_, float("nan") if vt in FLOATS else -1, dtype=TORCH_DT[vt], device="cuda")


def differs(got, want):
    got = got.cpu().numpy()
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{got.dtype}{got.shape} for {want.dtype}{want.shape}"
    width = got.itemsize
    bad = np.nonzero((got.view(np.uint8).reshape(-1, width) != want.view(np.uint8).reshape(-1, width)).any(axis=1))[0]
    return f"{len(bad)} of {len(want)} entries differ, first {bad[:5]}: {got[bad[:5]]} for {want[bad[:5]]}"


# ---- 1
EXACT = [("i32", "f32", s, k) for s in SHAPES for k in K_ALL] + \
        [(t, v, s, k) for t in TUPLES for v in VTS if (t, v) != ("i32", "f32")
         for s in ("staircase", "hub_middle", "power_law") for k in K_OTHER + K_EDGE]


@pytest.mark.parametrize("tup,vt,name,k", EXACT, ids=[f"{t}-{v}-{s}-k{k}" for t, v, s, k in EXACT])
def test_exact(ops, tup, vt, name, k):
    n, m, rp, col = shape(name)
    ot, idt = TUPLES[tup]
    val, U, V = operands(name, vt, k)
    want = exact_want(name, vt, k)
    out = filled((len(col),), vt)
    got = ops.csr_sddmm(dev(rp, ot), dev(col, idt), dev(U), dev(V), val=dev(val), out=out)
    assert got is out
    assert same_bits(out, want), differs(out, want)  # (NaN or -1 left: an element that was not written)


# ---- 2
@pytest.mark.parametrize("k", [1, 4, 7, 64, 68, 130])
@pytest.mark.parametrize("vt", ["f32", "i64"])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "nnz0"])
def test_odd_slices_take_the_one_column_form(ops, name, vt, k):
    n, m, rp, col = shape(name)
    val, U, V = operands(name, vt, k)
    uw, vw = filled((n, k + 5), vt), filled((m, k + 7), vt)
    uw[:, 3:3 + k], vw[:, 3:3 + k] = dev(U), dev(V)
    us, vs = uw[:, 3:3 + k], vw[:, 3:3 + k]
    assert us.stride(0) == k + 5 and vs.stride(0) == k + 7 and us.data_ptr() % 16 != 0 and vs.data_ptr() % 16 != 0
    out = ops.csr_sddmm(dev(rp, np.int32), dev(col, np.int32), us, vs, val=dev(val), out=filled((len(col),), vt))
    want = exact_want(name, vt, k)
    assert same_bits(out, want), differs(out, want)


@pytest.mark.parametrize("k", [4, 8, 64, 66, 132, 260])
@pytest.mark.parametrize("tup,vt", [("i32", "f32"), ("i64", "f64"), ("i32_n64", "i64")])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "nnz0"])
def test_aligned_slices_take_the_16_byte_form(ops, name, tup, vt, k):
    n, m, rp, col = shape(name)
    ot, idt = TUPLES[tup]
    val, U, V = operands(name, vt, k)
    uw, vw = filled((n, 2 * k), vt), filled((m, 2 * k), vt)
    uw[:, :k], vw[:, :k] = dev(U), dev(V)
    us, vs = uw[:, :k], vw[:, :k]
    assert us.data_ptr() % 16 == 0 and vs.data_ptr() % 16 == 0 and (2 * k * us.element_size()) % 16 == 0
    assert (us.stride(0) == 2 * k or n <= 1) and (vs.stride(0) == 2 * k or m <= 1)
    out = ops.csr_sddmm(dev(rp, ot), dev(col, idt), us, vs, val=dev(val), out=filled((len(col),), vt))
    want = exact_want(name, vt, k)
    assert same_bits(out, want), differs(out, want)


# ---- 3
K_BOUND = (3, 64, 129, 132, 260)


@functools.lru_cache(None)
def uniform_data(name, vt):
    """(val, U, V of max(K_BOUND) columns, the wide prefix or None): uniform in (-1, 1), kept 2^-20 away from 0."""
    n, m, rp, col = shape(name)
    g = np.random.default_rng(182)

    def draw(size):
        u = g.uniform(-1.0, 1.0, size)
        return np.where(np.abs(u) < 2.0 ** -20, 2.0 ** -20, u).astype(VTS[vt])
    val, U, V = draw(len(col)), draw((n, max(K_BOUND))), draw((m, max(K_BOUND)))
    wide = _wide_for(vt, len(col))
    return val, U, V, (None if wide is None else dd.wide_prefix(rp, col, U, V, K_BOUND, m=m, wide=wide))


@pytest.mark.parametrize("k", K_BOUND)
@pytest.mark.parametrize("name", BOUND_SHAPES)
@pytest.mark.parametrize("vt", FLOATS)
def test_rounding_bound(ops, vt, name, k):
    n, m, rp, col = shape(name)
    u = 2.0 ** -24 if vt == "f32" else 2.0 ** -53
    val, U, V, wide = uniform_data(name, vt)
    if wide is None:  # (f64 on a platform without a wider format: only the shapes of at most 2000 entries)
        return
    (dot, tot), u_wide = wide[0][k], wide[1]
    w = val.astype(dot.dtype)
    outhat, S = (w * dot).astype(np.longdouble), (np.abs(w) * tot).astype(np.longdouble)
    out = ops.csr_sddmm(dev(rp, np.int32), dev(col, np.int32), dev(np.ascontiguousarray(U[:, :k])),
                        dev(np.ascontiguousarray(V[:, :k])), val=dev(val), out=filled((len(col),), vt))
    out = out.cpu().numpy().astype(np.longdouble)
    bound = (mv.gamma(k + 1, u) + mv.gamma(k + 1, u_wide)) * S
    err = np.abs(out - outhat)
    worst = int(np.argmax(err - bound))
    print(f"{name} {vt} k={k}: largest error / bound = {float(np.max(err[bound > 0] / bound[bound > 0])):.3g}")
    assert (err <= bound).all(), f"entry {worst}: error {err[worst]} over the bound {bound[worst]}"


# ---- 4
@functools.lru_cache(None)
def _uniform(name, vt, k):
    n, m, rp, col = shape(name)
    g = np.random.default_rng(183)
    return (g.uniform(-1, 1, len(col)).astype(VTS[vt]), g.uniform(-1, 1, (n, k)).astype(VTS[vt]),
            g.uniform(-1, 1, (m, k)).astype(VTS[vt]))


@pytest.mark.parametrize("k", [8, 129, 130])
@pytest.mark.parametrize("name", ["hub_middle", "power_law"])
@pytest.mark.parametrize("vt", FLOATS)
def test_determinism(ops, vt, name, k):
    from sparsebase_amd import capi
    n, m, rp, col = shape(name)
    val, U, V = _uniform(name, vt, k)
    drp, dcol, dval, du, dv = dev(rp, np.int32), dev(col, np.int32), dev(val), dev(U), dev(V)
    o1 = ops.csr_sddmm(drp, dcol, du, dv, val=dval).cpu().numpy()
    o2 = ops.csr_sddmm(drp, dcol, du, dv, val=dval).cpu().numpy()
    torch.cuda.synchronize()
    lib, h, s = capi.load(), C.c_void_p(), torch.cuda.Stream()
    assert lib.sbx_create(torch.cuda.current_device(), C.byref(h)) == 0
    try:
        assert lib.sbx_set_stream(h, C.c_void_p(s.cuda_stream)) == 0
        o3 = filled((len(col),), vt)
        torch.cuda.synchronize()
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = lib.sbdd_csr_sddmm(h, capi.SBX_I32, capi.V_F32 if vt == "f32" else capi.V_F64, n, m, len(col), k, p(drp), p(dcol),
                                p(dval), p(du), k, p(dv), k, p(o3))
        assert rc == 0, lib.sbx_last_error(h).decode()
        s.synchronize()
    finally:
        lib.sbx_sync(h)
        lib.sbx_destroy(h)
    assert not np.isnan(o1).any()
    assert same_bits(o2, o1) and same_bits(o3, o1)


@pytest.mark.parametrize("k", [3, 8, 64, 65, 132, 260])
@pytest.mark.parametrize("tup,vt", [("i32", "f32"), ("i64", "f64")])
def test_equal_entries_get_equal_bits(ops, tup, vt, k):
    """`dups` has 7 columns and rows of up to 39 entries: most (row, column) pairs occur several times.  With a value
    that depends on (row, column) alone, every occurrence has the same bits."""
    n, m, rp, col = shape("dups")
    ot, idt = TUPLES[tup]
    _, U, V = _uniform("dups", vt, k)
    rows = dd.rows_of(rp, len(col))
    val = np.random.default_rng(184).uniform(-1, 1, (n, m)).astype(VTS[vt])[rows, col]
    out = ops.csr_sddmm(dev(rp, ot), dev(col, idt), dev(U), dev(V), val=dev(val), out=filled((len(col),), vt)).cpu().numpy()
    assert not np.isnan(out).any()
    bits = out.view(np.uint32 if vt == "f32" else np.uint64)
    key = rows * m + col
    order = np.argsort(key, kind="stable")
    same_key = key[order][1:] == key[order][:-1]
    assert same_key.sum() > 1000
    assert (bits[order][1:][same_key] == bits[order][:-1][same_key]).all()


@pytest.mark.parametrize("k", [3, 8, 64, 65, 132, 260])
@pytest.mark.parametrize("vt", FLOATS)
def test_an_entry_does_not_depend_on_where_it_lies(ops, vt, k):
    """The triple (row 40, column 17, value w) is the first entry of a hub row of 5000 entries in one matrix, at position
    97; in the other it is alone in its row, at position 4321 (another batch, another lane, another span)."""
    n, m, row, c, w = 100, 300, 40, 17, -0.6180339887
    g = np.random.default_rng(185)
    U, V = g.uniform(-1, 1, (n, k)).astype(VTS[vt]), g.uniform(-1, 1, (m, k)).astype(VTS[vt])

    def matrix(before, length):
        lengths = np.zeros(n, np.int64)
        lengths[:row] = np.diff(np.linspace(0, before, row + 1).astype(np.int64))
        lengths[row] = length
        lengths[row + 1:] = 3
        rp = np.concatenate([[0], np.cumsum(lengths)])
        col = g.integers(0, m, rp[-1])
        val = g.uniform(-1, 1, rp[-1])
        col[before], val[before] = c, w
        return rp, col, val.astype(VTS[vt])
    got = []
    for before, length in ((97, 5000), (4321, 1)):
        rp, col, val = matrix(before, length)
        assert rp[row] == before and rp[row + 1] - rp[row] == length
        out = ops.csr_sddmm(dev(rp, np.int32), dev(col, np.int32), dev(U), dev(V), val=dev(val),
                            out=filled((len(col),), vt)).cpu().numpy()
        assert not np.isnan(out).any()
        got.append(out[before:before + 1])
    assert got[0].tobytes() == got[1].tobytes(), (got[0], got[1])


# ---- 5
@pytest.mark.parametrize("k", [3, 64, 129])
@pytest.mark.parametrize("tup,vt", [("i32", "f32"), ("i64", "f64"), ("i32_n64", "i32"), ("i32", "i64")])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "dups", "power_law"])
def test_pattern(ops, name, tup, vt, k):
    n, m, rp, col = shape(name)
    ot, idt = TUPLES[tup]
    _, U, V = operands(name, vt, k)
    drp, dcol, du, dv = dev(rp, ot), dev(col, idt), dev(U), dev(V)
    got = ops.csr_sddmm(drp, dcol, du, dv, out=filled((len(col),), vt))
    ones = ops.csr_sddmm(drp, dcol, du, dv, val=torch.ones(len(col), dtype=du.dtype, device="cuda"), out=filled((len(col),), vt))
    want = exact_want(name, vt, k, pattern=True)
    assert same_bits(got, want), differs(got, want)
    assert same_bits(ones, want), differs(ones, want)


# ---- 6
@pytest.mark.parametrize("k", [3, 64, 132])
@pytest.mark.parametrize("tup", list(TUPLES))
@pytest.mark.parametrize("vt", list(VTS))
def test_column_guard(ops, vt, tup, k):
    n, m, rp, col = shape("power_law")
    ot, idt = TUPLES[tup]
    val, U, V = operands("power_law", vt, k)
    g = np.random.default_rng(186)
    col = col.copy()
    pick = g.choice(len(col), 3000, replace=False)
    col[pick] = np.array([m, m + 1, -1])[g.integers(0, 3, len(pick))]
    col[[0, len(col) - 1]] = m, -1
    if vt in FLOATS:
        want = dd.sddmm_wide(rp, col, U, V, k, val, m=m, wide=VTS[vt])[0]  # (exact in the value type; +0 behind the guard)
    else:
        want = dd.sddmm_int(rp, col, U, V, k, val, m=m)
    guarded = (col < 0) | (col >= m)
    assert (want[guarded] == 0).all() and not np.signbit(want[guarded].astype(np.float64)).any()
    # U and V begin 16 rows inside larger tensors and end 16 before their ends: an unguarded column reads NaN (1000), not
    # a fault
    bigu, bigv = (torch.full((r + 32, k), float("nan") if vt in FLOATS else 1000, dtype=TORCH_DT[vt], device="cuda")
                  for r in (n, m))
    bigu[16:16 + n], bigv[16:16 + m] = dev(U), dev(V)
    got = ops.csr_sddmm(dev(rp, ot), dev(col, idt), bigu[16:16 + n], bigv[16:16 + m], val=dev(val), out=filled((len(col),), vt))
    assert same_bits(got, want), differs(got, want)


# ---- 7
@pytest.mark.parametrize("vt", list(VTS))
@pytest.mark.parametrize("name", ["staircase", "nnz0", "n0", "one"])
def test_k_zero_writes_plus_zero(ops, name, vt):
    n, m, rp, col = shape(name)
    val = -np.ones(len(col), VTS[vt])  # (a negative value: an empty sum is +0 all the same)
    out = filled((len(col),), vt)
    got = ops.csr_sddmm(dev(rp, np.int32), dev(col, np.int32), filled((n, 0), vt), filled((m, 0), vt), val=dev(val), out=out)
    assert got is out and same_bits(out, np.zeros(len(col), VTS[vt]))


@pytest.mark.parametrize("name", ["nnz0", "n0"])
def test_nothing_is_written_without_entries(ops, name):
    n, m, rp, col = shape(name)
    out = ops.csr_sddmm(dev(rp, np.int32), dev(col, np.int32), filled((n, 5), "f32"), filled((m, 5), "f32"))
    assert out.shape == (0,) and out.dtype == torch.float32


# ---- 8
def test_refusals(ops):
    from sparsebase_amd import capi
    hd = ops.handle_for(torch.device("cuda", torch.cuda.current_device()))
    lib = hd.lib
    n, m, k = 4, 3, 2
    rp, col = dev(np.array([0, 1, 2, 2, 3], np.int32)), dev(np.array([0, 2, 1], np.int32))
    val = torch.full((3,), 2.0, dtype=torch.float32, device="cuda")
    U = torch.ones((n, k), dtype=torch.float32, device="cuda")
    V = torch.ones((m, k), dtype=torch.float32, device="cuda")
    out = filled((3,), "f32")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ok = dict(it=capi.SBX_I32, vt=capi.V_F32, n=n, m=m, nnz=3, k=k, rp=rp, col=col, val=val, u=U, ldu=k, v=V, ldv=k, out=out)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.sbdd_csr_sddmm(hd.h, a["it"], a["vt"], a["n"], a["m"], a["nnz"], a["k"], p(a["rp"]), p(a["col"]), p(a["val"]),
                                p(a["u"]), a["ldu"], p(a["v"]), a["ldv"], p(a["out"]))
        return rc, lib.sbx_last_error(hd.h).decode()

    BAD, UNSUPPORTED = 1, 5
    for kw, status, word in [
            (dict(n=-1), BAD, "n is negative"), (dict(m=-1), BAD, "m is negative"), (dict(nnz=-1), BAD, "nnz is negative"),
            (dict(k=-1), BAD, "k is negative"), (dict(ldu=k - 1), BAD, "ldu"), (dict(ldv=k - 1), BAD, "ldv"),
            (dict(n=0), BAD, "nnz > 0 with n == 0"), (dict(rp=None), BAD, "row_ptr"), (dict(col=None), BAD, "col"),
            (dict(out=None), BAD, "out is NULL"), (dict(u=None), BAD, "u is NULL"), (dict(v=None), BAD, "v is NULL"),
            (dict(vt=capi.V_NONE), BAD, "value type"), (dict(vt=77), BAD, "value type"), (dict(it=9), BAD, "index type"),
            (dict(nnz=1 << 42), UNSUPPORTED, "nnz")]:
        rc, msg = call(**kw)
        assert rc == status and "sbdd_csr_sddmm" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to out"
    # k > 2^20 on a 1 x 1 matrix with buffers of the full legal size: nothing could fault even without the refusal
    kk = (1 << 20) + 1
    bu, bv = (torch.ones((1, kk), dtype=torch.float32, device="cuda") for _ in range(2))
    rc, msg = call(n=1, m=1, nnz=1, k=kk, rp=dev(np.array([0, 1], np.int32)), col=dev(np.array([0], np.int32)),
                   val=val[:1], u=bu, ldu=kk, v=bv, ldv=kk)
    assert rc == UNSUPPORTED and "sbdd_csr_sddmm" in msg and "k = " in msg, (rc, msg)
    # NULL u and v are fine where there is nothing to read: k == 0, or no entries
    assert call(k=0, ldu=0, ldv=0, u=None, v=None)[0] == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0.0, 0.0, 0.0] and not torch.signbit(out).any()
    out.fill_(float("nan"))
    assert call(nnz=0, u=None, v=None, col=None, out=None, rp=dev(np.zeros(5, np.int32)))[0] == 0
    assert call(n=0, nnz=0, rp=None)[0] == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    rc, msg = call()
    torch.cuda.synchronize()
    assert rc == 0 and out.cpu().tolist() == [4.0, 4.0, 4.0]


def test_the_tensor_layer_refuses(ops):
    rp, col = dev(np.array([0, 1], np.int32)), dev(np.array([0], np.int32))
    U = torch.ones((1, 4), dtype=torch.float32, device="cuda")
    V = torch.ones((3, 4), dtype=torch.float32, device="cuda")
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    assert ops.csr_sddmm(rp, col, U, V, val=one).cpu().tolist() == [4.0]
    for kw in (dict(U=U.cpu()),                                                             # no CPU path
               dict(V=torch.ones((4, 3), dtype=torch.float32, device="cuda").t()),           # stride(1) != 1
               dict(U=U[0]),                                                                # 1-D
               dict(U=torch.ones((2, 4), dtype=torch.float32, device="cuda")),               # rows of U against row_ptr
               dict(V=V[:, :3]),                                                            # k of U against k of V
               dict(V=V.double()),                                                          # dtypes
               dict(U=U.half(), V=V.half()),                                                # a 2-byte value type
               dict(val=one.double()), dict(val=torch.ones(2, dtype=torch.float32, device="cuda")),
               dict(out=one.double()), dict(out=torch.ones(2, dtype=torch.float32, device="cuda")),
               dict(out=torch.ones((1, 1), dtype=torch.float32, device="cuda"))):
        with pytest.raises(ValueError):
            ops.csr_sddmm(rp, col, **dict(dict(U=U, V=V), **kw))


# ---- 9
@pytest.mark.parametrize("k", [16, 65, 132])
def test_with_rcm_and_permute(ops, k):
    n, m, rp, col = shape("power_law")
    nnz = len(col)
    assert nnz < 2 ** 24  # (the origins travel as float32)
    val, U, V = _uniform("power_law", "f32", k)
    drp, dcol, dval, du, dv = dev(rp, np.int32), dev(col, np.int32), dev(val), dev(U), dev(V)
    out = ops.csr_sddmm(drp, dcol, du, dv, val=dval)
    order = ops.rcm_reorder(drp, dcol, symmetrize=True)
    origin_payload = torch.arange(nnz, dtype=torch.float32, device="cuda")
    brp, bcol, borigin = ops.permute_csr(n, n, drp, dcol, origin_payload, order, order)
    origin = borigin.long()
    assert torch.equal(torch.sort(origin).values, torch.arange(nnz, device="cuda"))
    up, vp = torch.empty_like(du), torch.empty_like(dv)
    up[order.long()], vp[order.long()] = du, dv
    outp = ops.csr_sddmm(brp, bcol, up, vp, val=dval[origin].contiguous())
    assert not torch.isnan(outp).any()
    assert torch.equal(outp.view(torch.int32), out[origin].view(torch.int32))  # bit for bit


# ---- 10
@pytest.mark.parametrize("k", [3, 64, 132])
@pytest.mark.parametrize("vt", list(VTS))
@pytest.mark.parametrize("name", ["hub_middle", "power_law"])
def test_the_sum_is_the_inner_product_with_the_spmm(ops, name, vt, k):
    """sum_p val[p] (W[row p] . X[col p]) == sum_ij W[i, j] (A X)[i, j]: the gradient identity, exact on small integers
    (every out[p] and every Y[i, j] is below 2^23; the two sums are taken in int64 on the host)."""
    n, m, rp, col = shape(name)
    val, W, X = operands(name, vt, k)
    drp, dcol, dval = dev(rp, np.int32), dev(col, np.int32), dev(val)
    out = ops.csr_sddmm(drp, dcol, dev(W), dev(X), val=dval, out=filled((len(col),), vt)).cpu().numpy()
    Y = ops.csr_spmm(drp, dcol, dev(X), val=dval, m=m).cpu().numpy()
    assert np.abs(Y).max() < 2 ** 23
    assert int(out.astype(np.int64).sum()) == int((W.astype(np.int64) * Y.astype(np.int64)).sum())
