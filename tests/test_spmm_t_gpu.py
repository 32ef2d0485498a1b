"""GPU tests of include/sbmt.h through ops.csr_transpose_plan and ops.csr_spmm_t, for every value type and every index
tuple, against tests/transpose_restate.py and against ops.csr_spmm on the materialised transpose.  The shapes are those
of tests/test_spmv_gpu.py, imported, and one rectangle made here ("rect": 6000 x 300, a column of 4100 entries that
crosses two span boundaries once transposed, one of exactly 2048, the first and the last column empty, three duplicated
entries, two rows with unsorted columns).

  1. the plan, exact    col_ptr, row and perm equal the restatement in all three tuples; with sorted rows (col_ptr, row)
                        are ops.csr_to_csc's and val[perm] its val_out, bitwise (4- and 8-byte values)
  2. the product is the existing product on the materialised transpose, bitwise: uniform values in (-1, 1) (the integer
                        types: integers of 21 bits, which wrap), Y pre-filled with NaN or -1
  3. exact integers     values and X in [-8, 8] against the restatement, k = 1 at unit strides and as a slice included
  4. leading dimensions and alignment   odd-offset slices (ldx = k + 5, ldy = k + 7) and aligned slices of 2 k-wide
                        tensors, the padding untouched
  5. determinism        two calls and a second handle on another stream: identical bytes; one vector replicated over
                        the k columns of X: k bit-equal columns of Y
  6. guards             3000 positions of perm set to nnz, nnz + 1, -1 and 3000 of row to n, -1; X a slice of exactly n
                        rows between rows of NaN, val a slice between NaNs; the restatement with those entries dropped
  7. pattern            val=None equals val=ones bitwise; perm == NULL is accepted through the C call
  8. refusals           every case of the header, with its status and the argument's name; a refused call writes nothing
  9. k = 1 rounding bound   |Y - Yhat| <= (gamma(len, u) + gamma(len, u_wide)) S: derived, not measured

The k of section 2 stand on both sides of every form boundary tests/test_spmm_gpu.py lists (its docstring): 32 | 33 and
64 | 65, 128 | 129, 256 | 257 at one column per lane; 128 | 132 and 256 | 260 (4-byte values), 64 | 66 and 128 | 130
(8-byte values) at 16 bytes per lane; 12 and 20 for groups that do not divide the wave.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmv_restate as mv  # noqa: E402
import transpose_restate as tr  # noqa: E402
from test_spmv_gpu import SHAPES, TUPLES, VTS, _wide_for, dev, ops, same_bits, shape  # noqa: E402,F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TORCH_DT = {"f32": torch.float32, "f64": torch.float64, "i32": torch.int32, "i64": torch.int64}
K_I32_F32 = [2, 3, 4, 8, 12, 20, 32, 33, 64, 65, 128, 129, 132, 256, 257, 260]
K_OTHER = [3, 8, 33, 64, 66, 129, 130, 132, 260]
K_MAX = 260
K_EXACT = 132
ALL_SHAPES = list(SHAPES) + ["rect"]
PLAN_SHAPES = ["staircase", "hub_middle", "power_law", "dups", "nnz0", "rect"]


def _rect():
    n, m = 6000, 300
    g = np.random.default_rng(811)
    free = np.array([c for c in range(1, m - 1) if c not in (7, 150)])  # (columns 0 and m - 1 stay empty)
    rows = []
    for i in range(n):
        r = set(g.choice(free, int(g.integers(0, 4)), replace=False).tolist())
        if i < 4100:
            r.add(7)
        if 1000 <= i < 3048:
            r.add(150)
        rows.append(sorted(r))
    for i in (5, 2000, 5999):  # three duplicated (row, column) entries
        mine = [c for c in rows[i] if c not in (7, 150)]  # (the two counted columns keep their counts)
        rows[i] = sorted(rows[i] + ([mine[0]] if mine else [20, 20]))
    for i in (1500, 4000):  # unsorted columns inside two rows
        while len(set(rows[i])) < 3:
            rows[i] = sorted(set(rows[i]) | {int(g.choice(free))})
        rows[i] = rows[i][::-1]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c in r], np.int64)
    cnt = np.bincount(col, minlength=m)
    assert cnt[7] == 4100 and cnt[150] == 2048 and cnt[0] == 0 and cnt[m - 1] == 0
    return n, m, rp, col


@functools.lru_cache(None)
def tshape(name):
    return _rect() if name == "rect" else shape(name)


@functools.lru_cache(None)
def plan_ref(name):
    n, m, rp, col = tshape(name)
    return tr.plan(rp, col, m)


@functools.lru_cache(None)
def dev_plan(ops, name, tup):
    """The library's plan of a shape, built once per index tuple and held to the restatement in section 1."""
    n, m, rp, col = tshape(name)
    ot, idt = TUPLES[tup]
    return ops.csr_transpose_plan(dev(rp, ot), dev(col, idt), m)


def prefilled(n, k, vt, width=None):
    return torch.full((n, k if width is None else width), float("nan") if vt in ("f32", "f64") else -1, dtype=TORCH_DT[vt],
                      device="cuda")


def rows(t):
    """t itself, or for a tensor without elements (n == 0) one of its shape with the strides of a row-major block: numpy
    and torch give such a tensor strides of 0, which say nothing and which the tensor layer refuses."""
    return t if t.numel() else torch.empty(tuple(t.shape), dtype=t.dtype, device=t.device)


def differs(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{got.dtype}{got.shape} for {want.dtype}{want.shape}"
    bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
    return f"{len(bad)} of {want.size} elements differ, first (row, column) {bad[:5].tolist()}: " \
           f"{[got[tuple(b)] for b in bad[:5]]} for {[want[tuple(b)] for b in bad[:5]]}"


# ---- 1
@pytest.mark.parametrize("tup", list(TUPLES))
@pytest.mark.parametrize("name", PLAN_SHAPES)
def test_plan_exact(ops, name, tup):
    n, m, rp, col = tshape(name)
    ot, idt = TUPLES[tup]
    cp, row, perm = plan_ref(name)
    p = dev_plan(ops, name, tup)
    assert (p.n, p.m) == (n, m)
    assert same_bits(p.col_ptr, cp.astype(ot)), "col_ptr"
    assert same_bits(p.perm, perm.astype(ot)), "perm"
    assert same_bits(p.row, row.astype(idt)), "row"


@pytest.mark.parametrize("vt", ["f32", "f64"])
@pytest.mark.parametrize("tup", list(TUPLES))
@pytest.mark.parametrize("name", ["staircase", "power_law", "rect"])
def test_plan_is_csr_to_csc_on_sorted_rows(ops, name, tup, vt):
    n, m, rp, col = tshape(name)
    ot, idt = TUPLES[tup]
    col = col[np.lexsort((col, tr.rows_of(rp, len(col))))]  # every row's columns ascending
    val = np.random.default_rng(812).uniform(-1, 1, len(col)).astype(VTS[vt])
    drp, dcol, dval = dev(rp, ot), dev(col, idt), dev(val)
    p = ops.csr_transpose_plan(drp, dcol, m)
    cp, ro, vo = ops.csr_to_csc(n, m, drp, dcol, dval)
    assert torch.equal(p.col_ptr, cp) and torch.equal(p.row, ro)
    assert same_bits(dval[p.perm.long()], vo.cpu().numpy())


# ---- 2
@functools.lru_cache(None)
def uniform_dev(name, vt):
    """(val, X of K_MAX columns) on the device: uniform in (-1, 1); the integer types: integers of 21 bits."""
    n, m, rp, col = tshape(name)
    g = np.random.default_rng(813)
    if vt in ("f32", "f64"):
        draw = lambda size: g.uniform(-1.0, 1.0, size).astype(VTS[vt])
    else:
        draw = lambda size: g.integers(-2 ** 20, 2 ** 20, size).astype(VTS[vt])
    return dev(draw(len(col))), dev(draw((n, K_MAX)))


BITWISE = [("i32", "f32", s, k) for s in ALL_SHAPES for k in K_I32_F32] + \
          [(t, v, s, k) for t in TUPLES for v in VTS if (t, v) != ("i32", "f32")
           for s in ("staircase", "hub_middle", "rect") for k in K_OTHER]


@pytest.mark.parametrize("tup,vt,name,k", BITWISE, ids=[f"{t}-{v}-{s}-k{k}" for t, v, s, k in BITWISE])
def test_bits_of_spmm_on_the_materialised_transpose(ops, tup, vt, name, k):
    n, m, rp, col = tshape(name)
    p = dev_plan(ops, name, tup)
    val, X = uniform_dev(name, vt)
    x = rows(X[:, :k].contiguous())
    got = ops.csr_spmm_t(p, x, val, out=prefilled(m, k, vt))
    want = ops.csr_spmm(p.col_ptr, p.row, x, val=val[p.perm.long()], m=n, out=prefilled(m, k, vt))
    assert got.shape == (m, k)
    if vt in ("f32", "f64"):
        assert not torch.isnan(got).any(), "an element of Y was not written"
    assert same_bits(got, want.cpu().numpy()), differs(got, want.cpu().numpy())


# ---- 3
@functools.lru_cache(None)
def small_ints(name):
    n, m, rp, col = tshape(name)
    g = np.random.default_rng(814)
    return g.integers(-8, 9, len(col)), g.integers(-8, 9, (n, K_EXACT))


@functools.lru_cache(None)
def exact_ref(name, pattern=False):
    """The restatement's m x K_EXACT product in int64, computed once."""
    n, m, rp, col = tshape(name)
    val, X = small_ints(name)
    cp, row, perm = plan_ref(name)
    ref = tr.spmm_t_int(n, cp, row, perm, X.reshape(-1), K_EXACT, None if pattern else val)
    assert np.abs(ref).max(initial=0) < 2 ** 23  # exact in float32 in any order
    return ref


def operands(name, vt, k):
    val, X = small_ints(name)
    return val.astype(VTS[vt]), np.ascontiguousarray(X[:, :k]).astype(VTS[vt])


EXACT = [("i32", "f32", s, k) for s in ALL_SHAPES for k in (1, 2, 8, 33, 64, 132)] + \
        [(t, v, s, k) for t in TUPLES for v in VTS if (t, v) != ("i32", "f32")
         for s in ("staircase", "hub_middle", "rect") for k in (1, 3, 64, 66)]


@pytest.mark.parametrize("tup,vt,name,k", EXACT, ids=[f"{t}-{v}-{s}-k{k}" for t, v, s, k in EXACT])
def test_exact(ops, tup, vt, name, k):
    n, m, rp, col = tshape(name)
    val, X = operands(name, vt, k)
    want = np.ascontiguousarray(exact_ref(name)[:, :k]).astype(VTS[vt])
    y = prefilled(m, k, vt)
    got = ops.csr_spmm_t(dev_plan(ops, name, tup), rows(dev(X)), dev(val), out=y)  # (k = 1: unit strides)
    assert got is y
    assert same_bits(y, want), differs(y, want)


# ---- 4
@pytest.mark.parametrize("k", [1, 4, 7, 64, 68, 130])
@pytest.mark.parametrize("vt", ["f32", "i64"])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "nnz0", "rect"])
def test_leading_dimensions_and_alignment(ops, name, vt, k):
    n, m, rp, col = tshape(name)
    val, X = operands(name, vt, k)
    want = np.ascontiguousarray(exact_ref(name)[:, :k]).astype(VTS[vt])
    xw = prefilled(n, k, vt, k + 5)
    xw[:, 3:3 + k] = dev(X)
    yw = prefilled(m, k, vt, k + 7)
    sentinel = yw.clone()
    xs, ys = xw[:, 3:3 + k], yw[:, 3:3 + k]  # (k = 1: a slice, not unit strides)
    assert xs.stride(0) == k + 5 and ys.stride(0) == k + 7 and xs.data_ptr() % 16 != 0 and ys.data_ptr() % 16 != 0
    got = ops.csr_spmm_t(dev_plan(ops, name, "i32"), xs, dev(val), out=ys)
    assert got is ys
    assert same_bits(ys.contiguous(), want), differs(ys.contiguous(), want)
    outside = torch.ones_like(yw, dtype=torch.bool)
    outside[:, 3:3 + k] = False
    assert same_bits(yw[outside], sentinel[outside].cpu().numpy()), "the padding of Y was written"


@pytest.mark.parametrize("k", [8, 64, 66, 132])
@pytest.mark.parametrize("tup,vt", [("i32", "f32"), ("i64", "f64"), ("i32_n64", "i64")])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "nnz0", "rect"])
def test_aligned_leading_dimensions(ops, name, tup, vt, k):
    n, m, rp, col = tshape(name)
    val, X = operands(name, vt, k)
    want = np.ascontiguousarray(exact_ref(name)[:, :k]).astype(VTS[vt])
    xw = prefilled(n, k, vt, 2 * k)
    xw[:, :k] = dev(X)
    yw = prefilled(m, k, vt, 2 * k)
    sentinel = yw.clone()
    xs, ys = xw[:, :k], yw[:, :k]
    assert xs.data_ptr() % 16 == 0 and ys.data_ptr() % 16 == 0 and (2 * k * xs.element_size()) % 16 == 0
    assert (xs.stride(0) == 2 * k or n <= 1) and (ys.stride(0) == 2 * k or m <= 1)
    got = ops.csr_spmm_t(dev_plan(ops, name, tup), xs, dev(val), out=ys)
    assert got is ys
    assert same_bits(ys.contiguous(), want), differs(ys.contiguous(), want)
    assert same_bits(yw[:, k:].contiguous(), sentinel[:, k:].cpu().numpy()), "the padding of Y was written"
    # the same slices through the existing product on the materialised transpose: the same bits at the same alignment
    p = dev_plan(ops, name, tup)
    y2 = prefilled(m, k, vt, 2 * k)
    ops.csr_spmm(p.col_ptr, p.row, xs, val=dev(val)[p.perm.long()], m=n, out=y2[:, :k])
    assert same_bits(y2, yw.cpu().numpy())


# ---- 5
def _call(lib, h, capi, tup, vt, n, m, nnz, k, p, val, x, ldx, y, ldy, perm="plan"):
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    it = {"i32": capi.SBX_I32, "i64": capi.SBX_I64, "i32_n64": capi.SBX_I32_N64}[tup]
    code = {"f32": capi.V_F32, "f64": capi.V_F64, "i32": capi.V_I32, "i64": capi.V_I64}[vt]
    return lib.sbmt_csr_spmm_t(h, it, code, n, m, nnz, k, ptr(p.col_ptr), ptr(p.row), ptr(p.perm if perm == "plan" else perm),
                               ptr(val), ptr(x), ldx, ptr(y), ldy)


@pytest.mark.parametrize("k", [1, 8, 129, 130])
@pytest.mark.parametrize("name", ["hub_middle", "rect"])
@pytest.mark.parametrize("vt", ["f32", "f64"])
def test_determinism(ops, vt, name, k):
    from sparsebase_amd import capi
    n, m, rp, col = tshape(name)
    p = dev_plan(ops, name, "i32")
    val, X = uniform_dev(name, vt)
    x = X[:, :k].contiguous()
    y1 = ops.csr_spmm_t(p, x, val).cpu().numpy()
    y2 = ops.csr_spmm_t(p, x, val).cpu().numpy()
    torch.cuda.synchronize()
    lib, h, s = capi.load(), C.c_void_p(), torch.cuda.Stream()
    assert lib.sbx_create(torch.cuda.current_device(), C.byref(h)) == 0
    try:
        assert lib.sbx_set_stream(h, C.c_void_p(s.cuda_stream)) == 0
        y3 = prefilled(m, k, vt)
        torch.cuda.synchronize()
        rc = _call(lib, h, capi, "i32", vt, n, m, len(col), k, p, val, x, k, y3, k)
        assert rc == 0, lib.sbx_last_error(h).decode()
        s.synchronize()
    finally:
        lib.sbx_sync(h)
        lib.sbx_destroy(h)
    assert not np.isnan(y1).any()
    assert same_bits(y2, y1) and same_bits(y3, y1)


@pytest.mark.parametrize("k", [5, 64, 66, 132, 257, 260])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "rect"])
@pytest.mark.parametrize("vt", ["f32", "f64"])
def test_columns_agree(ops, vt, name, k):
    n, m, rp, col = tshape(name)
    val, X = uniform_dev(name, vt)
    x = X[:, :1].repeat(1, k).contiguous()
    y = ops.csr_spmm_t(dev_plan(ops, name, "i32"), x, val, out=prefilled(m, k, vt)).cpu().numpy()
    assert not np.isnan(y).any()
    cols = np.ascontiguousarray(y.T).view(np.uint8).reshape(k, m * y.itemsize)
    odd = [j for j in range(1, k) if not np.array_equal(cols[j], cols[0])]
    assert not odd, f"columns {odd[:8]} of Y differ from column 0 for equal columns of X"


# ---- 6
@pytest.mark.parametrize("k", [3, 64])
@pytest.mark.parametrize("tup", list(TUPLES))
@pytest.mark.parametrize("vt", list(VTS))
def test_guards(ops, vt, tup, k):
    """Malformed data the header promises to survive: positions and rows outside their arrays contribute nothing and
    nothing is loaded through them (an unguarded one would read the NaN, or 1000, around val and X)."""
    name = "power_law"
    n, m, rp, col = tshape(name)
    ot, idt = TUPLES[tup]
    nnz = len(col)
    val, X = operands(name, vt, k)
    cp, row, perm = plan_ref(name)
    g = np.random.default_rng(815)
    perm, row = perm.copy(), row.copy()
    pick = g.choice(nnz, 6000, replace=False)
    perm[pick[:3000]] = np.array([nnz, nnz + 1, -1])[g.integers(0, 3, 3000)]
    row[pick[3000:]] = np.array([n, -1])[g.integers(0, 2, 3000)]
    perm[[0, nnz - 1]] = nnz, -1
    row[[1, nnz - 2]] = n, -1
    want = tr.spmm_t_int(n, cp, row, perm, X.astype(np.int64).reshape(-1), k, val.astype(np.int64)).astype(VTS[vt])
    fill = float("nan") if vt in ("f32", "f64") else 1000
    bigx = torch.full((n + 32, k), fill, dtype=TORCH_DT[vt], device="cuda")
    bigx[16:16 + n] = dev(X)
    bigv = torch.full((nnz + 32,), fill, dtype=TORCH_DT[vt], device="cuda")
    bigv[16:16 + nnz] = dev(val)
    p = ops.TransposePlan(n, m, dev(cp, ot), dev(row, idt), dev(perm, ot))
    got = ops.csr_spmm_t(p, bigx[16:16 + n], bigv[16:16 + nnz], out=prefilled(m, k, vt))
    assert same_bits(got, want), differs(got, want)


# ---- 7
@pytest.mark.parametrize("k", [1, 3, 64, 129])
@pytest.mark.parametrize("tup,vt", [("i32", "f32"), ("i64", "f64"), ("i32_n64", "i32"), ("i32", "i64")])
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "dups", "rect"])
def test_pattern(ops, name, tup, vt, k):
    from sparsebase_amd import capi
    n, m, rp, col = tshape(name)
    _, X = operands(name, vt, k)
    p, dx = dev_plan(ops, name, tup), dev(X)
    got = ops.csr_spmm_t(p, dx, out=prefilled(m, k, vt))
    ones = ops.csr_spmm_t(p, dx, torch.ones(len(col), dtype=dx.dtype, device="cuda"), out=prefilled(m, k, vt))
    want = np.ascontiguousarray(exact_ref(name, pattern=True)[:, :k]).astype(VTS[vt])
    assert same_bits(got, want), differs(got, want)
    assert same_bits(ones, want), differs(ones, want)
    hd = ops.handle_for(dx.device)
    y = prefilled(m, k, vt)
    rc = _call(hd.lib, hd.h, capi, tup, vt, n, m, len(col), k, p, None, dx, k, y, k, perm=None)  # perm == NULL
    assert rc == 0, hd.lib.sbx_last_error(hd.h).decode()
    assert same_bits(y, want), differs(y, want)


# ---- 8
def test_refusals_of_the_product(ops):
    from sparsebase_amd import capi
    hd = ops.handle_for(torch.device("cuda", torch.cuda.current_device()))
    lib = hd.lib
    n, m, k = 3, 4, 2  # A is 3 x 4 with the entries (0, 0), (1, 2), (2, 1); A^T has 4 rows
    cp, row, perm = dev(np.array([0, 1, 2, 3, 3], np.int32)), dev(np.array([0, 2, 1], np.int32)), dev(np.array([0, 2, 1], np.int32))
    val = torch.ones(3, dtype=torch.float32, device="cuda")
    X = torch.ones((n, k), dtype=torch.float32, device="cuda")
    Y = prefilled(m, k, "f32")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ok = dict(it=capi.SBX_I32, vt=capi.V_F32, n=n, m=m, nnz=3, k=k, cp=cp, row=row, perm=perm, val=val, x=X, ldx=k, y=Y, ldy=k)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.sbmt_csr_spmm_t(hd.h, a["it"], a["vt"], a["n"], a["m"], a["nnz"], a["k"], p(a["cp"]), p(a["row"]), p(a["perm"]),
                                 p(a["val"]), p(a["x"]), a["ldx"], p(a["y"]), a["ldy"])
        return rc, lib.sbx_last_error(hd.h).decode()

    BAD, UNSUPPORTED = 1, 5
    for kw, status, word in [
            (dict(n=-1), BAD, "n is negative"), (dict(m=-1), BAD, "m is negative"), (dict(nnz=-1), BAD, "nnz is negative"),
            (dict(k=-1), BAD, "k is negative"), (dict(ldx=k - 1), BAD, "ldx"), (dict(ldy=k - 1), BAD, "ldy"),
            (dict(m=0), BAD, "nnz > 0 with m == 0"), (dict(cp=None), BAD, "col_ptr"), (dict(row=None), BAD, "row is NULL"),
            (dict(perm=None), BAD, "perm is NULL"), (dict(x=None), BAD, "x is NULL"), (dict(y=None), BAD, "y is NULL"),
            (dict(vt=capi.V_NONE), BAD, "value type"), (dict(vt=77), BAD, "value type"), (dict(it=9), BAD, "index type"),
            (dict(nnz=1 << 42), UNSUPPORTED, "nnz")]:
        rc, msg = call(**kw)
        assert rc == status and "sbmt_csr_spmm_t" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(Y).all(), "a refused call wrote to Y"
    # k > 2^20 on a 1 x 1 matrix with buffers of the full legal size: nothing could fault even without the refusal
    kk = (1 << 20) + 1
    bx, by = torch.ones((1, kk), dtype=torch.float32, device="cuda"), prefilled(1, kk, "f32")
    one = dev(np.array([0], np.int32))
    rc, msg = call(n=1, m=1, nnz=1, k=kk, cp=dev(np.array([0, 1], np.int32)), row=one, perm=one, val=val[:1], x=bx, ldx=kk,
                   y=by, ldy=kk)
    assert rc == UNSUPPORTED and "sbmt_csr_spmm_t" in msg and "k = " in msg, (rc, msg)
    torch.cuda.synchronize()
    assert torch.isnan(by).all()
    # k == 0 and m == 0 succeed and write nothing
    assert call(k=0, ldx=0, ldy=0)[0] == 0 and call(k=0)[0] == 0
    assert call(m=0, nnz=0, cp=dev(np.zeros(1, np.int32)))[0] == 0
    torch.cuda.synchronize()
    assert torch.isnan(Y).all()
    rc, msg = call()
    torch.cuda.synchronize()
    assert rc == 0 and Y.cpu().tolist() == [[1, 1], [1, 1], [1, 1], [0, 0]]


def test_refusals_of_the_plan(ops):
    from sparsebase_amd import capi
    hd = ops.handle_for(torch.device("cuda", torch.cuda.current_device()))
    lib = hd.lib
    n, m = 3, 4
    rp, col = dev(np.array([0, 1, 2, 3], np.int32)), dev(np.array([0, 2, 1], np.int32))
    outs = [torch.full((c,), -7, dtype=torch.int32, device="cuda") for c in (m + 1, 3, 3)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ok = dict(it=capi.SBX_I32, n=n, m=m, nnz=3, rp=rp, col=col, cp=outs[0], row=outs[1], perm=outs[2])

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.sbmt_csr_transpose_plan(hd.h, a["it"], a["n"], a["m"], a["nnz"], p(a["rp"]), p(a["col"]), p(a["cp"]),
                                         p(a["row"]), p(a["perm"]))
        return rc, lib.sbx_last_error(hd.h).decode()

    BAD, UNSUPPORTED = 1, 5
    for kw, status, word in [
            (dict(n=-1), BAD, "n is negative"), (dict(m=-1), BAD, "m is negative"), (dict(nnz=-1), BAD, "nnz is negative"),
            (dict(rp=None), BAD, "row_ptr is NULL"), (dict(col=None), BAD, "col is NULL"),
            (dict(cp=None), BAD, "col_ptr_out is NULL"), (dict(row=None), BAD, "row_out is NULL"),
            (dict(perm=None), BAD, "perm_out is NULL"), (dict(it=9), BAD, "index type"),
            (dict(nnz=1 << 31), UNSUPPORTED, "nnz"), (dict(n=(1 << 31) - 1), UNSUPPORTED, "n = "),
            (dict(m=(1 << 31) - 1), UNSUPPORTED, "m = ")]:
        rc, msg = call(**kw)
        assert rc == status and "sbmt_csr_transpose_plan" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all((o == -7).all() for o in outs), "a refused call wrote to an output"
    # a column outside [0, m) is found by the check of col, which is read back: a refusal, in every tuple
    for tup, (ot, idt) in TUPLES.items():
        it = {"i32": capi.SBX_I32, "i64": capi.SBX_I64, "i32_n64": capi.SBX_I32_N64}[tup]
        for bad in (m, -1):
            o = [torch.zeros(c, dtype=torch.from_numpy(np.zeros(0, t)).dtype, device="cuda")
                 for c, t in ((m + 1, ot), (3, idt), (3, ot))]
            rc, msg = call(it=it, rp=dev(np.array([0, 1, 2, 3], ot)), col=dev(np.array([0, bad, 1], idt)), cp=o[0], row=o[1],
                           perm=o[2])
            assert rc == BAD and "sbmt_csr_transpose_plan" in msg and "column" in msg, (tup, bad, rc, msg)
    with pytest.raises(capi.SbxError):
        ops.csr_transpose_plan(rp, dev(np.array([0, 4, 1], np.int32)), m)
    rc, msg = call()
    torch.cuda.synchronize()
    assert rc == 0 and [o.cpu().tolist() for o in outs] == [[0, 1, 2, 3, 3], [0, 2, 1], [0, 2, 1]]


def test_the_tensor_layer_refuses(ops):
    rp, col = dev(np.array([0, 1], np.int32)), dev(np.array([0], np.int32))
    p = ops.csr_transpose_plan(rp, col, 1)
    X = torch.ones((1, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        ops.csr_spmm_t(p, X.cpu())
    with pytest.raises(ValueError):
        ops.csr_spmm_t(p, torch.ones((4, 2), dtype=torch.float32, device="cuda").t()[:1])  # stride(1) != 1
    with pytest.raises(ValueError):
        ops.csr_spmm_t(p, X, out=torch.ones((4, 2), dtype=torch.float32, device="cuda").t()[:1])
    with pytest.raises(ValueError):
        ops.csr_spmm_t(p, X[0])  # 1-D
    with pytest.raises(TypeError):
        ops.csr_spmm_t(p, X, val=torch.ones(2, dtype=torch.float32, device="cuda"))  # one value too many
    with pytest.raises(ValueError):
        ops.csr_spmm_t(p._replace(perm=p.perm[:0]), X)  # a plan with a short array
    with pytest.raises(ValueError):
        ops.csr_spmm_t(p._replace(n=2), X)  # X holds fewer rows than the matrix


# ---- 9
@functools.lru_cache(None)
def bound_data(name, vt):
    n, m, rp, col = tshape(name)
    g = np.random.default_rng(816)

    def draw(size):  # uniform in (-1, 1), kept 2^-20 away from 0 (no product is subnormal)
        u = g.uniform(-1.0, 1.0, size)
        return np.where(np.abs(u) < 2.0 ** -20, 2.0 ** -20, u).astype(VTS[vt])
    val, x = draw(len(col)), draw((n, 1))
    wide = _wide_for(vt, len(col))
    cp, row, perm = plan_ref(name)
    return val, x, (None if wide is None else tr.spmm_t_wide(n, cp, row, perm, x.reshape(-1), 1, val, wide=wide))


@pytest.mark.parametrize("name", ["rect", "tall", "staircase", "hub_middle"])
@pytest.mark.parametrize("vt", ["f32", "f64"])
def test_k1_rounding_bound(ops, vt, name):
    n, m, rp, col = tshape(name)
    u = 2.0 ** -24 if vt == "f32" else 2.0 ** -53
    length = np.diff(plan_ref(name)[0])[:, None]
    val, x, wide = bound_data(name, vt)
    if wide is None:  # (f64 on a platform without a wider format: only the shapes of at most 2000 entries)
        return
    yhat, S, u_wide = wide
    y = ops.csr_spmm_t(dev_plan(ops, name, "i32"), dev(x), dev(val), out=prefilled(m, 1, vt)).cpu().numpy().astype(np.longdouble)
    bound = (mv.gamma(length, u) + mv.gamma(length, u_wide)) * S.astype(np.longdouble)
    err = np.abs(y - yhat.astype(np.longdouble))
    worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
    print(f"{name} {vt} k=1: largest error / bound = {float(np.max(err[bound > 0] / bound[bound > 0])):.3g}")
    assert (err <= bound).all(), f"element {worst} of a column of {length[worst[0], 0]} entries: error {err[worst]} over the bound {bound[worst]}"
