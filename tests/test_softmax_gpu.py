"""GPU tests of include/sbsm.h through ops.csr_row_softmax, ops.csr_row_softmax_backward and
ops.csr_row_softmax_autograd, for f32 (f64 is refused: not built yet) and every index tuple, against
tests/softmax_restate.py, on the shapes of tests/test_spmv_gpu.py (the smallest at which runs cross lanes, waves, tiles of 2048 entries and chains of tiles).

  1. exact, bitwise     one constant per row and -inf at a third of the positions: every exp is exactly 1 or 0 and every
                        sum a small integer in any order, so out is exactly 1 / count or +0; the pattern form against
                        1 / len; the backward on integers in [-8, 8]
  2. the bounds         of tests/softmax_restate.py on random values, every entry
  3. one pair per row   equal values in a row have equal bits; a row's outputs sum to 1 within gamma(len, u)
  4. determinism        two calls and a second handle on another stream: identical bytes, both directions
  5. in place           out is val, dz is g
  6. special values     all -inf, NaN, +inf, huge finite values, a shift by 64
  7. test_exp_ulps      re-measures the device's exp through the public entry point
  8. refusals           every case of the header and the ValueErrors of the tensor layer
  9. autograd           the wrapper's forward and backward are the library's two calls, bit for bit
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softmax_restate as sm  # noqa: E402
from spmv_restate import gamma  # noqa: E402
from test_spmv_gpu import BOUND_SHAPES, SHAPES, TUPLES, dev, first_difference, same_bits, shape  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VTS = {"f32": np.float32}  # (f64: SBX_ERR_UNSUPPORTED until its kernels are built, include/sbsm.h)
CASES = [(t, v, s) for t in TUPLES for v in VTS for s in SHAPES]
IDS = ["-".join(c) for c in CASES]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no CPU fallback)")
    from sparsebase_amd import ops
    return ops


def csr(name):
    n, _, rp, _ = shape(name)
    return n, rp, int(rp[-1])


def rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def nan_filled(nnz, vt):
    return torch.full((nnz,), float("nan"), dtype=torch.float32 if vt == "f32" else torch.float64, device="cuda")


# ---- 1
@functools.lru_cache(None)
def masked_constant(name, vt):
    """(val, want): one integer constant per row, -inf at a third of the positions; want = 1 / count or +0, bit for bit."""
    n, rp, nnz = csr(name)
    g = np.random.default_rng(201)
    rows = rows_of(rp)
    val = g.integers(-50, 51, n).astype(VTS[vt])[rows] if nnz else np.zeros(0, VTS[vt])
    masked = g.random(nnz) < 1.0 / 3
    val[masked] = -np.inf
    count = np.bincount(rows[~masked], minlength=n)
    with np.errstate(divide="ignore"):
        want = np.where(masked, VTS[vt](0), VTS[vt](1) / count.astype(VTS[vt])[rows]).astype(VTS[vt])
    return val, want


@pytest.mark.parametrize("tup,vt,name", CASES, ids=IDS)
def test_exact_forward(ops, tup, vt, name):
    n, rp, nnz = csr(name)
    assert np.diff(rp).max(initial=0) < 2 ** 24  # (a count is exact in float32)
    val, want = masked_constant(name, vt)
    out = nan_filled(nnz, vt)
    got = ops.csr_row_softmax(dev(rp, TUPLES[tup][0]), dev(val), out=out)
    assert got is out
    assert same_bits(out, want), first_difference(out, want)  # (NaN left: an entry that was not written)


@pytest.mark.parametrize("tup,vt,name", CASES, ids=IDS)
def test_pattern(ops, tup, vt, name):
    n, rp, nnz = csr(name)
    want = (VTS[vt](1) / np.diff(rp).astype(VTS[vt])[rows_of(rp)]).astype(VTS[vt])
    out = nan_filled(nnz, vt)
    ops.csr_row_softmax(dev(rp, TUPLES[tup][0]), None, out=out, dtype=out.dtype, nnz=nnz)
    assert same_bits(out, want), first_difference(out, want)


@functools.lru_cache(None)
def small_ints(name, vt):
    """(s, g, want): integers in [-8, 8]; every partial sum of a row's dot and every dz is an integer below 2^24."""
    n, rp, nnz = csr(name)
    g = np.random.default_rng(202)
    s, gr = g.integers(-8, 9, nnz).astype(np.int64), g.integers(-8, 9, nnz).astype(np.int64)
    rows = rows_of(rp)
    d = np.zeros(n, np.int64)
    np.add.at(d, rows, s * gr)
    absdot = np.zeros(n, np.int64)
    np.add.at(absdot, rows, np.abs(s * gr))
    want = s.astype(VTS[vt]) * (gr - d[rows]).astype(VTS[vt])  # (the IEEE product: 0 times a negative difference is -0)
    return s.astype(VTS[vt]), gr.astype(VTS[vt]), want, int(absdot.max(initial=0))


@pytest.mark.parametrize("tup,vt,name", CASES, ids=IDS)
def test_exact_backward(ops, tup, vt, name):
    n, rp, nnz = csr(name)
    s, g, want, absdot = small_ints(name, vt)
    # exactness, whatever the order of the dot: a partial sum is at most the row's sum of |s g|, and |dz| <= 8 (8 + |d|)
    assert 8 * (8 + absdot) < 2 ** 24
    out = nan_filled(nnz, vt)
    got = ops.csr_row_softmax_backward(dev(rp, TUPLES[tup][0]), dev(s), dev(g), out=out)
    assert got is out
    assert same_bits(out, want), first_difference(out, want)


# ---- 2
BOUNDED = BOUND_SHAPES + ("power_law",)


@functools.lru_cache(None)
def random_values(name, vt, kind):
    """(val, ref, bound): normal values with sigma = 4, or uniform over a spread of 200 (T_i saturates in float32)."""
    n, rp, nnz = csr(name)
    g = np.random.default_rng(203)
    val = (g.normal(0, 4, nnz) if kind == "normal" else g.uniform(-100, 100, nnz)).astype(VTS[vt])
    ref = sm.softmax_wide(rp, val)
    return val, ref, sm.forward_bound(rp, val, ref, VTS[vt])


def assert_within(got, ref, bound, what):
    err = np.abs(got.cpu().numpy().astype(np.longdouble) - ref)
    worst = int(np.argmax(err - bound))
    print(f"{what}: largest error / bound = {float(np.max(err / bound)):.3g}")
    assert (err <= bound).all(), f"{what}: entry {worst}: error {err[worst]} over the bound {bound[worst]} (ref {ref[worst]})"


FORWARD_CASES = [(t, v, s, "normal") for t in TUPLES for v in VTS for s in BOUNDED] + \
    [(t, v, "hub_middle", "spread200") for t in TUPLES for v in VTS]


@pytest.mark.parametrize("tup,vt,name,kind", FORWARD_CASES, ids=["-".join(c) for c in FORWARD_CASES])
def test_forward_bound(ops, tup, vt, name, kind):
    n, rp, nnz = csr(name)
    val, ref, bound = random_values(name, vt, kind)
    got = ops.csr_row_softmax(dev(rp, TUPLES[tup][0]), dev(val), out=nan_filled(nnz, vt))
    assert_within(got, ref, bound, f"{name} {vt} {tup} {kind}")


@functools.lru_cache(None)
def backward_values(name, vt):
    n, rp, nnz = csr(name)
    s = sm.softmax_wide(rp, random_values(name, vt, "normal")[0]).astype(VTS[vt])  # (what the forward gives, rounded)
    g = np.random.default_rng(204).uniform(-1, 1, nnz).astype(VTS[vt])
    ref, S = sm.backward_wide(rp, s, g)
    return s, g, ref, sm.backward_bound(rp, S, VTS[vt])


@pytest.mark.parametrize("name", BOUNDED)
@pytest.mark.parametrize("vt", list(VTS))
@pytest.mark.parametrize("tup", list(TUPLES))
def test_backward_bound(ops, tup, vt, name):
    n, rp, nnz = csr(name)
    s, g, ref, bound = backward_values(name, vt)
    got = ops.csr_row_softmax_backward(dev(rp, TUPLES[tup][0]), dev(s), dev(g), out=nan_filled(nnz, vt))
    err = np.abs(got.cpu().numpy().astype(np.longdouble) - ref)
    worst = int(np.argmax(err - bound))
    print(f"{name} {vt} {tup}: largest error / bound = {float(np.max(err[bound > 0] / bound[bound > 0])):.3g}")
    assert (err <= bound).all(), f"entry {worst}: error {err[worst]} over the bound {bound[worst]}"


# ---- 3
@pytest.mark.parametrize("name", ["dups", "staircase", "hub_middle", "hub_last"])
@pytest.mark.parametrize("vt", list(VTS))
def test_one_pair_per_row(ops, vt, name):
    n, rp, nnz = csr(name)
    g = np.random.default_rng(205)
    rows = rows_of(rp)
    palette = g.normal(0, 4, (n, 4)).astype(VTS[vt])  # four distinct numbers per row
    val = palette[rows, g.integers(0, 4, nnz)]
    out = ops.csr_row_softmax(dev(rp, np.int32), dev(val), out=nan_filled(nnz, vt)).cpu().numpy()
    bits = out.view(np.uint32 if vt == "f32" else np.uint64)
    order = np.lexsort((val, rows))
    r, v, b = rows[order], val[order], bits[order]
    same = (r[1:] == r[:-1]) & (v[1:] == v[:-1])
    bad = np.nonzero(same & (b[1:] != b[:-1]))[0]
    assert len(bad) == 0, f"{len(bad)} pairs of equal values in one row with different bits, first in row {r[bad[:1]]}"
    assert same.sum() > nnz // 2
    total = np.zeros(n, np.longdouble)
    np.add.at(total, rows, out.astype(np.longdouble))
    length = np.diff(rp)
    off = np.abs(total - 1)[length > 0]
    assert (off <= gamma(length[length > 0], sm.unit(VTS[vt]))).all(), f"a row's outputs are {off.max()} away from 1"


# ---- 4
@pytest.mark.parametrize("name", ["hub_middle", "power_law"])
@pytest.mark.parametrize("vt", list(VTS))
def test_determinism(ops, vt, name):
    from sparsebase_amd import capi
    n, rp, nnz = csr(name)
    val = random_values(name, vt, "normal")[0]
    s, g, _, _ = backward_values(name, vt)
    drp, dval, ds, dg = dev(rp, np.int32), dev(val), dev(s), dev(g)
    f1, f2 = (ops.csr_row_softmax(drp, dval).cpu().numpy() for _ in range(2))
    b1, b2 = (ops.csr_row_softmax_backward(drp, ds, dg).cpu().numpy() for _ in range(2))
    torch.cuda.synchronize()
    lib, h, st = capi.load(), C.c_void_p(), torch.cuda.Stream()
    assert lib.sbx_create(torch.cuda.current_device(), C.byref(h)) == 0
    try:
        assert lib.sbx_set_stream(h, C.c_void_p(st.cuda_stream)) == 0
        f3, b3 = nan_filled(nnz, vt), nan_filled(nnz, vt)
        torch.cuda.synchronize()
        p = lambda t: C.c_void_p(t.data_ptr())
        code = capi.V_F32 if vt == "f32" else capi.V_F64
        assert lib.sbsm_csr_row_softmax(h, capi.SBX_I32, code, n, nnz, p(drp), p(dval), p(f3)) == 0, lib.sbx_last_error(h).decode()
        assert lib.sbsm_csr_row_softmax_backward(h, capi.SBX_I32, code, n, nnz, p(drp), p(ds), p(dg), p(b3)) == 0, \
            lib.sbx_last_error(h).decode()
        st.synchronize()
    finally:
        lib.sbx_sync(h)
        lib.sbx_destroy(h)
    assert not np.isnan(f1).any() and not np.isnan(b1).any()
    assert same_bits(f2, f1) and same_bits(f3, f1)
    assert same_bits(b2, b1) and same_bits(b3, b1)


# ---- 5
@pytest.mark.parametrize("name", ["staircase", "hub_middle", "power_law"])
@pytest.mark.parametrize("vt", list(VTS))
def test_in_place(ops, vt, name):
    n, rp, nnz = csr(name)
    val = random_values(name, vt, "normal")[0]
    s, g, _, _ = backward_values(name, vt)
    drp = dev(rp, np.int32)
    want = ops.csr_row_softmax(drp, dev(val)).cpu().numpy()
    buf = dev(val)
    assert ops.csr_row_softmax(drp, buf, out=buf) is buf
    assert same_bits(buf, want), first_difference(buf, want)
    want = ops.csr_row_softmax_backward(drp, dev(s), dev(g)).cpu().numpy()
    buf = dev(g)
    assert ops.csr_row_softmax_backward(drp, dev(s), buf, out=buf) is buf
    assert same_bits(buf, want), first_difference(buf, want)


# ---- 6
@pytest.mark.parametrize("vt", list(VTS))
def test_special_values(ops, vt):
    """The staircase has rows that end on, straddle and begin at a span boundary; the hub is a row over 35 spans."""
    for name in ("staircase", "hub_middle"):
        n, rp, nnz = csr(name)
        val = random_values(name, vt, "normal")[0].copy()
        length = np.diff(rp)
        if name == "staircase":
            crossing = [i for i in range(n) if length[i] > 1 and rp[i] // 2048 != (rp[i + 1] - 1) // 2048]
            all_masked, with_nan, with_inf = crossing[0], crossing[2], crossing[4]
            val[rp[with_nan] + 1] = np.nan
            val[rp[with_inf + 1] - 1] = np.inf  # (its last entry: beyond the boundary)
        else:
            hub = int(np.argmax(length))
            all_masked, with_nan, with_inf = hub - 2 if length[hub - 2] else hub - 1, hub, None
            val[rp[hub] + 40000] = np.nan
        val[rp[all_masked]:rp[all_masked + 1]] = -np.inf
        ref = sm.softmax_wide(rp, val)
        got = ops.csr_row_softmax(dev(rp, np.int32), dev(val), out=nan_filled(nnz, vt)).cpu().numpy()
        assert length[all_masked] > 0 and same_bits(got[rp[all_masked]:rp[all_masked + 1]], np.zeros(length[all_masked], VTS[vt]))
        poisoned = np.isnan(ref)
        assert poisoned.sum() == length[with_nan] + (length[with_inf] if with_inf is not None else 0)
        assert (np.isnan(got) == poisoned).all()  # every entry of those rows, and of no other
        ok = ~poisoned
        bound = sm.forward_bound(rp, val, ref, VTS[vt])
        assert (np.abs(got[ok].astype(np.longdouble) - ref[ok]) <= bound[ok]).all()
        if name == "hub_middle":  # +inf inside the hub
            val[rp[hub] + 40000] = np.inf
            got = ops.csr_row_softmax(dev(rp, np.int32), dev(val), out=nan_filled(nnz, vt)).cpu().numpy()
            assert (np.isnan(got) == poisoned).all()


@pytest.mark.parametrize("vt", list(VTS))
def test_huge_values_and_shift(ops, vt):
    big = 3e38 if vt == "f32" else 1e308
    rp = np.array([0, 2, 6, 6, 9])
    val = np.array([big, big, big, -big, big, -big, -big, -big, 0.0], VTS[vt])
    got = ops.csr_row_softmax(dev(rp, np.int64), dev(val)).cpu().numpy()
    ref = sm.softmax_wide(rp, val)
    assert np.isfinite(got).all() and got[0] == 0.5 and got[1] == 0.5
    assert (np.abs(got.astype(np.longdouble) - ref) <= sm.forward_bound(rp, val, ref, VTS[vt])).all()
    for name in ("staircase", "hub_middle"):  # softmax(v) and softmax(v + 64): the shift is exact in the type
        n, rp, nnz = csr(name)
        val = (np.round(random_values(name, vt, "normal")[0] * 1024) / 1024).astype(VTS[vt])
        assert ((val + VTS[vt](64)) - VTS[vt](64) == val).all()
        ref = sm.softmax_wide(rp, val)
        bound = sm.forward_bound(rp, val, ref, VTS[vt])
        for v in (val, val + VTS[vt](64)):
            assert_within(ops.csr_row_softmax(dev(rp, np.int32), dev(v)), ref, bound, f"{name} {vt} shift")


# ---- 7
def measure_exp(ops, vt):
    """The largest |exp_device(t) - exp(t)| / (u exp(t)) over 2^16 rows {0, t}: s_i = 1 exactly, the second output is
    exp(t) bit for bit."""
    lo, hi = (-87.0, -17.4) if vt == "f32" else (-708.0, -37.5)
    count = 1 << 16
    t = np.random.default_rng(206).uniform(lo, hi, count).astype(VTS[vt])
    val = np.zeros(2 * count, VTS[vt])
    val[1::2] = t
    got = ops.csr_row_softmax(dev(np.arange(0, 2 * count + 1, 2), np.int32), dev(val)).cpu().numpy()
    assert (got[0::2] == 1).all()
    want = np.exp(t.astype(np.longdouble))
    return float(np.max(np.abs(got[1::2].astype(np.longdouble) - want) / (sm.unit(VTS[vt]) * want)))


@pytest.mark.parametrize("vt", list(VTS))
def test_exp_ulps(ops, vt):
    measured = measure_exp(ops, vt)
    print(f"exp {vt}: measured {measured:.4f} u, EXP_ULPS = {sm.EXP_ULPS}")
    assert measured <= sm.EXP_ULPS / 2


# ---- 8
def test_refusals(ops):
    from sparsebase_amd import capi
    hd = ops.handle_for(torch.device("cuda", torch.cuda.current_device()))
    lib = hd.lib
    rp = dev(np.array([0, 1, 2, 2, 3], np.int32))
    a, b, o = (torch.full((3,), 2.0, dtype=torch.float32, device="cuda") for _ in range(3))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def fwd(it=capi.SBX_I32, vt=capi.V_F32, n=4, nnz=3, rp=rp, val=a, out=o):
        return lib.sbsm_csr_row_softmax(hd.h, it, vt, n, nnz, p(rp), p(val), p(out)), lib.sbx_last_error(hd.h).decode()

    def bwd(it=capi.SBX_I32, vt=capi.V_F32, n=4, nnz=3, rp=rp, s=a, g=b, out=o):
        return lib.sbsm_csr_row_softmax_backward(hd.h, it, vt, n, nnz, p(rp), p(s), p(g), p(out)), \
            lib.sbx_last_error(hd.h).decode()

    BAD, UNSUPPORTED = 1, 5
    shared = [(dict(n=-1), BAD, "n is negative"), (dict(nnz=-1), BAD, "nnz is negative"),
              (dict(n=0), BAD, "nnz > 0 with n == 0"), (dict(rp=None), BAD, "row_ptr is NULL"),
              (dict(it=7), BAD, "index type"), (dict(vt=capi.V_NONE), BAD, "value type"), (dict(vt=99), BAD, "value type"),
              (dict(vt=capi.V_F64), UNSUPPORTED, "F64 is not built"), (dict(vt=capi.V_I32), UNSUPPORTED, "value type"), (dict(vt=capi.V_I64), UNSUPPORTED, "value type"),
              (dict(vt=capi.V_U32), UNSUPPORTED, "value type"), (dict(vt=capi.V_U64), UNSUPPORTED, "value type"),
              (dict(nnz=1 << 42), UNSUPPORTED, "nnz")]
    for call, name, extra in ((fwd, "sbsm_csr_row_softmax", [(dict(out=None), BAD, "out is NULL")]),
                              (bwd, "sbsm_csr_row_softmax_backward", [(dict(out=None), BAD, "dz is NULL"),
                                                                     (dict(s=None), BAD, "s is NULL"),
                                                                     (dict(g=None), BAD, "g is NULL")])):
        for kw, status, word in shared + extra:
            rc, msg = call(**kw)
            assert rc == status and word in msg and msg.startswith(name + ":"), (kw, rc, msg)
        assert call(n=0, nnz=0, rp=None, out=None)[0] == 0  # n == 0 and nnz == 0: SBX_OK, nothing written
        o.fill_(7)
        assert call(nnz=0)[0] == 0
        torch.cuda.synchronize()
        assert (o == 7).all()
        assert call()[0] == 0
    assert fwd(val=None)[0] == 0  # a pattern
    torch.cuda.synchronize()
    assert o.tolist() == [1.0, 1.0, 1.0]


def test_tensor_layer_refusals(ops):
    rp = dev(np.array([0, 1, 3], np.int32))
    f32 = lambda k: torch.ones(k, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="dtype= and nnz="):
        ops.csr_row_softmax(rp, None)
    with pytest.raises(ValueError, match="must be float32"):
        ops.csr_row_softmax(rp, torch.ones(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="must be float32"):
        ops.csr_row_softmax(rp, torch.ones(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="must be float32"):
        ops.csr_row_softmax_backward(rp, torch.ones(3, dtype=torch.float64, device="cuda"), torch.ones(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="out must be 1-D"):
        ops.csr_row_softmax(rp, f32(3), out=f32(4))
    with pytest.raises(ValueError, match="out must be 1-D"):
        ops.csr_row_softmax(rp, f32(3), out=torch.ones(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="val must be 1-D"):
        ops.csr_row_softmax(rp, torch.ones((3, 1), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="g must be 1-D"):
        ops.csr_row_softmax_backward(rp, f32(3), f32(2))
    with pytest.raises(ValueError, match="g must be 1-D"):
        ops.csr_row_softmax_backward(rp, f32(3), torch.ones(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="device tensors only"):
        ops.csr_row_softmax(rp, torch.ones(3))
    assert ops.csr_row_softmax(rp, None, dtype=torch.float32, nnz=3).tolist() == [1.0, 0.5, 0.5]


# ---- 9
def test_autograd_backward_is_the_library_s(ops):
    """ops.csr_row_softmax_autograd: the forward's bits, and through torch's autograd the bits of
    ops.csr_row_softmax_backward, held to the backward bound; 12 rows, an empty one and rows of one entry."""
    lengths = [3, 0, 1, 5, 2, 7, 4, 1, 6, 2, 3, 8]
    rp = np.concatenate([[0], np.cumsum(lengths)])
    g = np.random.default_rng(209)
    val, grad = g.normal(0, 1, rp[-1]).astype(np.float32), g.uniform(-1, 1, rp[-1]).astype(np.float32)
    drp = dev(rp, np.int64)
    v = dev(val).requires_grad_(True)
    s = ops.csr_row_softmax_autograd(drp, v)
    assert s.requires_grad and same_bits(s.detach(), ops.csr_row_softmax(drp, dev(val)).cpu().numpy())
    s.backward(dev(grad))
    assert same_bits(v.grad, ops.csr_row_softmax_backward(drp, s.detach(), dev(grad)).cpu().numpy())
    ref, S = sm.backward_wide(rp, s.detach().cpu().numpy(), grad)
    assert (np.abs(v.grad.cpu().numpy().astype(np.longdouble) - ref) <= sm.backward_bound(rp, S, np.float32)).all()
