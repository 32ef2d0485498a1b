"""GPU tests of ops.csr_spmm_autograd and ops.csr_sddmm_autograd, the differentiable forms of the two products whose
backward needs the transposed product of include/sbmt.h.

  1. gradcheck       torch.autograd.gradcheck in float64 at its default tolerances on a 40 x 30 matrix of 200 entries with
                     duplicates, an empty row and an empty column: k = 5 for the product (val and X), d = 5 for the SDDMM
                     (val, U and V), and the pattern forms.  The functions are bilinear: the derivatives are exact.
  2. definitions     float32 on hub_middle: every gradient is, bit for bit, the direct ops call it is defined as
  3. needs_input_grad   with requires_grad off for an input the corresponding call is not made: a plan of empty tensors
                     would raise in csr_spmm_t, and does once X (or V) asks for its gradient
  4. one layer       SDDMM -> row softmax -> SpMM with the attention as values, on power_law at d = k = 16, loss = sum of
                     Y * R: against the same layer written with torch gathers and index_add_ in float64.  The yardstick is
                     that torch composition in float32 against the float64 one; both errors are printed.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transpose_restate as tr  # noqa: E402
from test_spmv_gpu import dev, ops, same_bits, shape  # noqa: E402,F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _small():
    """40 x 30, 200 entries: duplicates, row 11 and column 17 empty, unsorted rows."""
    g = np.random.default_rng(901)
    n, m = 40, 30
    rows = g.choice([r for r in range(n) if r != 11], 195)
    cols = g.choice([c for c in range(m) if c != 17], 195)
    rows, cols = np.concatenate([rows, rows[:5]]), np.concatenate([cols, cols[:5]])  # five duplicated entries
    o = np.argsort(rows, kind="stable")
    rows, cols = rows[o], cols[o]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    assert rp[12] == rp[11] and 17 not in cols and len(cols) == 200
    return n, m, rp, cols.astype(np.int64)


def _rand(shape_, seed, dtype=torch.float64, grad=True):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape_, generator=g, dtype=torch.float64) * 2 - 1).to(dtype).cuda().requires_grad_(grad)


# ---- 1
@pytest.mark.parametrize("pattern", [False, True])
@pytest.mark.parametrize("with_plan", [False, True])
def test_gradcheck_spmm(ops, pattern, with_plan):
    n, m, rp, col = _small()
    drp, dcol = dev(rp, np.int32), dev(col, np.int32)
    plan = ops.csr_transpose_plan(drp, dcol, m) if with_plan else None
    X = _rand((m, 5), 1)
    if pattern:
        assert torch.autograd.gradcheck(lambda x: ops.csr_spmm_autograd(drp, dcol, None, x, plan=plan), (X,))
    else:
        val = _rand((len(col),), 2)
        assert torch.autograd.gradcheck(lambda v, x: ops.csr_spmm_autograd(drp, dcol, v, x, plan=plan), (val, X))


@pytest.mark.parametrize("pattern", [False, True])
def test_gradcheck_sddmm(ops, pattern):
    n, m, rp, col = _small()
    drp, dcol = dev(rp, np.int32), dev(col, np.int32)
    plan = ops.csr_transpose_plan(drp, dcol, m)
    U, V = _rand((n, 5), 3), _rand((m, 5), 4)
    if pattern:
        assert torch.autograd.gradcheck(lambda u, v: ops.csr_sddmm_autograd(drp, dcol, u, v, plan=plan), (U, V))
    else:
        val = _rand((len(col),), 5)
        assert torch.autograd.gradcheck(lambda a, u, v: ops.csr_sddmm_autograd(drp, dcol, u, v, val=a, plan=plan), (val, U, V))


# ---- 2
def test_gradients_are_the_calls_they_are_defined_as(ops):
    n, m, rp, col = shape("hub_middle")
    drp, dcol = dev(rp, np.int32), dev(col, np.int32)
    plan = ops.csr_transpose_plan(drp, dcol, m)
    f32 = torch.float32
    val, X, G = _rand((len(col),), 6, f32), _rand((m, 16), 7, f32), _rand((n, 16), 8, f32, grad=False)
    ops.csr_spmm_autograd(drp, dcol, val, X, plan=plan).backward(G)
    assert same_bits(val.grad, ops.csr_sddmm(drp, dcol, G, X.detach()).cpu().numpy())
    assert same_bits(X.grad, ops.csr_spmm_t(plan, G, val.detach()).cpu().numpy())
    U, V, a = _rand((n, 16), 9, f32), _rand((m, 16), 10, f32), _rand((len(col),), 11, f32)
    g = _rand((len(col),), 12, f32, grad=False)
    ops.csr_sddmm_autograd(drp, dcol, U, V, val=a, plan=plan).backward(g)
    w = g * a.detach()
    assert same_bits(a.grad, ops.csr_sddmm(drp, dcol, U.detach(), V.detach(), val=g).cpu().numpy())
    assert same_bits(U.grad, ops.csr_spmm(drp, dcol, V.detach(), val=w).cpu().numpy())
    assert same_bits(V.grad, ops.csr_spmm_t(plan, U.detach(), val=w).cpu().numpy())
    U2, V2 = U.detach().clone().requires_grad_(), V.detach().clone().requires_grad_()
    ops.csr_sddmm_autograd(drp, dcol, U2, V2, plan=plan).backward(g)  # the pattern form: w = g
    assert same_bits(U2.grad, ops.csr_spmm(drp, dcol, V.detach(), val=g).cpu().numpy())
    assert same_bits(V2.grad, ops.csr_spmm_t(plan, U.detach(), val=g).cpu().numpy())


# ---- 3
def test_a_gradient_nobody_asks_for_is_not_computed(ops):
    n, m, rp, col = _small()
    drp, dcol = dev(rp, np.int32), dev(col, np.int32)
    empty = ops.TransposePlan(n, m, drp[:0], dcol[:0], drp[:0])  # csr_spmm_t raises on it: m + 1 offsets are missing
    val, X = _rand((len(col),), 13), _rand((m, 5), 14, grad=False)
    ops.csr_spmm_autograd(drp, dcol, val, X, plan=empty).sum().backward()  # dval alone: the plan is never touched
    assert val.grad is not None and X.grad is None
    with pytest.raises(ValueError):
        ops.csr_spmm_autograd(drp, dcol, val, X.clone().requires_grad_(), plan=empty).sum().backward()
    U, V = _rand((n, 5), 15), _rand((m, 5), 16, grad=False)
    ops.csr_sddmm_autograd(drp, dcol, U, V, val=val, plan=empty).sum().backward()  # dval and dU
    assert U.grad is not None and V.grad is None
    with pytest.raises(ValueError):
        ops.csr_sddmm_autograd(drp, dcol, U, V.clone().requires_grad_(), plan=empty).sum().backward()
    ops.profile_enable(True)
    try:
        X2 = _rand((m, 5), 17)
        before = ops.profile_report().get("spmm_t", (0, 0, 0))[1]
        ops.csr_spmm_autograd(drp, dcol, val.detach(), X2, plan=ops.csr_transpose_plan(drp, dcol, m)).sum().backward()
        torch.cuda.synchronize()
        after = ops.profile_report().get("spmm_t", (0, 0, 0))[1]
    finally:
        ops.profile_enable(False)
    assert after > before and X2.grad is not None  # (the transposed product ran, under its own kernel group)


# ---- 4
MARGIN = 4.0  # our error may be this many times the yardstick's: see the docstring of test_one_layer


def _torch_layer(rows, cols, n, m, Q, K, Vf, R):
    """The layer with gathers and index_add_ in the dtype of its operands: scores, a row softmax, attention x features."""
    z = (Q[rows] * K[cols]).sum(1)
    zmax = torch.full((n,), -float("inf"), dtype=z.dtype, device=z.device).scatter_reduce(0, rows, z, "amax")
    e = torch.exp(z - zmax[rows])
    s = e / torch.zeros(n, dtype=z.dtype, device=z.device).index_add_(0, rows, e)[rows]
    Y = torch.zeros((n, Vf.shape[1]), dtype=z.dtype, device=z.device).index_add_(0, rows, s[:, None] * Vf[cols])
    return (Y * R).sum()


def test_one_layer(ops):
    """The margin.  Both float32 computations round every product and sum to u = 2^-24 and differ in the order of their
    sums alone: ours adds a row's (a column's) products in runs of a span combined by a fixed tree, torch's index_add_ in
    whatever order its atomics land.  For sums of len terms either order is within gamma(len, u) of the exact sum, so
    neither can be said to be the more accurate; the two errors are of one magnitude and the ratio between them is noise
    of the order of a few units.  MARGIN = 4 allows ours to be four times the yardstick's; measured on an MI355X the
    largest relative errors are printed by this test and recorded in DESIGN §4.27."""
    n, m, rp, col = shape("power_law")
    d = 16
    drp, dcol = dev(rp, np.int32), dev(col, np.int32)
    rows, cols = dev(tr.rows_of(rp, len(col))), dev(col)
    plan = ops.csr_transpose_plan(drp, dcol, m)
    base = [_rand((n, d), 21, grad=False) * 0.5, _rand((m, d), 22, grad=False) * 0.5, _rand((m, d), 23, grad=False)]
    R = _rand((n, d), 24, grad=False)

    def grads(fn, dtype):
        ins = [t.to(dtype).clone().requires_grad_() for t in base]
        fn(*ins, R.to(dtype)).backward()
        return [t.grad.double() for t in ins]

    def ours(Q, K, Vf, Rr):
        z = ops.csr_sddmm_autograd(drp, dcol, Q, K, plan=plan)
        s = ops.csr_row_softmax_autograd(drp, z)
        return (ops.csr_spmm_autograd(drp, dcol, s, Vf, plan=plan) * Rr).sum()

    ref = lambda Q, K, Vf, Rr: _torch_layer(rows, cols, n, m, Q, K, Vf, Rr)
    g64 = grads(ref, torch.float64)
    g32 = grads(ref, torch.float32)
    got = grads(ours, torch.float32)
    for name, a, b, c in zip(("dQ", "dK", "dV"), g64, g32, got):
        scale = a.abs().max().item()
        yard, mine = (b - a).abs().max().item() / scale, (c - a).abs().max().item() / scale
        print(f"{name}: largest error / largest gradient: ours {mine:.3g}, torch float32 {yard:.3g}")
        assert scale > 0 and mine <= MARGIN * yard, (name, mine, yard)
