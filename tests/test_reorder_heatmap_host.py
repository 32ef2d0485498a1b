"""ReorderHeatmap's rule, checked on the CPU (no GPU): a numpy restatement of sbx_csr_reorder_heatmap (include/sbx.h),
a literal transcription of the reference (reorder/reorder_heatmap.cc:43-119), the reference tests' two 3 x 3 known
answers, the outputs recorded from the real reference (tests/golden/boba_heatmap.npz), and the equalities between
them, bit for bit."""
import numpy as np
import pytest

from test_boba_host import GOLDEN, random_messy_coo


class HeatmapBadArgs(Exception):
    pass


def heatmap(rp, col, order_r, order_c, b, m=None):
    """heat[bu * b + bv] = float32(count) / float32(nnz), bu / bv the clamped blocks of order_r[i] / order_c[c]."""
    rp = np.asarray(rp, np.int64)
    col = np.asarray(col, np.int64)
    n = len(rp) - 1
    m = n if m is None else int(m)
    if b < 1 or b > n or b > m:
        raise HeatmapBadArgs(b)
    bsize = n // b
    order_r = np.asarray(order_r, np.int64)
    order_c = np.asarray(order_c, np.int64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    bu = np.minimum(order_r[rows] // bsize, b - 1)
    bv = np.minimum(order_c[col] // bsize, b - 1)
    cnt = np.bincount(bu * b + bv, minlength=b * b)
    with np.errstate(invalid="ignore", divide="ignore"):
        return cnt.astype(np.float32) / np.float32(rp[n])


def reference_heatmap(rp, col, order_r, order_c, b, m):
    """reorder_heatmap.cc:55-118 line by line (the discarded bandwidth statistics left out)."""
    n = len(rp) - 1
    if b > n or b > m:
        raise HeatmapBadArgs(b)
    bsize = n // b
    density = [[0] * b for _ in range(b)]
    for i in range(n):
        u = int(order_r[i])
        bu = u // bsize
        if bu >= b:
            bu = b - 1
        for ptr in range(int(rp[i]), int(rp[i + 1])):
            v = int(order_c[int(col[ptr])])
            bv = v // bsize
            if bv >= b:
                bv = b - 1
            density[bu][bv] += 1
    out = np.zeros(b * b, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(b):
            for j in range(b):
                out[i * b + j] = np.float32(density[i][j]) / (np.float32(rp[n]) + np.float32(0.0))
    return out


def csr_of(row, col, n):
    """Row-sorted CSR of a COO (rows below n), entries of a row in their stored order."""
    row = np.asarray(row, np.int64)
    col = np.asarray(col, np.int64)
    o = np.argsort(row, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, row + 1, 1)
    return np.cumsum(rp), col[o]


def degree_order(rp):
    """inv[old] = new for rows by ascending degree, ties by id (a simple, deterministic order)."""
    deg = np.diff(np.asarray(rp, np.int64))
    o = np.lexsort((np.arange(len(deg)), deg))
    inv = np.empty(len(deg), np.int64)
    inv[o] = np.arange(len(deg))
    return inv


def orders_for(rp, col, n, m, seed):
    """(name, order_r, order_c) triples: identity, degree (columns by the identity past row n) and random."""
    g = np.random.default_rng(seed)
    dr = degree_order(rp)
    dc = np.concatenate([dr, np.arange(len(dr), m)]) if m > len(dr) else dr[:m]
    return [("identity", np.arange(n), np.arange(m)), ("degree", dr, dc), ("random", g.permutation(n), g.permutation(m))]


def heat_shape(row, col, n, m):
    """The heatmap's CSR shape for a recorded COO: rows and columns past (n, m) widen it."""
    hn = max(n, int(np.max(row)) + 1 if len(row) else 0)
    hm = max(m, int(np.max(col)) + 1 if len(col) else 0)
    return hn, hm


def golden_heatmaps():
    z = np.load(GOLDEN)
    for name in z["names"].tolist():
        for oname in ("identity", "degree", "random"):
            key = "%s/heat/%s" % (name, oname)
            if key + "/bs" not in z:
                continue
            row, col = z[name + "/row"], z[name + "/col"]
            n, m = z[name + "/shape"].tolist()
            hn, hm = heat_shape(row, col, n, m)
            rp, ccol = csr_of(row, col, hn)
            vals = z[key + "/vals"]
            off = 0
            for b in z[key + "/bs"].tolist():
                yield name, oname, rp, ccol, hm, z[key + "/order_r"], z[key + "/order_c"], b, vals[off:off + b * b]
                off += b * b


# functionality_common.inc: n = 3, rows {0: 1 2, 1: 0, 2: 0}; heatmap_no_order_true / heatmap_rc_order_true
RP3, COL3 = [0, 2, 3, 4], [1, 2, 0, 0]
NO_ORDER_TRUE = [0, 0.25, 0.25, 0.25, 0, 0, 0.25, 0, 0]
R_REORDER, C_REORDER = [1, 2, 0], [2, 0, 1]
RC_ORDER_TRUE = [0, 0, 0.25, 0.25, 0.25, 0, 0, 0, 0.25]


def test_reference_known_answers():
    assert heatmap(RP3, COL3, [0, 1, 2], [0, 1, 2], 3).tolist() == NO_ORDER_TRUE
    assert heatmap(RP3, COL3, R_REORDER, C_REORDER, 3).tolist() == RC_ORDER_TRUE
    assert reference_heatmap(RP3, COL3, R_REORDER, C_REORDER, 3, 3).tolist() == RC_ORDER_TRUE


def test_restatement_and_transcription_equal_the_recorded_reference():
    count = 0
    for name, oname, rp, col, m, orr, orc, b, want in golden_heatmaps():
        got = heatmap(rp, col, orr, orc, b, m)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or (
            np.isnan(want).all() and np.isnan(got).all()), (name, oname, b)
        ref = reference_heatmap(rp, col, orr, orc, b, m)
        assert np.array_equal(ref, got, equal_nan=True), (name, oname, b)
        count += 1
    assert count >= 150


@pytest.mark.parametrize("seed", range(4))
def test_restatement_equals_transcription_on_random_cases(seed):
    g = np.random.default_rng(300 + seed)
    for trial in range(600):
        n = int(g.integers(1, 30))
        m = int(g.integers(1, 30))
        row, col = random_messy_coo(g, n, n, int(g.integers(0, 4 * n + 2)))
        col = col % m
        rp, ccol = csr_of(row, col, n)
        orr = g.integers(0, 2 * n, n) if trial % 4 == 0 else g.permutation(n)  # positions past n clamp
        orc = g.integers(0, 2 * m, m) if trial % 4 == 1 else g.permutation(m)
        b = int(g.integers(1, min(n, m) + 1))
        want = reference_heatmap(rp, ccol, orr, orc, b, m)
        assert np.array_equal(heatmap(rp, ccol, orr, orc, b, m), want, equal_nan=True), (n, m, b)


def test_bad_num_parts():
    for b in (0, -1, 4):
        with pytest.raises(HeatmapBadArgs):
            heatmap(RP3, COL3, [0, 1, 2], [0, 1, 2], b)
    with pytest.raises(HeatmapBadArgs):
        heatmap(RP3, COL3, [0, 1, 2], [0, 1], 3, m=2)


def test_empty_matrix_is_nan():
    assert np.isnan(heatmap([0, 0, 0], [], [0, 1], [0, 1], 2)).all()
