"""CPU restatements of include/sbx_stats.h and of the host layer's degree-statistic features, checked against the
reference's own test vectors and against tests/golden/degree_stats.npz: the outputs of the real reference's feature
classes (float and double) over 36 offset arrays and four CSRs (NOTES.md has the fixture's provenance).  The GPU tests
import the restatements from here.

Bit-identical to the reference: Avg, Min, Max, Median, OffDiagBlockNNZ.  Not bit-identical, by construction (the
reference accumulates in F, row after row): StandardDeviation, CoefficientOfVariation, GeometricAvg.  How near the
reference must sit, with u = 2^-24 (float) or 2^-53 (double), n degrees below 2^24 (so F(d) is exact), avg = sum / n
and T the exact sum of squared deviations:

  sum of squared deviations, compared in the square:  |ref^2 - T| <= (n + 8) u T + 2 n u^2 avg^2.
    The reference's average is avg (1 + e0), |e0| <= u.  sum (d_i - avg - avg e0)^2 = T + n avg^2 e0^2, because the
    deviations sum to zero: the first-order effect of the rounded average cancels and n u^2 avg^2 remains.  Each term
    takes one rounding in the subtraction (squared: 2u) and one in the product; the sequential sum of n non-negative
    terms adds at most (n - 1) u to each; the square root adds u, 2u in the square: (n + 4) u in all.  The four
    further u and the doubled second term cover what is of second order in u for the n of the fixture.
  coefficient of variation: the same bound, widened by 3u relative (the rounded average in the divisor, the division,
    and one more for second-order terms).
  geometric average: relative error <= (ln(G) (n + 2) + 4) u with G the exact value.
    The n additions of non-negative logarithms give the sum a relative error of at most n u, the division by n one
    more u; a relative error e of the exponent (ln G) multiplies the result by exp(ln(G) e).  exp and the final
    rounding add 2u.  (ln(G) (n + 1) + 2) u in all, the rest covers the second order.

The values this project computes come from exact integers through correctly rounded operations; their own distance
from the exact value is at most 4u in the square (N -> double, the division, the square root twice, the cast to F)
and (ln(G) (n + 3) + 3) 2^-53 + u for the geometric average.
"""
import math
import os
import re
from decimal import Decimal, getcontext
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "degree_stats.npz")
U = {np.float32: Fraction(1, 2 ** 24), np.float64: Fraction(1, 2 ** 53)}
getcontext().prec = 60


# ---- include/sbx_stats.h, restated in Python ints ----------------------------------------------------------------------
def degree_stats(ptr):
    """Every field of sbxstat_degrees for the offset array `ptr`, `sumsq` as one int; sum_log by math.fsum."""
    p = [int(x) for x in np.asarray(ptr).tolist()]
    n = len(p) - 1
    d = [p[i + 1] - p[i] for i in range(n)]
    s = sorted(d)
    return {"count": n, "sum": p[n] - p[0], "min": min(d), "max": max(d), "zeros": sum(1 for x in d if x == 0),
            "sumsq": sum(x * x for x in d), "median_lo": s[(n - 1) // 2], "median_hi": s[n // 2],
            "sum_log": math.fsum(math.log(x) for x in d if x > 0)}


def off_diag(rp, col, n, m, h, w):
    """off_diag_block_nnz.cc:94-116 with every product in Python ints; None where the reference divides by zero."""
    rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int64)
    if h <= 0:
        return 0
    if w <= 0:
        return None
    cnt = 0
    for p in range(min(h, n)):  # (block p starts at row min(n, p (n / h) + min(p, n % h)) >= min(n, p): empty from p = n on)
        rs, re_ = min(n, p * (n // h) + min(p, n % h)), min(n, (p + 1) * (n // h) + min(p + 1, n % h))
        cs, ce = min(m, p * (m // w) + min(p, m % w)), min(m, (p + 1) * (m // w) + min(p + 1, m % w))
        seg = col[rp[rs]:rp[re_]]  # (the rows of a block are contiguous, so are their entries)
        cnt += int(np.count_nonzero((seg < cs) | (seg >= ce)))
    return cnt


# ---- the host layer's values (feature/degree_stats.h), the same operations in the same order --------------------------
def squared_deviations(st):
    """(N, T): N = n sumsq - sum^2 exactly, T = (double)N / (double)n."""
    n = st["count"]
    if n * st["sumsq"] >= 2 ** 127:
        raise OverflowError("n * sumsq does not fit 127 bits")
    N = n * st["sumsq"] - st["sum"] ** 2
    return N, float(N) / float(n)


def feature_values(st, F):
    n = st["count"]
    out = {"avg": F(st["sum"]) / F(n), "min": st["min"], "max": st["max"]}
    if n % 2 == 0:
        out["median"] = F(float(F(st["median_lo"] + st["median_hi"])) / 2.0)
    else:
        out["median"] = F(st["median_hi"])
    _, T = squared_deviations(st)
    out["standard_deviation"] = F(math.sqrt(T))
    mean = float(st["sum"]) / float(n)
    out["coefficient_of_variation"] = F(math.sqrt(T) / mean) if mean else F("nan")  # (0 / 0 in C++)
    out["geometric_avg"] = F(0) if st["zeros"] > 0 else F(math.exp(st["sum_log"] / float(n)))
    return out


# ---- what the reference computes (feature/*_degree_column.cc): sequential sums in F ----------------------------------
def reference_values(ptr, F):
    p = np.asarray(ptr, np.int64)
    n = len(p) - 1
    d = np.diff(p)
    with np.errstate(all="ignore"):
        avg = F(int(p[n] - p[0])) / F(n)
        dev = d.astype(F) - avg  # (cols[i + 1] - cols[i] - avg_degree: the integer converts to F)
        ssq = np.cumsum(dev * dev, dtype=F)[-1]  # (np.cumsum adds one after the other, as the loop does)
        root = F(math.sqrt(float(ssq)))  # (sqrt(double) rounded to F: correctly rounded either way)
        s = F(0)
        for x in d.tolist():  # sum += log(degree): log in double, the addition in double, the sum rounded to F
            s = F(float(s) + (math.log(x) if x > 0 else -math.inf))
        geo = F(math.exp(float(s / F(n))))
        sd = np.sort(d)
        med = F(float(F(int(sd[n // 2 - 1] + sd[n // 2]))) / 2.0) if n % 2 == 0 else F(int(sd[n // 2]))
        return {"avg": avg, "min": int(d.min()), "max": int(d.max()), "median": med, "standard_deviation": root,
                # sqrt(F) / F: the C sqrt(double), so the quotient is taken in double and rounded to F once
                "coefficient_of_variation": F(np.float64(math.sqrt(float(ssq))) / np.float64(avg)), "geometric_avg": geo}


# ---- bounds ------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _ln(x):
    return Decimal(x).ln()


def exact_geometric(ptr):
    d = np.diff(np.asarray(ptr, np.int64)).tolist()
    if min(d) == 0:
        return None
    return (sum(_ln(x) for x in d) / len(d)).exp()


def squared_deviation_bound(st, F, extra=0):
    """(T, allowed): |value^2 - T| <= allowed, `extra` further u of relative error in the square."""
    n, u = st["count"], U[F]
    T = Fraction(st["count"] * st["sumsq"] - st["sum"] ** 2, n)
    avg = Fraction(st["sum"], n)
    return T, (n + 8 + extra) * u * T + 2 * n * u * u * avg * avg


def geometric_bound(G, n, F):
    return (G.ln() * (n + 2) + 4) * Decimal(U[F].numerator) / Decimal(U[F].denominator)


# ---- fixtures ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    names = [str(x) for x in g["names"]]
    ff, fi = [str(x) for x in g["float_fields"]], [str(x) for x in g["int_fields"]]
    cases = []
    for i, name in enumerate(names):
        ptr = g[f"ptr_{i}"]
        ref = {np.float32: dict(zip(ff, g["ref_f32"][i])), np.float64: dict(zip(ff, g["ref_f64"][i]))}
        cases.append((name, ptr, ref, dict(zip(fi, (int(x) for x in g["ref_int"][i]))), degree_stats(ptr)))
    od = [tuple(g[f"od_{i}_{k}"] for k in ("n", "m", "row_ptr", "col", "hw", "ref")) for i in range(int(g["od_count"]))]
    return cases, od


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b))


# ---- the reference's own test vectors, as data -----------------------------------------------------------------------------
REF_ROW_PTR, REF_COL = [0, 2, 2, 5, 7, 9, 11, 12], [2, 3, 0, 3, 4, 0, 2, 2, 5, 4, 6, 5]  # off_diag_block_nnz_tests.cc


def test_reference_test_vectors():
    assert off_diag(REF_ROW_PTR, REF_COL, 7, 7, 3, 3) == 8
    # functionality_common.inc: col_ptr = row_ptr = {0, 2, 3, 4}; the feature tests compute their expectations from it
    st = degree_stats([0, 2, 3, 4])
    assert (st["count"], st["sum"], st["min"], st["max"], st["zeros"], st["sumsq"]) == (3, 4, 1, 2, 0, 6)
    assert (st["median_lo"], st["median_hi"]) == (1, 1)
    v = feature_values(st, np.float32)
    assert v["avg"] == np.float32(4) / np.float32(3) and v["min"] == 1 and v["max"] == 2 and v["median"] == 1.0
    assert abs(float(v["standard_deviation"]) - math.sqrt(6 / 9)) < 1e-6  # (the reference's EXPECT_NEAR tolerance)
    assert abs(float(v["coefficient_of_variation"]) - math.sqrt(6 / 9) / (4 / 3)) < 1e-6
    assert abs(float(v["geometric_avg"]) - 2 ** (1 / 3)) < 1e-6


def test_restated_reference_agrees_with_the_compiled_one(golden):
    cases, _ = golden
    for name, ptr, ref, ref_int, _ in cases:
        assert ref_int["min"] == ref_int["min_column"] == ref_int["min_max_avg_min"]
        assert ref_int["max"] == ref_int["max_column"] == ref_int["min_max_avg_max"]
        for F in (np.float32, np.float64):
            r, want = reference_values(ptr, F), ref[F]
            assert r["min"] == ref_int["min"] and r["max"] == ref_int["max"], name
            assert same_bits(r["avg"], F(want["avg_column"])) and same_bits(r["avg"], F(want["avg"])), name
            assert same_bits(r["avg"], F(want["min_max_avg_avg"])), name
            assert same_bits(r["median"], F(want["median_column"])), name
            assert same_bits(r["standard_deviation"], F(want["standard_deviation_column"])), name
            assert same_bits(r["coefficient_of_variation"], F(want["coefficient_of_variation_column"])), name
            # log and exp are the C library's, which is not correctly rounded: an ulp or two between two versions of it
            got, w = float(r["geometric_avg"]), float(want["geometric_avg_column"])
            assert abs(got - w) <= 4 * float(np.spacing(F(w))), name


def test_bit_identical_features_equal_the_reference(golden):
    cases, od = golden
    for name, ptr, ref, ref_int, st in cases:
        assert st["min"] == ref_int["min_column"] == ref_int["min"] and st["max"] == ref_int["max_column"] == ref_int["max"]
        for F in (np.float32, np.float64):
            v = feature_values(st, F)
            assert same_bits(v["avg"], F(ref[F]["avg_column"])) and same_bits(v["avg"], F(ref[F]["avg"])), name
            assert same_bits(v["median"], F(ref[F]["median_column"])), name
    for n, m, rp, col, hw, want in od:
        for (h, w), r in zip(hw.tolist(), want.tolist()):
            got = off_diag(rp, col, int(n), int(m), h, w)
            assert (got is None and r == -1) or np.int32(got) == r, (int(n), int(m), h, w)  # (the reference counts in IDType)


def test_reference_and_this_project_sit_inside_the_derived_bounds(golden):
    cases, _ = golden
    for name, ptr, ref, _, st in cases:
        n = st["count"]
        assert st["max"] < 2 ** 24
        G = exact_geometric(ptr)
        for F in (np.float32, np.float64):
            u, v = U[F], feature_values(st, F)
            T, allowed = squared_deviation_bound(st, F)
            r = Fraction(float(ref[F]["standard_deviation_column"]))
            print(f"{name} {F.__name__}: std ref^2-T {float(r * r - T):.3e} allowed {float(allowed):.3e}")
            assert abs(r * r - T) <= allowed, name
            mine = Fraction(float(v["standard_deviation"]))
            assert abs(mine * mine - T) <= 4 * u * T, name
            assert abs(mine * mine - r * r) <= allowed + 4 * u * T, name
            if st["sum"]:
                avg = Fraction(st["sum"], n)
                for value, rel in ((ref[F]["coefficient_of_variation_column"], 3 * u), (v["coefficient_of_variation"], 0)):
                    X = (Fraction(float(value)) * avg) ** 2
                    slack = allowed if rel else 6 * u * T  # (this project's: 4u as above, one division and one cast more)
                    assert (T - slack) * (1 - rel) ** 2 <= X <= (T + slack) * (1 + rel) ** 2, name
            else:
                assert np.isnan(ref[F]["coefficient_of_variation_column"]) and np.isnan(v["coefficient_of_variation"])
            if G is None:
                assert ref[F]["geometric_avg_column"] == 0 and v["geometric_avg"] == 0, name
                continue
            bound = geometric_bound(G, n, F)
            rel_ref = abs(Decimal(float(ref[F]["geometric_avg_column"])) - G) / G
            print(f"{name} {F.__name__}: geo rel {float(rel_ref):.3e} bound {float(bound):.3e}")
            assert rel_ref <= bound, name
            mine_bound = (G.ln() * (n + 3) + 3) / Decimal(2 ** 53) + Decimal(u.numerator) / Decimal(u.denominator)
            rel_mine = abs(Decimal(float(v["geometric_avg"])) - G) / G
            assert rel_mine <= mine_bound, name  # (so the two values lie within bound + mine_bound of each other)


def test_large_degrees_carry_and_overflow():
    st = degree_stats([0, 2 ** 40, 2 ** 40 + 1, 2 ** 41 + 7])
    assert st["sumsq"] >> 64 and st["max"] == 2 ** 40 + 6
    assert feature_values(st, np.float64)["standard_deviation"] > 0
    big = {"count": 3, "sumsq": 2 ** 126, "sum": 2 ** 63 - 1}
    with pytest.raises(OverflowError):
        squared_deviations(big)


# ---- the header and the tables exist ---------------------------------------------------------------------------------------
def test_header_and_tables_exist():
    from sparsebase_amd import capi, ops
    text = open(os.path.join(ROOT, "include", "sbx_stats.h")).read()
    assert '#include "sbx.h"' in text and re.search(r"#define SBX_STATS_VERSION 100\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(sbxstat_[a-z0-9_]+)\s*\(", text))) == sorted(capi.STATS_PROTOTYPES)
    assert callable(ops.degree_stats) and callable(ops.csr_off_diag_block_nnz)
    import torch
    with pytest.raises(ValueError):
        ops.degree_stats(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.csr_off_diag_block_nnz(torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 3, 2)
