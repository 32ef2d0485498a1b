"""CPU tests of the text writers' two Python statements (tests/text_restate.py): the restatement of the rules of
include/sbx_text.h with the host layer's file composition on top, and the literal transcription of the reference's
MTXWriter / EdgeListWriter — both against the bytes and messages recorded from the real reference
(tests/golden/text_writers.npz, tools/make_text_writers_golden.py), and against each other on random small inputs."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_restate as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "text_writers.npz")


def golden_cases():
    z = np.load(GOLDEN)
    for k, case in enumerate(json.loads(z["cases"].tobytes().decode())):
        arrays = {name: (z[f"{name}_{k}"] if f"{name}_{k}" in z.files else None) for name in ("row", "col", "val")}
        yield case, arrays, (z[f"file_{k}"].tobytes() if case["file_left"] else None)


def both(case, a):
    """(restatement, transcription) of one case: each (bytes or None, message or None)."""
    void = case["vtype"] == "void"
    if case["kind"] == "array":
        opts = dict(object_=case["object"], format_=case["format"], field=case["field"], symmetry=case["symmetry"])
        vals = [] if a["val"] is None else a["val"]
        return tr.array_file(vals, void, **opts), tr.ref_mtx_write_array(vals, void, **opts)
    if case["kind"] == "edges":
        return ((tr.edge_list_file(a["row"], a["col"], a["val"], case["directed"]), None),
                (tr.ref_edge_list_write_coo(a["row"], a["col"], a["val"], case["directed"]), None))
    opts = dict(object_=case["object"], format_=case["format"], field=case["field"], symmetry=case["symmetry"])
    return (tr.mtx_file(case["n"], case["m"], a["row"], a["col"], a["val"], void, **opts),
            tr.ref_mtx_write_coo(case["n"], case["m"], a["row"], a["col"], a["val"], void, **opts))


def test_golden_file_is_small_and_covers_the_ground():
    assert os.path.getsize(GOLDEN) < 100_000
    cases = [c for c, _, _ in golden_cases()]
    assert len(cases) >= 20
    mtx = [c for c in cases if c["kind"] == "mtx" and not c["message"]]
    assert {c["symmetry"] for c in mtx} == {"general", "symmetric", "skew-symmetric"}
    assert {c["format"] for c in mtx} == {"coordinate", "array"} and any(c["field"] == "pattern" for c in mtx)
    assert {c["vtype"] for c in cases} == {"void", "int", "float", "double"}
    assert any(c["kind"] == "array" and not c["message"] for c in cases)
    edges = [c for c in cases if c["kind"] == "edges"]
    assert {c["directed"] for c in edges} == {True, False}
    messages = {c["message"] for c in cases if c["message"]}
    assert len(messages) == 13  # every distinct message mtx_writer.cc throws (:38-69, :83-85, :109-112, :166, :192, :394-397, :409)


def test_transcription_and_restatement_against_the_recorded_reference():
    for case, a, left in golden_cases():
        (r_bytes, r_msg), (t_bytes, t_msg) = both(case, a)
        want_msg = case["message"] or None
        # the transcription: the reference to the byte, the file it leaves behind a throw included
        assert t_msg == want_msg, (case, t_msg)
        assert t_bytes == left, (case, t_bytes, left)
        # the restatement: the same message; the same file when there is no refusal, no file when there is one
        assert r_msg == want_msg, (case, r_msg)
        assert r_bytes == (None if want_msg else left), (case, r_bytes, left)


def _random_case(g):
    vtype = ["void", "int", "float", "double"][g.integers(0, 4)]
    dt = {"void": None, "int": np.int32, "float": np.float32, "double": np.float64}[vtype]
    n = int(g.integers(1, 7))
    m = n if g.random() < 0.7 else int(g.integers(1, 7))
    sym = ["general", "symmetric", "skew-symmetric", "hermitian", "odd"][g.choice(5, p=[0.3, 0.3, 0.3, 0.05, 0.05])]
    fmt = ["coordinate", "array", "odd"][g.choice(3, p=[0.75, 0.2, 0.05])]
    field = ["real", "integer", "pattern", "odd"][g.choice(4, p=[0.5, 0.15, 0.3, 0.05])]
    obj = ["matrix", "vector", "odd"][g.choice(3, p=[0.9, 0.05, 0.05])]
    nnz = int(g.integers(0, 12))
    if fmt == "array":  # (no duplicate coordinate: the reference misaligns its lines behind one, the library refuses it)
        cells = g.choice(n * m, min(nnz, n * m), replace=False)
        row, col = cells % n, cells // n
    else:
        row, col = g.integers(0, n, nnz), g.integers(0, m, nnz)
        if sym in ("symmetric", "skew-symmetric") and n == m and g.random() < 0.8:  # mostly (skew-)symmetric for real
            row, col = np.concatenate([row, col]), np.concatenate([col, row])
    val = None
    if dt is not None:
        half = (g.integers(-3, 4, len(row)) * (0.5 if dt != np.int32 else 1)).astype(dt)
        if fmt != "array" and len(row) and sym in ("symmetric", "skew-symmetric") and len(row) % 2 == 0:
            h = len(row) // 2
            half[h:] = -half[:h] if sym == "skew-symmetric" else half[:h]
            if sym == "skew-symmetric" and g.random() < 0.7:
                half[row == col] = 0
        val = half
    case = dict(kind="mtx", vtype=vtype, n=n, m=m, object=obj, format=fmt, field=field, symmetry=sym)
    return case, dict(row=row.astype(np.int32), col=col.astype(np.int32), val=val)


def test_restatement_equals_transcription_on_random_small_inputs():
    g = np.random.default_rng(5)
    outcomes = {}
    for _ in range(3000):
        case, a = _random_case(g)
        (r_bytes, r_msg), (t_bytes, t_msg) = both(case, a)
        assert r_msg == t_msg, (case, a, r_msg, t_msg)
        if t_msg is None:
            assert r_bytes == t_bytes, (case, a)
        else:
            assert r_bytes is None
        outcomes[t_msg] = outcomes.get(t_msg, 0) + 1
    assert outcomes.get(None, 0) > 500 and len(outcomes) >= 10, outcomes
    # edge lists: directed with anything; undirected where no surviving weight is ambiguous (weights equal per pair)
    for _ in range(500):
        nnz = int(g.integers(0, 30))
        row, col = g.integers(0, 6, nnz), g.integers(0, 6, nnz)
        directed = bool(g.integers(0, 2))
        val = [None, (np.minimum(row, col) * 10 + np.maximum(row, col)).astype(np.float32) / 4][g.integers(0, 2)]
        assert tr.edge_list_file(row, col, val, directed) == tr.ref_edge_list_write_coo(row, col, val, directed)
    # WriteArray
    for opts in (dict(), dict(format_="coordinate"), dict(symmetry="symmetric"), dict(object_="vector"), dict(field="pattern")):
        vals = (g.integers(-50, 50, 9) / 8).astype(np.float64)
        r, t = tr.array_file(vals, False, **opts), tr.ref_mtx_write_array(vals, False, **opts)
        assert r[1] == t[1] and (t[1] is not None or r[0] == t[0])


def test_nan_sign_and_the_format_rules():
    assert tr.fmt(np.float32("nan")) == "nan" and tr.fmt(-np.float64("nan")) == "-nan"
    assert [tr.fmt(x) for x in (0.5, 2.5, 1000005.0, 999999.5, 1e-5, 0.0001, 100000.0, 1e6, -0.0)] == \
        ["0.5", "2.5", "1e+06", "1e+06", "1e-05", "0.0001", "100000", "1e+06", "-0"]
    assert tr.fmt(np.float32(0.1), 9) == "0.100000001" and tr.fmt(0.1, 17) == "0.10000000000000001"
