"""CPU restatements for the text writers (test infrastructure, no GPU, no library).

Two independent things, which tests/test_text_writers_host.py compares with each other and with the bytes recorded
from the real reference (tests/golden/text_writers.npz):

  1. the RULES of include/sbx_text.h restated in Python (format_values, format_coordinate, format_dense,
     symmetry_check, undirected_unique) and, on top of them, what the host-layer writers put into a file
     (mtx_file, array_file, edge_list_file): every check first, then banner, size line, text;
  2. a LITERAL TRANSCRIPTION of the reference's writers, loop for loop (ref_mtx_write_coo with its quadratic symmetry
     check, ref_mtx_write_array, ref_edge_list_write_coo), returning the bytes the file holds when the function
     returns or throws, and the exception's message.

Python's "%.*g" is correctly rounded and formats like glibc's except for the sign of a NaN ("nan" where glibc prints
"-nan"), which fmt() handles from the sign bit.
"""
import numpy as np

LOWER, NO_DIAGONAL, PATTERN = 1, 2, 4


def fmt(v, precision=6):
    """One value as `ostream << v` prints it (floats: printf("%.*g", precision, (double)v))."""
    if isinstance(v, (np.floating, float)):
        x = float(v)  # (a float32 widens exactly)
        if x != x:
            return "-nan" if np.signbit(v) else "nan"
        return "%.*g" % (precision, x)
    return str(int(v))


# ------------------------------------------------------------------------------------------ 1. the rules of sbx_text.h
def format_values(vals, precision=6):
    return "".join(fmt(v, precision) + "\n" for v in vals).encode()


def keep(r, c, flags):
    if flags & LOWER and c > r:
        return False
    if flags & NO_DIAGONAL and c == r:
        return False
    return True


def format_coordinate(row, col, val=None, index_base=1, precision=6, flags=0):
    out = []
    valued = val is not None and not flags & PATTERN
    for i in range(len(row)):
        r, c = int(row[i]), int(col[i])
        if not keep(r, c, flags):
            continue
        out.append(f"{r + index_base} {c + index_base}" + (" " + fmt(val[i], precision) if valued else "") + "\n")
    return "".join(out).encode()


def format_dense(n, m, row, col, val=None, precision=6):
    """n * m lines, column-major; ValueError for an id outside the matrix or a coordinate stored twice."""
    cells = {}
    for i in range(len(row)):
        r, c = int(row[i]), int(col[i])
        if not (0 <= r < n and 0 <= c < m):
            raise ValueError("range")
        if (r, c) in cells:
            raise ValueError("duplicate")
        cells[(r, c)] = i
    lines = []
    for c in range(m):
        for r in range(n):
            i = cells.get((r, c))
            lines.append("0" if i is None or val is None else fmt(val[i], precision))
    return "".join(x + "\n" for x in lines).encode()


def _neg(v):
    """-v as the C++ expression gives it for v's type (two's-complement wrap for the integers)."""
    if isinstance(v, np.integer):
        return (np.array(0, v.dtype) - np.array(v, v.dtype))[()]  # (arrays wrap silently)
    return -v


def symmetry_check(n, row, col, val=None, skew=False):
    """(all matched, diagonal entries, diagonal entries whose value is != 0), by a dictionary of the coordinates."""
    where = {}
    for i in range(len(row)):
        r, c = int(row[i]), int(col[i])
        if not (0 <= r < n and 0 <= c < n):
            raise ValueError("range")
        where.setdefault((r, c), []).append(i)
    ok, diag, diag_nz = True, 0, 0
    with np.errstate(over="ignore"):
        for i in range(len(row)):
            r, c = int(row[i]), int(col[i])
            if r == c:
                diag += 1
                if val is not None and val[i] != 0:
                    diag_nz += 1
                continue
            found = False
            for j in where.get((c, r), ()):
                if val is None:
                    found = not skew
                else:
                    found = bool(val[j] == (_neg(val[i]) if skew else val[i]))
                if found:
                    break
            ok = ok and found
    return ok, diag, diag_nz


def undirected_unique(row, col, val=None):
    """row <= col, stable sort by (row, col), the first of every run."""
    u = np.minimum(row, col)
    v = np.maximum(row, col)
    order = np.lexsort((v, u))  # (stable)
    u, v = u[order], v[order]
    w = None if val is None else np.asarray(val)[order]
    first = np.ones(len(u), bool)
    first[1:] = (u[1:] != u[:-1]) | (v[1:] != v[:-1])
    return u[first], v[first], (None if w is None else w[first])


# what the host layer writes: (file bytes, None) or (None, message) — a refused write leaves no file
def _option_checks(object_, format_, field, symmetry):
    if object_ not in ("matrix", "vector"):
        return "Illegal value for the 'object' option in matrix market header"
    if object_ == "vector":
        return "Matrix market writer does not currently support writing vectors."
    if format_ not in ("array", "coordinate"):
        return "Illegal value for the 'format' option in matrix market header"
    if field not in ("real", "double", "complex", "integer", "pattern"):
        return "Illegal value for the 'field' option in matrix market header"
    if symmetry not in ("general", "symmetric", "skew-symmetric", "hermitian"):
        return "Illegal value for the 'symmetry' option in matrix market header"
    if format_ == "array" and field == "pattern":
        return "Matrix market files with array format cannot have the field 'pattern' "
    if format_ == "array" and symmetry != "general":
        return "Matrix market files with array format cannot have the property 'symmetry' "
    if symmetry == "hermitian":
        return "Matrix market writer does not currently support hermitian symmetry."
    return None


def mtx_file(n, m, row, col, val, void_type=False, object_="matrix", format_="coordinate", field="real",
             symmetry="general", precision=6):
    """MTXWriter::WriteCOO of the host layer.  void_type: the ValueType is void (val is None then); a non-void type
    with val None compares coordinates only."""
    msg = _option_checks(object_, format_, field, symmetry)
    if msg:
        return None, msg
    if void_type and field != "pattern":
        return None, "Cannot write an MTX with void ValueType, unless field is pattern."
    said = symmetry in ("symmetric", "skew-symmetric")
    nnz = len(row)
    size_nnz = nnz
    if said:
        if n != m:
            return None, "Matrix is not symmetric!"
        skew = symmetry == "skew-symmetric"
        ok, diag, diag_nz = symmetry_check(n, row, col, None if void_type else val, skew)
        if not ok:
            return None, "Matrix is not symmetric!"
        if skew and diag_nz:
            return None, "Skew-symmetric matrix with non-zero diagonal values!"
        size_nnz = nnz - (nnz - diag) // 2 - (diag if skew else 0)
    banner = f"%%MatrixMarket {object_} {format_} {field} {symmetry}\n".encode()
    if format_ == "array":
        return banner + f"{n} {m}\n".encode() + format_dense(n, m, row, col, None if void_type else val, precision), None
    flags = (PATTERN if field == "pattern" else 0)
    if said:
        flags |= LOWER | (NO_DIAGONAL if symmetry == "skew-symmetric" else 0)
    return banner + f"{n} {m} {size_nnz}\n".encode() + format_coordinate(row, col, val, 1, precision, flags), None


def array_file(vals, void_type=False, object_="matrix", format_="array", field="real", symmetry="general", precision=6):
    msg = _option_checks(object_, format_, field, symmetry)
    if msg:
        return None, msg
    if format_ == "coordinate":
        return None, "Matrix market writer does not currently support writing array as coordinate."
    if void_type:
        return None, "Cannot write an MTX with void ValueType"
    return (f"%%MatrixMarket {object_} {format_} {field} {symmetry}\n1 {len(vals)}\n".encode()
            + format_values(vals, precision)), None


def edge_list_file(row, col, val=None, directed=True, precision=6):
    if not directed:
        row, col, val = undirected_unique(np.asarray(row), np.asarray(col), val)
    return format_coordinate(row, col, val, 0, precision, 0)


# ------------------------------------------------------------------- 2. the reference's writers, transcribed literally
class _Throw(Exception):
    pass


def ref_mtx_write_coo(n, m, row, col, val, void_type=False, object_="matrix", format_="coordinate", field="real",
                      symmetry="general"):
    """io/mtx_writer.cc:29-354.  Returns (the file's bytes or None if it was never opened, message or None)."""
    f = None
    try:
        msg = _option_checks(object_, format_, field, symmetry)  # :38-69, the same chain of ifs
        if msg:
            raise _Throw(msg)
        f = []
        f.append(f"%%MatrixMarket {object_} {format_} {field} {symmetry}\n")
        if void_type:
            if field != "pattern":
                raise _Throw("Cannot write an MTX with void ValueType, unless field is pattern.")
        dimensions = (n, m)
        said = symmetry in ("symmetric", "skew-symmetric", "hermitian")
        num_nnz = len(row)
        NNZ = num_nnz
        count_symmetric = 0
        count_diagonal = 0
        is_diagonal_all_zero = True
        if said and dimensions[0] != dimensions[1]:
            raise _Throw("Matrix is not symmetric!")
        if said and dimensions[0] == dimensions[1]:
            with np.errstate(over="ignore"):
                for i in range(num_nnz):
                    if row[i] != col[i]:
                        found_symmetric = False
                        for j in range(num_nnz):
                            if symmetry == "skew-symmetric":
                                if void_type:
                                    break
                                if row[j] == col[i] and col[j] == row[i] and val[j] == _neg(val[i]):
                                    found_symmetric = True
                                    count_symmetric += 1
                                    break
                            else:
                                if void_type:
                                    if row[j] == col[i] and col[j] == row[i]:
                                        found_symmetric = True
                                        count_symmetric += 1
                                        break
                                else:
                                    if row[j] == col[i] and col[j] == row[i] and val[j] == val[i]:
                                        found_symmetric = True
                                        count_symmetric += 1
                                        break
                        if not found_symmetric:
                            raise _Throw("Matrix is not symmetric!")
                    else:
                        count_diagonal += 1
                        if not void_type:
                            if val[i] != 0:
                                is_diagonal_all_zero = False
            if symmetry == "skew-symmetric":
                if not is_diagonal_all_zero:
                    raise _Throw("Skew-symmetric matrix with non-zero diagonal values!")
                NNZ -= (count_symmetric // 2) + count_diagonal
            else:
                NNZ -= count_symmetric // 2
        if format_ == "array":
            f.append(f"{dimensions[0]} {dimensions[1]}\n")
        else:
            f.append(f"{dimensions[0]} {dimensions[1]} {NNZ}\n")
        if format_ == "array":
            if void_type:
                index = 0
                while index < dimensions[0] * dimensions[1]:
                    f.append("0\n")
                    index += 1
            else:
                sort_vec = sorted(((int(col[i]), int(row[i]), i) for i in range(num_nnz)), key=lambda t: (t[0], t[1]))
                index = 0
                for c, r, i in sort_vec:
                    current_index = c * dimensions[0] + r
                    while index < current_index:
                        f.append("0\n")
                        index += 1
                    f.append(fmt(val[i]) + "\n")
                    index += 1
                while index < dimensions[0] * dimensions[1]:
                    f.append("0\n")
                    index += 1
        else:
            def line(i):
                f.append(f"{int(row[i]) + 1} {int(col[i]) + 1}")
                if void_type:
                    if field == "pattern":
                        f.append("\n")
                else:
                    if field == "pattern":
                        f.append("\n")
                    else:
                        f.append(" " + fmt(val[i]) + "\n")
            if said:
                for i in range(num_nnz):
                    if symmetry != "skew-symmetric" and col[i] == row[i]:
                        line(i)
                    if col[i] < row[i]:
                        line(i)
            else:
                for i in range(num_nnz):
                    line(i)
        return "".join(f).encode(), None
    except _Throw as e:
        return (None if f is None else "".join(f).encode()), str(e)


def ref_mtx_write_array(vals, void_type=False, object_="matrix", format_="array", field="real", symmetry="general"):
    """io/mtx_writer.cc:356-423."""
    f = None
    try:
        msg = _option_checks(object_, format_, field, symmetry)
        if msg:
            raise _Throw(msg)
        if format_ == "coordinate":
            raise _Throw("Matrix market writer does not currently support writing array as coordinate.")
        f = [f"%%MatrixMarket {object_} {format_} {field} {symmetry}\n"]
        if void_type:
            raise _Throw("Cannot write an MTX with void ValueType")
        f.append(f"1 {len(vals)}\n")
        for i in range(len(vals)):
            f.append(fmt(vals[i]) + "\n")
        return "".join(f).encode(), None
    except _Throw as e:
        return (None if f is None else "".join(f).encode()), str(e)


def ref_edge_list_write_coo(row, col, val=None, directed=True):
    """io/edge_list_writer.cc:18-101 (Python's sort is stable where std::sort leaves the order of equal keys open: the
    cases that use this hold no duplicate whose surviving weight would differ)."""
    edges = []
    for i in range(len(row)):
        u, v = int(row[i]), int(col[i])
        if not directed and u > v:
            u, v = v, u
        edges.append((u, v, None if val is None else val[i]))
    if not directed:
        edges.sort(key=lambda t: (t[0], t[1]))
        uniq = []
        for e in edges:
            if not uniq or (uniq[-1][0], uniq[-1][1]) != (e[0], e[1]):
                uniq.append(e)
        edges = uniq
    return "".join(f"{u} {v}" + ("" if val is None else " " + fmt(w)) + "\n" for u, v, w in edges).encode()
