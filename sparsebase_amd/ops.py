"""Tensor-level plumbing over the C ABI (include/sbx.h, sbx_text.h, sbx_stats.h, sbio.h, sbgr.h, sbhg.h, sbfx.h, sbsym.h, sbmv.h, sbmm.h,
sbdd.h, sbsm.h, sbmt.h).

torch owns the device buffers and the stream; every function here only
marshals pointers into libsbx.so.  Nothing in this module computes on the CPU:
if the HIP library or a GPU is missing the calls raise.
"""
import ctypes as C
import threading
from typing import NamedTuple

import torch

from . import capi

_VT = {torch.int32: capi.V_I32, torch.float32: capi.V_F32, torch.int64: capi.V_I64,
       torch.float64: capi.V_F64}
_handles = {}
_lock = threading.Lock()


def _vt(val):
    if val is None:
        return capi.V_NONE
    if val.dtype not in _VT:
        raise TypeError(f"unsupported value dtype {val.dtype}")
    return _VT[val.dtype]


def _it(t, ids=None):
    """Index tuple of a call: `t` is the call's offset array where it has one (row_ptr / col_ptr), else an id array;
    `ids` an id array of the same call (col, row): int64 offsets over int32 ids are SBX_I32_N64."""
    if t.dtype == torch.int32:
        if ids is not None and ids.dtype != torch.int32:
            raise TypeError("32-bit offsets with 64-bit ids: not a tuple the library takes")
        return capi.SBX_I32
    if t.dtype == torch.int64:
        if ids is not None and ids.dtype == torch.int32:
            return capi.SBX_I32_N64
        return capi.SBX_I64
    raise TypeError(f"index tensors must be int32/int64, got {t.dtype}")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _check_dev(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError("sparsebase_amd.ops works on device tensors only (no CPU path)")
        if not t.is_contiguous():
            raise ValueError("tensors must be contiguous")
        dev = t.device if dev is None else dev
        if t.device != dev:
            raise ValueError("all tensors must live on the same device")
    return dev


class Handle:
    """One sbx handle per (device); bound to torch's current stream on every call."""

    def __init__(self, device_index):
        self.lib = capi.load()
        self.h = C.c_void_p()
        rc = self.lib.sbx_create(int(device_index), C.byref(self.h))
        if rc != capi.SBX_OK:
            raise capi.SbxError(rc, "sbx_create failed (HIP hot path has no CPU fallback)")
        self.device_index = device_index

    def bind_stream(self):
        s = torch.cuda.current_stream(self.device_index).cuda_stream
        self.check(self.lib.sbx_set_stream(self.h, C.c_void_p(s)))

    def check(self, rc):
        if rc != capi.SBX_OK:
            raise capi.SbxError(rc, self.lib.sbx_last_error(self.h).decode())

    def reserve(self, nbytes):
        self.check(self.lib.sbx_reserve(self.h, C.c_size_t(nbytes)))


def profile_enable(on=True, device=None):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    hd = handle_for(dev)
    hd.check(hd.lib.sbx_profile_enable(hd.h, int(bool(on))))


def profile_report(device=None):
    """{kernel group: (total_ms, launches)} accumulated since profile_enable(True)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    hd = handle_for(dev)
    out = {}
    for i in range(hd.lib.sbx_profile_kernel_count()):
        ms, cnt = C.c_double(0), C.c_int64(0)
        hd.check(hd.lib.sbx_profile_query(hd.h, i, C.byref(ms), C.byref(cnt)))
        nb = C.c_int64(0)
        hd.check(hd.lib.sbx_profile_query_bytes(hd.h, i, C.byref(nb)))
        if cnt.value:
            out[hd.lib.sbx_profile_kernel_name(i).decode()] = (ms.value, cnt.value, nb.value)
    return out


def handle_for(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    with _lock:
        if idx not in _handles:
            _handles[idx] = Handle(idx)
    hd = _handles[idx]
    hd.bind_stream()
    return hd


# ----------------------------------------------------------------------------- A1 / A4
def coo_is_sorted(row, col):
    hd = handle_for(_check_dev(row, col))
    out = C.c_int(0)
    hd.check(hd.lib.sbx_coo_is_sorted(hd.h, _it(row), row.numel(), _p(row), _p(col), C.byref(out)))
    return bool(out.value)


def coo_sort_(n, m, row, col, val=None):
    """In place, like the COO constructor (format/coo.cc:110-157)."""
    hd = handle_for(_check_dev(row, col, val))
    hd.check(hd.lib.sbx_coo_sort(hd.h, _it(row), _vt(val), n, m, row.numel(), _p(row), _p(col), _p(val)))


def csr_rows_sorted(row_ptr, col):
    hd = handle_for(_check_dev(row_ptr, col))
    out = C.c_int(0)
    hd.check(hd.lib.sbx_csr_rows_sorted(hd.h, _it(row_ptr, col), row_ptr.numel() - 1, _p(row_ptr), _p(col), C.byref(out)))
    return bool(out.value)


def csr_sort_rows_(n, m, row_ptr, col, val=None):
    """In place, like the CSR constructor (format/csr.cc:99-157)."""
    hd = handle_for(_check_dev(row_ptr, col, val))
    hd.check(hd.lib.sbx_csr_sort_rows(hd.h, _it(row_ptr, col), _vt(val), n, m, col.numel(), _p(row_ptr), _p(col), _p(val)))


# ----------------------------------------------------------------------------- A2 / A3
def coo_to_csr(n, m, row, col, val=None, move=False, rows_sorted=False, out=None, offset_dtype=None):
    """offset_dtype=torch.int64 with int32 ids: the <32-bit ids, 64-bit offsets> tuple (SBX_I32_N64)."""
    hd = handle_for(_check_dev(row, col, val))
    nnz = row.numel()
    if out is None:
        rp = torch.empty(n + 1, dtype=offset_dtype or row.dtype, device=row.device)
        co = None if move else torch.empty_like(col)
        vo = None if (move or val is None) else torch.empty_like(val)
    else:
        rp, co, vo = out
    flags = (capi.FLAG_MOVE if move else 0) | (capi.FLAG_ROWS_SORTED if rows_sorted else 0)
    hd.check(hd.lib.sbx_coo_to_csr(hd.h, _it(rp, row), _vt(val), n, m, nnz, _p(row), _p(col), _p(val), _p(rp), _p(co),
                                   _p(vo), flags))
    return (rp, col, val) if move else (rp, co, vo)


def csr_to_coo(n, m, row_ptr, col, val=None, move=False, out=None):
    hd = handle_for(_check_dev(row_ptr, col, val))
    nnz = col.numel()
    if out is None:
        ro = torch.empty(nnz, dtype=col.dtype if col is not None else row_ptr.dtype, device=row_ptr.device)
        co = None if move else torch.empty_like(col)
        vo = None if (move or val is None) else torch.empty_like(val)
    else:
        ro, co, vo = out
    flags = capi.FLAG_MOVE if move else 0
    hd.check(hd.lib.sbx_csr_to_coo(hd.h, _it(row_ptr, ro), _vt(val), n, m, nnz, _p(row_ptr), _p(col), _p(val), _p(ro),
                                   _p(co), _p(vo), flags))
    return (ro, col, val) if move else (ro, co, vo)


def coo_to_csc(n, m, row, col, val=None, offset_dtype=None):
    """COO -> CSC (col_ptr[m+1], row[nnz], val[nnz]); converter_order_two.cc:21-70."""
    hd = handle_for(_check_dev(row, col, val))
    nnz = col.numel()
    cp = torch.empty(m + 1, dtype=offset_dtype or row.dtype, device=row.device)
    ro = torch.empty_like(row)
    vo = None if val is None else torch.empty_like(val)
    hd.check(hd.lib.sbx_coo_to_csc(hd.h, _it(cp, row), _vt(val), n, m, nnz, _p(row), _p(col), _p(val), _p(cp), _p(ro), _p(vo)))
    return cp, ro, vo


def csr_to_csc(n, m, row_ptr, col, val=None):
    """CSR -> CSC (the transpose when rows are sorted); converter_order_two.cc:120-128."""
    hd = handle_for(_check_dev(row_ptr, col, val))
    nnz = col.numel()
    cp = torch.empty(m + 1, dtype=row_ptr.dtype, device=row_ptr.device)
    ro = torch.empty_like(col)
    vo = None if val is None else torch.empty_like(val)
    hd.check(hd.lib.sbx_csr_to_csc(hd.h, _it(row_ptr, col), _vt(val), n, m, nnz, _p(row_ptr), _p(col), _p(val), _p(cp),
                                   _p(ro), _p(vo)))
    return cp, ro, vo


# ----------------------------------------------------------------------------- Matrix Market ingest
def mtx_parse_coordinate(text, n_rows, n_cols, entries, fields, symmetry=0, zero_index=True, upper_triangle=False,
                         index_dtype=torch.int32, value_dtype=None):
    """text: uint8 device tensor with the bytes after the size line.  Returns (row, col, val) trimmed to nnz."""
    hd = handle_for(_check_dev(text))
    expand = symmetry != 0 and not upper_triangle
    cap = max(1, entries * (2 if expand else 1))
    row = torch.empty(cap, dtype=index_dtype, device=text.device)
    col = torch.empty(cap, dtype=index_dtype, device=text.device)
    val = None if (value_dtype is None or fields != 3) else torch.empty(cap, dtype=value_dtype, device=text.device)
    nnz = C.c_int64(0)
    flags = (1 if zero_index else 0) | (2 if upper_triangle else 0)
    hd.check(hd.lib.sbx_mtx_parse_coordinate(hd.h, _it(row), _vt(val), _p(text), text.numel(), n_rows, n_cols, entries,
                                             fields, symmetry, flags, cap, _p(row), _p(col), _p(val), C.byref(nnz)))
    k = nnz.value
    return row[:k], col[:k], (None if val is None else val[:k])


def mtx_parse_values(text, count, value_dtype):
    """text: uint8 device tensor with the bytes after the size line of an array-format file.  Returns its first `count`
    values, in file order (sbio_mtx_parse_values)."""
    hd = handle_for(_check_dev(text))
    val = torch.empty(max(1, count), dtype=value_dtype, device=text.device)
    hd.check(hd.lib.sbio_mtx_parse_values(hd.h, _vt(val), _p(text), text.numel(), count, _p(val)))
    return val[:count]


def dense_to_coo(n, m, dense, index_dtype=torch.int32):
    """dense: n * m values in column-major order (cell (r, c) at c * n + r).  Returns (row, col, val) of the cells with
    value != 0, ordered by (row, col), trimmed to nnz (sbio_dense_to_coo: the counting call, the allocation, the fill)."""
    dev = _check_dev(dense)
    hd = handle_for(dev)
    if dense.numel() != n * m:
        raise ValueError(f"dense holds {dense.numel()} values, {n} x {m} needs {n * m}")
    it = _it(torch.empty(0, dtype=index_dtype))
    nnz = C.c_int64(0)
    hd.check(hd.lib.sbio_dense_to_coo(hd.h, it, _vt(dense), n, m, _p(dense), 0, None, None, None, C.byref(nnz)))
    k = nnz.value
    row = torch.empty(k, dtype=index_dtype, device=dev)
    col = torch.empty(k, dtype=index_dtype, device=dev)
    val = torch.empty(k, dtype=dense.dtype, device=dev)
    if k:
        hd.check(hd.lib.sbio_dense_to_coo(hd.h, it, _vt(dense), n, m, _p(dense), k, _p(row), _p(col), _p(val), C.byref(nnz)))
        assert nnz.value == k
    return row, col, val


def coo_to_dense_vector(length, row, col, val):
    """The dense vector of a sorted COO of a 1 x N or N x 1 matrix: zeros, then out[row + col] = val, the last of equal
    positions winning (sbio_coo_to_dense_vector)."""
    dev = _check_dev(row, col, val)
    hd = handle_for(dev)
    out = torch.empty(length, dtype=val.dtype, device=dev)
    hd.check(hd.lib.sbio_coo_to_dense_vector(hd.h, _it(row), _vt(val), length, row.numel(), _p(row), _p(col), _p(val), _p(out)))
    return out


def text_count_tokens(text):
    hd = handle_for(_check_dev(text))
    out = C.c_int64(0)
    hd.check(hd.lib.sbx_text_count_tokens(hd.h, _p(text), text.numel(), C.byref(out)))
    return out.value


def edge_list_parse(text, weighted=False, remove_duplicates=False, remove_self_edges=False, read_undirected=True,
                    square=False, index_dtype=torch.int32, value_dtype=None):
    """Edge list text (uint8 device tensor) -> (n, m, row, col, val) sorted by (row, col); EdgeListReader::ReadCOO."""
    hd = handle_for(_check_dev(text))
    fields = 3 if weighted else 2
    tokens = text_count_tokens(text)
    if tokens % fields:
        raise ValueError(f"edge list holds {tokens} tokens, not a multiple of {fields}")
    entries = tokens // fields
    cap = max(1, entries * (2 if read_undirected else 1))
    row = torch.empty(cap, dtype=index_dtype, device=text.device)
    col = torch.empty(cap, dtype=index_dtype, device=text.device)
    val = None if (value_dtype is None or not weighted) else torch.empty(cap, dtype=value_dtype, device=text.device)
    dims = (C.c_int64 * 3)()
    flags = (1 if remove_duplicates else 0) | (2 if remove_self_edges else 0) | (4 if read_undirected else 0) | \
        (8 if square else 0)
    hd.check(hd.lib.sbx_edge_list_parse(hd.h, _it(row), _vt(val), _p(text), text.numel(), entries, int(weighted), flags,
                                        cap, _p(row), _p(col), _p(val), dims))
    k = dims[2]
    return dims[0], dims[1], row[:k], col[:k], (None if val is None else val[:k])


# ----------------------------------------------------------------------------- features
def csr_degrees(row_ptr, id_dtype=None):
    """id_dtype=torch.int32 over an int64 row_ptr: the <32-bit ids, 64-bit offsets> tuple (degrees are ids)."""
    hd = handle_for(_check_dev(row_ptr))
    n = row_ptr.numel() - 1
    out = torch.empty(n, dtype=id_dtype or row_ptr.dtype, device=row_ptr.device)
    hd.check(hd.lib.sbx_csr_degrees(hd.h, _it(row_ptr, out), n, _p(row_ptr), _p(out)))
    return out


def csr_degree_distribution(row_ptr, nnz, dtype=torch.float32):
    hd = handle_for(_check_dev(row_ptr))
    n = row_ptr.numel() - 1
    out = torch.empty(n, dtype=dtype, device=row_ptr.device)
    hd.check(hd.lib.sbx_csr_degree_distribution(hd.h, _it(row_ptr), n, nnz, _p(row_ptr), out.element_size(), _p(out)))
    return out


def csr_bandwidth(row_ptr, col):
    hd = handle_for(_check_dev(row_ptr, col))
    out = C.c_int64(0)
    hd.check(hd.lib.sbx_csr_bandwidth(hd.h, _it(row_ptr, col), row_ptr.numel() - 1, col.numel(), _p(row_ptr), _p(col),
                                      C.byref(out)))
    return out.value


def csr_profile(row_ptr, col):
    hd = handle_for(_check_dev(row_ptr, col))
    out = C.c_int64(0)
    hd.check(hd.lib.sbx_csr_profile(hd.h, _it(row_ptr, col), row_ptr.numel() - 1, col.numel(), _p(row_ptr), _p(col),
                                    C.byref(out)))
    return out.value


def csr_degrees_degree_distribution(row_ptr, nnz, dtype=torch.float32, id_dtype=None, out=None):
    """Degrees and DegreeDistribution of a CSR in one pass over row_ptr (feature::Degrees_DegreeDistribution): the pair
    (degrees, distribution), bit for bit what csr_degrees and csr_degree_distribution return.  out=(degrees,
    distribution) writes into the caller's tensors.  See sbfx_csr_degrees_degree_distribution in include/sbfx.h."""
    hd = handle_for(_check_dev(row_ptr, *(out or ())))
    n = row_ptr.numel() - 1
    if out is None:
        out = (torch.empty(n, dtype=id_dtype or row_ptr.dtype, device=row_ptr.device),
               torch.empty(n, dtype=dtype, device=row_ptr.device))
    deg, dist = out
    if deg.numel() != n or dist.numel() != n or dist.dtype not in (torch.float32, torch.float64):
        raise ValueError("out: n degrees of the id type and n float32 / float64 values")
    hd.check(hd.lib.sbfx_csr_degrees_degree_distribution(hd.h, _it(row_ptr, deg), n, int(nnz), _p(row_ptr),
                                                         dist.element_size(), _p(deg), _p(dist)))
    return deg, dist


def csr_bandwidth_profile(row_ptr, col):
    """Bandwidth and Profile of a CSR in one pass over col (feature::Bandwidth_Profile): the pair of ints csr_bandwidth
    and csr_profile return.  See sbfx_csr_bandwidth_profile in include/sbfx.h."""
    hd = handle_for(_check_dev(row_ptr, col))
    bw, pr = C.c_int64(0), C.c_int64(0)
    hd.check(hd.lib.sbfx_csr_bandwidth_profile(hd.h, _it(row_ptr, col), row_ptr.numel() - 1, col.numel(), _p(row_ptr),
                                               _p(col), C.byref(bw), C.byref(pr)))
    return bw.value, pr.value


def csr_jaccard_weights(row_ptr, col, dtype=torch.float32):
    """Jaccard weight of every nonzero of a square CSR graph with sorted rows (feature::JaccardWeights): a device
    tensor of col.numel() float32 / float64 values, see sbx_csr_jaccard_weights in include/sbx.h for the rules."""
    hd = handle_for(_check_dev(row_ptr, col))
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"Jaccard weights are float32 or float64, not {dtype}")
    out = torch.empty(col.numel(), dtype=dtype, device=row_ptr.device)
    hd.check(hd.lib.sbx_csr_jaccard_weights(hd.h, _it(row_ptr, col), row_ptr.numel() - 1, col.numel(), _p(row_ptr),
                                            _p(col), out.element_size(), _p(out)))
    return out


def csr_triangle_count(row_ptr, col, directed=False, exact=False):
    """feature::TriangleCount of a square CSR graph, an int.  exact=False is the reference's value (which is not the
    number of triangles: a 4-cycle 1-2-3-4 gives 1, a triangle 0-1-2 gives 0); exact=True counts the triangles of the
    simple undirected graph, or with directed=True the directed 3-cycles.  See sbx_csr_triangle_count in
    include/sbx.h for the rules."""
    hd = handle_for(_check_dev(row_ptr, col))
    out = C.c_int64(0)
    flags = (capi.TC_DIRECTED if directed else 0) | (capi.TC_EXACT if exact else 0)
    hd.check(hd.lib.sbx_csr_triangle_count(hd.h, _it(row_ptr, col), row_ptr.numel() - 1, col.numel(), _p(row_ptr),
                                           _p(col), flags, C.byref(out)))
    return out.value


def degree_stats(ptr, median=True, log=True):
    """Every statistic of the degrees ptr[i + 1] - ptr[i] of an offset array (a CSR's row_ptr, a CSC's col_ptr) in one
    synchronous call: a dict of Python ints (count, sum, min, max, zeros, sumsq — one exact int —, median_lo, median_hi)
    plus the float sum_log.  median=False leaves both medians -1, log=False leaves sum_log 0.  See
    sbxstat_degree_stats in include/sbx_stats.h."""
    hd = handle_for(_check_dev(ptr))
    out = capi.StatDegrees()
    flags = (capi.STAT_MEDIAN if median else 0) | (capi.STAT_LOG if log else 0)
    hd.check(hd.lib.sbxstat_degree_stats(hd.h, _it(ptr), ptr.numel() - 1, _p(ptr), flags, C.byref(out)))
    res = {k: int(getattr(out, k)) for k in ("count", "sum", "min", "max", "zeros", "median_lo", "median_hi")}
    res["sumsq"] = (int(out.sumsq_hi) << 64) | int(out.sumsq_lo)
    res["sum_log"] = float(out.sum_log)
    return res


def csr_off_diag_block_nnz(row_ptr, col, m, block_rows, block_cols=None):
    """feature::OffDiagBlockNNZ: the number of entries outside the diagonal blocks when the rows are cut into
    block_rows contiguous blocks and the m columns into block_cols (block_rows when None), an int.  See
    sbxstat_csr_off_diag_block_nnz in include/sbx_stats.h for the rule."""
    hd = handle_for(_check_dev(row_ptr, col))
    out = C.c_int64(0)
    hd.check(hd.lib.sbxstat_csr_off_diag_block_nnz(hd.h, _it(row_ptr, col), row_ptr.numel() - 1, int(m), col.numel(),
                                                   _p(row_ptr), _p(col), int(block_rows),
                                                   int(block_rows if block_cols is None else block_cols), C.byref(out)))
    return out.value


# ----------------------------------------------------------------------------- reorderers
def degree_reorder(row_ptr, ascending=True, out=None, id_dtype=None):
    hd = handle_for(_check_dev(row_ptr))
    n = row_ptr.numel() - 1
    inv = torch.empty(n, dtype=id_dtype or row_ptr.dtype, device=row_ptr.device) if out is None else out
    hd.check(hd.lib.sbx_degree_reorder(hd.h, _it(row_ptr, inv), n, _p(row_ptr), int(bool(ascending)), _p(inv)))
    return inv


def rcm_reorder(row_ptr, col, out=None, return_stats=False, symmetrize=False):
    """symmetrize=True orders the pattern of A + A^T where A is not structurally symmetric (what sbx_rcm_reorder refuses):
    one sbsym_csr_symmetrize call in pattern mode that leaves a symmetric A alone, then RCM on A or on the symmetrized
    pattern."""
    hd = handle_for(_check_dev(row_ptr, col))
    n = row_ptr.numel() - 1
    if symmetrize:
        rp_s, col_s, _, added = _csr_symmetrize(hd, row_ptr, col, None, capi.SYM_SKIP_IF_SYMMETRIC)
        if added:
            row_ptr, col = rp_s, col_s
    inv = torch.empty(n, dtype=col.dtype, device=row_ptr.device) if out is None else out
    stats = capi.RcmStats()
    hd.check(hd.lib.sbx_rcm_reorder(hd.h, _it(row_ptr, col), n, col.numel(), _p(row_ptr), _p(col), _p(inv),
                                    C.byref(stats)))
    if return_stats:
        return inv, {k: getattr(stats, k) for k, _ in capi.RcmStats._fields_}
    return inv


# ----------------------------------------------------------------------------- A + A^T (include/sbsym.h)
def csr_missing_mirrors(row_ptr, col):
    """How many entries a square CSR with column-sorted rows lacks to be structurally symmetric, an int (0: it is).
    See sbsym_csr_missing_mirrors in include/sbsym.h."""
    hd = handle_for(_check_dev(row_ptr, col))
    out = C.c_int64(0)
    hd.check(hd.lib.sbsym_csr_missing_mirrors(hd.h, _it(row_ptr, col), row_ptr.numel() - 1, col.numel(), _p(row_ptr),
                                              _p(col), C.byref(out)))
    return out.value


def _csr_symmetrize(hd, row_ptr, col, val, flags):
    """One sbsym_csr_symmetrize call into 2 * nnz entries of capacity (A + A^T never holds more), trimmed."""
    nnz = col.numel()
    cap = max(1, 2 * nnz)
    rpo = torch.empty_like(row_ptr)
    co = torch.empty(cap, dtype=col.dtype, device=col.device)
    vo = None if val is None else torch.empty(cap, dtype=val.dtype, device=val.device)
    nnz_out, added = C.c_int64(0), C.c_int64(0)
    hd.check(hd.lib.sbsym_csr_symmetrize(hd.h, _it(row_ptr, col), _vt(val), row_ptr.numel() - 1, nnz, _p(row_ptr), _p(col),
                                         _p(val), flags, cap, _p(rpo), _p(co), _p(vo), C.byref(nnz_out), C.byref(added)))
    k = nnz_out.value
    return rpo, co[:k], (None if vo is None else vo[:k]), added.value


def csr_symmetrize(row_ptr, col, val=None, no_diagonal=False):
    """A + A^T of a square CSR with column-sorted rows: (row_ptr_out, col_out, val_out, added).  Every stored entry stays,
    with its value; every missing mirror is added once, with the value of the first stored entry it mirrors; values are
    opaque payloads.  no_diagonal drops the stored (i, i).  See sbsym_csr_symmetrize in include/sbsym.h."""
    hd = handle_for(_check_dev(row_ptr, col, val))
    return _csr_symmetrize(hd, row_ptr, col, val, capi.SYM_NO_DIAGONAL if no_diagonal else 0)


# ----------------------------------------------------------------------------- y = A x (include/sbmv.h)
def csr_check(row_ptr, col, m):
    """Raises capi.SbxError (bad argument; the message names what failed and where) unless (row_ptr, col) is a
    well-formed CSR with m columns: row_ptr[0] == 0, row_ptr non-decreasing, row_ptr[n] == nnz, every column in [0, m).
    Synchronous.  See sbmv_csr_check in include/sbmv.h."""
    hd = handle_for(_check_dev(row_ptr, col))
    hd.check(hd.lib.sbmv_csr_check(hd.h, _it(row_ptr, col), row_ptr.numel() - 1, int(m), col.numel(), _p(row_ptr), _p(col)))


def csr_spmv(row_ptr, col, x, val=None, m=None, out=None):
    """y = A x of a CSR matrix: a device tensor of n values of x's dtype (float32, float64, int32 or int64; integers wrap).
    val=None is a pattern matrix (every stored value 1); m defaults to x.numel().  Deterministic and asynchronous; an
    entry whose column lies outside [0, m) contributes nothing.  See sbmv_csr_spmv in include/sbmv.h."""
    hd = handle_for(_check_dev(row_ptr, col, x, val, out))
    n = row_ptr.numel() - 1
    m = x.numel() if m is None else int(m)
    if m > x.numel():
        raise ValueError(f"x holds {x.numel()} values, the matrix has {m} columns")
    if val is not None and (val.dtype != x.dtype or val.numel() != col.numel()):
        raise TypeError("val must have the dtype of x and one value per stored entry")
    y = torch.empty(n, dtype=x.dtype, device=x.device) if out is None else out
    if y.dtype != x.dtype or y.numel() != n:
        raise TypeError("out must have the dtype of x and one value per row")
    hd.check(hd.lib.sbmv_csr_spmv(hd.h, _it(row_ptr, col), _vt(x), n, m, col.numel(), _p(row_ptr), _p(col), _p(val), _p(x),
                                  _p(y)))
    return y


# ----------------------------------------------------------------------------- Y = A X (include/sbmm.h)
def _check_rows(t, what):
    """A 2-D device tensor whose rows are contiguous (stride(1) == 1, any leading dimension at least its width)."""
    if not t.is_cuda:
        raise ValueError("sparsebase_amd.ops works on device tensors only (no CPU path)")
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{what} must be 2-D with stride(1) == 1 and stride(0) >= its width")


def _ld(t):
    return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])


def csr_spmm(row_ptr, col, X, val=None, m=None, out=None):
    """Y = A X of a CSR matrix and a dense row-major block: a device tensor of n x k values of X's dtype (float32, float64,
    int32 or int64; integers wrap).  X is 2-D with stride(1) == 1 (a column slice of a wider tensor is fine: its stride(0)
    is the leading dimension), as is `out`.  val=None is a pattern matrix (every stored value 1); m defaults to
    X.shape[0].  Deterministic and asynchronous; an entry whose column lies outside [0, m) contributes nothing; nothing is
    written outside out[:, :k].  See sbmm_csr_spmm in include/sbmm.h."""
    dev = _check_dev(row_ptr, col, val)
    _check_rows(X, "X")
    if out is not None:
        _check_rows(out, "out")
    if X.device != dev or (out is not None and out.device != dev):
        raise ValueError("all tensors must live on the same device")
    hd = handle_for(dev)
    n, k = row_ptr.numel() - 1, int(X.shape[1])
    m = int(X.shape[0]) if m is None else int(m)
    if m > X.shape[0]:
        raise ValueError(f"X holds {X.shape[0]} rows, the matrix has {m} columns")
    if val is not None and (val.dtype != X.dtype or val.numel() != col.numel()):
        raise TypeError("val must have the dtype of X and one value per stored entry")
    y = torch.empty((n, k), dtype=X.dtype, device=X.device) if out is None else out
    if y.dtype != X.dtype or tuple(y.shape) != (n, k):
        raise TypeError("out must have the dtype of X, one row per row of the matrix and one column per column of X")
    hd.check(hd.lib.sbmm_csr_spmm(hd.h, _it(row_ptr, col), _vt(X), n, m, col.numel(), k, _p(row_ptr), _p(col), _p(val),
                                  _p(X), _ld(X), _p(y), _ld(y)))
    return y


# ----------------------------------------------------------------------------- out = val (.) (U V^T) (include/sbdd.h)
def csr_sddmm(row_ptr, col, U, V, val=None, out=None):
    """The sampled dense-dense product on a CSR pattern: out[p] = val[p] * (U[row(p), :] . V[col[p], :]) for every stored
    entry p, a 1-D device tensor of col.numel() values of U's dtype (float32, float64, int32 or int64; integers wrap).  U
    is (n, k) and V is (m, k), both 2-D with stride(1) == 1 (a column slice of a wider tensor is fine: its stride(0) is the
    leading dimension); val=None is a pattern matrix (every stored value 1, out[p] the dot itself).  Deterministic,
    asynchronous and independent of where an entry lies; an entry whose column lies outside [0, m) gets +0.  See
    sbdd_csr_sddmm in include/sbdd.h."""
    dev = _check_dev(row_ptr, col, val, out)
    for t, what in ((U, "U"), (V, "V")):
        if not (t.is_cuda and t.dim() == 2 and t.numel() == 0):  # (the strides of a tensor without elements say nothing)
            _check_rows(t, what)
    if U.device != dev or V.device != dev:
        raise ValueError("all tensors must live on the same device")
    n, nnz, k = row_ptr.numel() - 1, col.numel(), int(U.shape[1])
    if int(U.shape[0]) != n:
        raise ValueError(f"U holds {U.shape[0]} rows, the matrix has {n}")
    if int(V.shape[1]) != k:
        raise ValueError(f"U has {k} columns, V has {V.shape[1]}")
    if V.dtype != U.dtype or U.dtype not in _VT:
        raise ValueError("U and V must have the same dtype: float32, float64, int32 or int64")
    if val is not None and (val.dtype != U.dtype or val.dim() != 1 or val.numel() != nnz):
        raise ValueError("val must be 1-D with the dtype of U and one value per stored entry")
    o = torch.empty(nnz, dtype=U.dtype, device=U.device) if out is None else out
    if o.dtype != U.dtype or o.dim() != 1 or o.numel() != nnz:
        raise ValueError("out must be 1-D with the dtype of U and one value per stored entry")
    hd = handle_for(dev)
    hd.check(hd.lib.sbdd_csr_sddmm(hd.h, _it(row_ptr, col), _vt(U), n, int(V.shape[0]), nnz, k, _p(row_ptr), _p(col), _p(val),
                                   _p(U), _ld(U), _p(V), _ld(V), _p(o)))
    return o


# ----------------------------------------------------------------------------- row softmax (include/sbsm.h)
_FLOATS = (torch.float32,)  # (float64 is not built yet: include/sbsm.h)


def _check_entries(t, what, dtype, nnz):
    if t.dtype != dtype or t.dim() != 1 or t.numel() != nnz:
        raise ValueError(f"{what} must be 1-D with dtype {dtype} and one value per stored entry ({nnz})")


def csr_row_softmax(row_ptr, val, out=None, dtype=None, nnz=None):
    """The softmax over the stored values of every row of a CSR matrix: out[p] = exp(val[p] - max_i) / sum_i, a 1-D device
    tensor of one float32 value per stored entry.  -inf masks an entry (+0; a row of -inf alone is +0
    everywhere); a row with a NaN or a +inf is NaN throughout.  val=None is a pattern (every stored value equal: out[p] =
    1 / len_i) and needs dtype= and nnz=.  `out` may be `val` itself.  Deterministic and asynchronous.  See
    sbsm_csr_row_softmax in include/sbsm.h."""
    dev = _check_dev(row_ptr, val, out)
    if row_ptr.dim() != 1 or row_ptr.numel() < 1:
        raise ValueError("row_ptr must be 1-D with n + 1 offsets")
    if val is None:
        if dtype is None or nnz is None:
            raise ValueError("val=None (a pattern) needs dtype= and nnz=")
        nnz = int(nnz)
    else:
        if (dtype is not None and dtype != val.dtype) or (nnz is not None and int(nnz) != val.numel()):
            raise ValueError("dtype= and nnz= disagree with val")
        dtype, nnz = val.dtype, val.numel()
        _check_entries(val, "val", dtype, nnz)
    if dtype not in _FLOATS:
        raise ValueError("the values must be float32")
    o = torch.empty(nnz, dtype=dtype, device=dev) if out is None else out
    _check_entries(o, "out", dtype, nnz)
    hd = handle_for(dev)
    hd.check(hd.lib.sbsm_csr_row_softmax(hd.h, _it(row_ptr), _VT[dtype], row_ptr.numel() - 1, nnz, _p(row_ptr), _p(val), _p(o)))
    return o


def csr_row_softmax_backward(row_ptr, s, g, out=None):
    """The backward of csr_row_softmax: dz[p] = s[p] * (g[p] - sum over the row of s[q] g[q]), with s the forward's output
    and g the gradient with respect to it.  `out` may be `g` itself.  Deterministic and asynchronous.  See
    sbsm_csr_row_softmax_backward in include/sbsm.h."""
    dev = _check_dev(row_ptr, s, g, out)
    if row_ptr.dim() != 1 or row_ptr.numel() < 1:
        raise ValueError("row_ptr must be 1-D with n + 1 offsets")
    if s.dtype not in _FLOATS:
        raise ValueError("the values must be float32")
    nnz = s.numel()
    _check_entries(s, "s", s.dtype, nnz)
    _check_entries(g, "g", s.dtype, nnz)
    o = torch.empty_like(s) if out is None else out
    _check_entries(o, "out", s.dtype, nnz)
    hd = handle_for(dev)
    hd.check(hd.lib.sbsm_csr_row_softmax_backward(hd.h, _it(row_ptr), _VT[s.dtype], row_ptr.numel() - 1, nnz, _p(row_ptr),
                                                  _p(s), _p(g), _p(o)))
    return o


class _RowSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, row_ptr, val):
        s = csr_row_softmax(row_ptr, val.detach().contiguous())
        ctx.save_for_backward(row_ptr, s)
        return s

    @staticmethod
    def backward(ctx, g):
        row_ptr, s = ctx.saved_tensors
        return None, csr_row_softmax_backward(row_ptr, s, g.contiguous())


def csr_row_softmax_autograd(row_ptr, val):
    """csr_row_softmax as a differentiable function of val: the backward is one call of csr_row_softmax_backward."""
    return _RowSoftmax.apply(row_ptr, val)


# ----------------------------------------------------------------------------- Y = A^T X from a plan (include/sbmt.h)
class TransposePlan(NamedTuple):
    """The pattern of the transpose of an n x m CSR matrix and where each of its entries lies in the CSR arrays: three
    device tensors that depend on (row_ptr, col) alone.  Values never enter: one plan serves every val."""
    n: int
    m: int
    col_ptr: torch.Tensor  # m + 1 offsets, the dtype of row_ptr
    row: torch.Tensor      # nnz row ids, the dtype of col
    perm: torch.Tensor     # nnz positions in the CSR arrays, the dtype of row_ptr


def csr_transpose_plan(row_ptr, col, m):
    """TransposePlan(n, m, col_ptr, row, perm) of a CSR matrix with m columns: perm is the stable order of the stored
    entries by column, (col_ptr, row) the CSR arrays of the transpose.  Synchronous; a column outside [0, m) raises.  See
    sbmt_csr_transpose_plan in include/sbmt.h."""
    hd = handle_for(_check_dev(row_ptr, col))
    if row_ptr.dim() != 1 or row_ptr.numel() < 1 or col.dim() != 1:
        raise ValueError("row_ptr must be 1-D with n + 1 offsets and col 1-D")
    n, m, nnz = row_ptr.numel() - 1, int(m), col.numel()
    cp = torch.empty(m + 1, dtype=row_ptr.dtype, device=row_ptr.device)
    ro = torch.empty_like(col)
    pm = torch.empty(nnz, dtype=row_ptr.dtype, device=row_ptr.device)
    hd.check(hd.lib.sbmt_csr_transpose_plan(hd.h, _it(row_ptr, col), n, m, nnz, _p(row_ptr), _p(col), _p(cp), _p(ro), _p(pm)))
    return TransposePlan(n, m, cp, ro, pm)


def csr_spmm_t(plan, X, val=None, out=None):
    """Y = A^T X from a TransposePlan: a device tensor of m x k values of X's dtype (float32, float64, int32 or int64;
    integers wrap).  X is (n, k), 2-D with stride(1) == 1 (a column slice of a wider tensor is fine), as is `out`.  val
    holds the matrix's values in CSR order, as csr_spmm takes them; val=None is a pattern matrix.  Deterministic and
    asynchronous; for k >= 2 the bits are those of csr_spmm on the materialised transpose.  See sbmt_csr_spmm_t in
    include/sbmt.h."""
    dev = _check_dev(plan.col_ptr, plan.row, plan.perm, val)
    _check_rows(X, "X")
    if out is not None:
        _check_rows(out, "out")
    if X.device != dev or (out is not None and out.device != dev):
        raise ValueError("all tensors must live on the same device")
    n, m, k, nnz = int(plan.n), int(plan.m), int(X.shape[1]), plan.row.numel()
    if plan.col_ptr.numel() != m + 1 or plan.perm.numel() != nnz or plan.perm.dtype != plan.col_ptr.dtype:
        raise ValueError("the plan needs m + 1 offsets and one position, of the offsets' dtype, per stored entry")
    if n > X.shape[0]:
        raise ValueError(f"X holds {X.shape[0]} rows, the matrix has {n}")
    if val is not None and (val.dtype != X.dtype or val.dim() != 1 or val.numel() != nnz):
        raise TypeError("val must be 1-D with the dtype of X and one value per stored entry")
    y = torch.empty((m, k), dtype=X.dtype, device=X.device) if out is None else out
    if y.dtype != X.dtype or tuple(y.shape) != (m, k):
        raise TypeError("out must have the dtype of X, one row per column of the matrix and one column per column of X")
    hd = handle_for(dev)
    hd.check(hd.lib.sbmt_csr_spmm_t(hd.h, _it(plan.col_ptr, plan.row), _vt(X), n, m, nnz, k, _p(plan.col_ptr), _p(plan.row),
                                    _p(plan.perm), _p(val), _p(X), _ld(X), _p(y), _ld(y)))
    return y


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, row_ptr, col, val, X, plan):
        Xd = X.detach()
        vd = None if val is None else val.detach().contiguous()
        ctx.save_for_backward(row_ptr, col, vd, Xd)
        ctx.plan = plan
        return csr_spmm(row_ptr, col, Xd, val=vd, m=plan.m)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        row_ptr, col, val, X = ctx.saved_tensors
        g = g.contiguous()
        dval = dX = None
        if val is not None and ctx.needs_input_grad[2]:
            dval = csr_sddmm(row_ptr, col, g, X)
        if ctx.needs_input_grad[3]:
            dX = csr_spmm_t(ctx.plan, g, val)
        return None, None, dval, dX, None


def csr_spmm_autograd(row_ptr, col, val, X, plan=None, m=None):
    """csr_spmm as a differentiable function of val and X: the backward is dval = csr_sddmm(row_ptr, col, dY, X) (the
    pattern form: no values) and dX = csr_spmm_t(plan, dY, val), each computed only where a gradient is asked for.
    val=None is a pattern matrix and has no gradient.  plan=None builds the TransposePlan on every call, a sort of all
    stored entries: a training loop builds it once with csr_transpose_plan(row_ptr, col, m) and passes it.  Not twice
    differentiable."""
    if plan is None:
        plan = csr_transpose_plan(row_ptr, col, int(X.shape[0]) if m is None else int(m))
    if plan.n != row_ptr.numel() - 1 or (m is not None and int(m) != plan.m):
        raise ValueError("the plan is not one of this matrix")
    if X.dim() == 2 and X.shape[0] > plan.m:  # (rows beyond the matrix's columns take no part and get a gradient of 0)
        X = X[:plan.m]
    return _SpMM.apply(row_ptr, col, val, X, plan)


class _SDDMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, row_ptr, col, val, U, V, plan):
        Ud, Vd = U.detach(), V.detach()
        vd = None if val is None else val.detach().contiguous()
        ctx.save_for_backward(row_ptr, col, vd, Ud, Vd)
        ctx.plan = plan
        return csr_sddmm(row_ptr, col, Ud, Vd, val=vd)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        row_ptr, col, val, U, V = ctx.saved_tensors
        g = g.contiguous()
        dval = dU = dV = None
        if val is not None and ctx.needs_input_grad[2]:
            dval = csr_sddmm(row_ptr, col, U, V, val=g)
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            w = g if val is None else g * val
            if ctx.needs_input_grad[3]:
                dU = csr_spmm(row_ptr, col, V, val=w)
            if ctx.needs_input_grad[4]:
                dV = csr_spmm_t(ctx.plan, U, val=w)
        return None, None, dval, dU, dV, None


def csr_sddmm_autograd(row_ptr, col, U, V, val=None, plan=None):
    """csr_sddmm as a differentiable function of val, U and V.  With g the gradient of the output and w = g * val (w = g
    for a pattern): dval = csr_sddmm(row_ptr, col, U, V, val=g), dU = csr_spmm(row_ptr, col, V, val=w) and
    dV = csr_spmm_t(plan, U, val=w), each computed only where a gradient is asked for.  plan=None builds the
    TransposePlan on every call: a training loop passes one (csr_transpose_plan(row_ptr, col, V.shape[0])).  Not twice
    differentiable."""
    if plan is None:
        plan = csr_transpose_plan(row_ptr, col, int(V.shape[0]))
    if plan.n != row_ptr.numel() - 1 or plan.m != int(V.shape[0]):
        raise ValueError("the plan is not one of this matrix")
    return _SDDMM.apply(row_ptr, col, val, U, V, plan)


def slashburn_reorder(row_ptr, col, k, greedy=False, hub_order=False, out=None, return_stats=False):
    """reorder::SlashburnReorder of a CSR graph: inv[old] = new (the dtype of col).  k hubs per round; greedy and
    hub_order are SlashburnReorderParams' flags, taken from this call alone.  See sbx_slashburn_reorder in
    include/sbx.h for the rules."""
    hd = handle_for(_check_dev(row_ptr, col))
    n = row_ptr.numel() - 1
    inv = torch.empty(n, dtype=col.dtype, device=row_ptr.device) if out is None else out
    stats = capi.SlashburnStats()
    flags = (capi.SB_GREEDY if greedy else 0) | (capi.SB_HUB_ORDER if hub_order else 0)
    hd.check(hd.lib.sbx_slashburn_reorder(hd.h, _it(row_ptr, col), n, col.numel(), _p(row_ptr), _p(col), int(k),
                                          flags, _p(inv), C.byref(stats)))
    if return_stats:
        return inv, {k_: getattr(stats, k_) for k_, _ in capi.SlashburnStats._fields_}
    return inv


def boba_reorder(row, col, n, m, out=None):
    """reorder::BOBAReorder of an n x m COO (row, col: the entries in any order): inv[old] = new for the max(n, m)
    vertices (the dtype of row).  See sbx_boba_reorder in include/sbx.h for the rule."""
    hd = handle_for(_check_dev(row, col))
    if row.dtype != col.dtype:
        raise TypeError("row and col must share one dtype")
    nodes = max(int(n), int(m))
    inv = torch.empty(nodes, dtype=row.dtype, device=row.device) if out is None else out
    hd.check(hd.lib.sbx_boba_reorder(hd.h, _it(row), int(n), int(m), row.numel(), _p(row), _p(col), _p(inv)))
    return inv


def csr_reorder_heatmap(row_ptr, col, order_r, order_c, num_parts, m=None, double=False):
    """reorder::ReorderHeatmap of an n x m CSR placed by order_r (n new row positions) and order_c (m new column
    positions): a device tensor of num_parts^2 float32 (double=True: float64) nonzero shares, cell (i, j) at
    i * num_parts + j.  m defaults to n.  See sbx_csr_reorder_heatmap in include/sbx.h for the rule."""
    hd = handle_for(_check_dev(row_ptr, col, order_r, order_c))
    n = row_ptr.numel() - 1
    m = n if m is None else int(m)
    b = int(num_parts)
    cells = b * b if 1 <= b <= min(n, m) else 0  # (an out-of-range b is the library's to refuse)
    out = torch.empty(cells, dtype=torch.float64 if double else torch.float32, device=row_ptr.device)
    hd.check(hd.lib.sbx_csr_reorder_heatmap(hd.h, _it(row_ptr, col), n, m, col.numel(), _p(row_ptr), _p(col),
                                            _p(order_r), _p(order_c), b, out.element_size(), _p(out)))
    return out


def gray_row_keys(m, row_ptr, col, resolution, nnz_threshold):
    hd = handle_for(_check_dev(row_ptr, col))
    n = row_ptr.numel() - 1
    deg = torch.empty(n, dtype=col.dtype, device=row_ptr.device)
    key = torch.empty(n, dtype=torch.int64, device=row_ptr.device)  # uint64 bit pattern
    counts = (C.c_int64 * 4)()
    hd.check(hd.lib.sbx_gray_row_keys(hd.h, _it(row_ptr, col), n, m, col.numel(), _p(row_ptr), _p(col), int(resolution),
                                      int(nnz_threshold), _p(deg), _p(key), counts))
    return deg, key, list(counts)


def gray_reorder(m, row_ptr, col, resolution, nnz_threshold, group_size, exact_ties=False):
    """GrayReorder with the ordering stage on the device (stable ties; exact_ties=True is refused by the library: the
    exact mode is the host layer's reorder::GrayReorder)."""
    hd = handle_for(_check_dev(row_ptr, col))
    n = row_ptr.numel() - 1
    inv = torch.empty(n, dtype=col.dtype, device=row_ptr.device)
    hd.check(hd.lib.sbx_gray_reorder(hd.h, _it(row_ptr, col), n, m, col.numel(), _p(row_ptr), _p(col), int(resolution),
                                     int(nnz_threshold), int(group_size), 1 if exact_ties else 0, _p(inv)))
    return inv


# ----------------------------------------------------------------------------- permutation
def inverse_permutation(perm):
    hd = handle_for(_check_dev(perm))
    inv = torch.empty_like(perm)
    hd.check(hd.lib.sbx_inverse_permutation(hd.h, _it(perm), perm.numel(), _p(perm), _p(inv)))
    return inv


def permute_csr(n, m, row_ptr, col, val, row_order, col_order, out=None):
    hd = handle_for(_check_dev(row_ptr, col, val, row_order, col_order))
    if out is None:
        rpo = torch.empty_like(row_ptr)
        co = torch.empty_like(col)
        vo = None if val is None else torch.empty_like(val)
    else:
        rpo, co, vo = out
    hd.check(hd.lib.sbx_permute_csr(hd.h, _it(row_ptr, col), _vt(val), n, m, col.numel(), _p(row_ptr), _p(col), _p(val),
                                    _p(row_order), _p(col_order), _p(rpo), _p(co), _p(vo)))
    return rpo, co, vo


def permute_csr_rows_nnz(n, row_ptr, row_order, row_begin, row_end):
    """Entries of the new rows [row_begin, row_end): the size of that shard's col / val slab."""
    hd = handle_for(_check_dev(row_ptr, row_order))
    got = C.c_int64(0)
    hd.check(hd.lib.sbx_permute_csr_rows_nnz(hd.h, _it(row_ptr, row_order), n, _p(row_ptr), _p(row_order), row_begin, row_end,
                                             C.byref(got)))
    return got.value


def permute_csr_rows(n, m, row_ptr, col, val, row_order, col_order, row_begin, row_end, capacity=None):
    """One row-range shard of the permuted matrix (the multi-GPU decomposition)."""
    hd = handle_for(_check_dev(row_ptr, col, val, row_order, col_order))
    nr = row_end - row_begin
    if capacity is None:  # exactly the shard's entries, not the whole matrix's
        capacity = permute_csr_rows_nnz(n, row_ptr, row_order, row_begin, row_end)
    rpo = torch.empty(nr + 1, dtype=row_ptr.dtype, device=row_ptr.device)
    co = torch.empty(max(capacity, 1), dtype=col.dtype, device=col.device)  # (an empty slab still needs an address)
    vo = None if val is None else torch.empty(max(capacity, 1), dtype=val.dtype, device=val.device)
    got = C.c_int64(0)
    hd.check(hd.lib.sbx_permute_csr_rows(hd.h, _it(row_ptr, col), _vt(val), n, m, col.numel(), _p(row_ptr), _p(col),
                                         _p(val), _p(row_order), _p(col_order), row_begin, row_end, _p(rpo), _p(co),
                                         _p(vo), capacity, C.byref(got)))
    k = got.value
    return rpo, co[:k], (None if vo is None else vo[:k])


def permute_array(order, vals):
    hd = handle_for(_check_dev(order, vals))
    out = torch.empty_like(vals)
    hd.check(hd.lib.sbx_permute_array(hd.h, _it(order), _vt(vals), order.numel(), _p(order), _p(vals), _p(out)))
    return out


# ----------------------------------------------------------------------------- sharded steps
class Comm:
    """An sbx communicator: RCCL (`Comm.rccl`, one GPU per rank, the id travels over torch.distributed) or an
    all-gather hook over a torch.distributed group of any backend (`Comm.hook`, e.g. gloo with ranks sharing a GPU)."""

    def __init__(self, lib, handle, keep=None):
        self.lib, self.c, self._keep = lib, handle, keep

    @classmethod
    def rccl(cls, device_index, group=None):
        import torch.distributed as dist
        lib = capi.load()
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        box = [None]
        if rank == 0:
            buf = C.create_string_buffer(capi.COMM_ID_BYTES)
            rc = lib.sbx_comm_unique_id(buf)
            if rc != capi.SBX_OK:
                raise capi.SbxError(rc, "sbx_comm_unique_id failed (librccl not loadable?)")
            box[0] = buf.raw
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        c = C.c_void_p()
        rc = lib.sbx_comm_create_rccl(int(device_index), rank, world, C.c_char_p(box[0]), C.byref(c))
        if rc != capi.SBX_OK:
            raise capi.SbxError(rc, "sbx_comm_create_rccl failed")
        return cls(lib, c)

    @classmethod
    def hook(cls, device_index, group=None):
        """All-gather through torch.distributed on host buffers (staged with sbx_memcpy_*): for backends without
        device collectives and for ranks that share one GPU."""
        import numpy as np
        import torch.distributed as dist
        lib = capi.load()
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        hd = handle_for(torch.device("cuda", device_index))

        def allgather(user, send, recv, nbytes, stream):
            try:
                mine = np.empty(nbytes, np.uint8)
                torch.cuda.current_stream(device_index).synchronize()
                if lib.sbx_memcpy_d2h(hd.h, mine.ctypes.data_as(C.c_void_p), C.c_void_p(send), nbytes) != capi.SBX_OK:
                    return 3
                parts = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(world)]
                dist.all_gather(parts, torch.from_numpy(mine), group=group)
                whole = torch.cat(parts).numpy()
                if lib.sbx_memcpy_h2d(hd.h, C.c_void_p(recv), whole.ctypes.data_as(C.c_void_p), nbytes * world) != capi.SBX_OK:
                    return 3
                return 0
            except Exception:  # noqa: BLE001  (must not unwind through the C frame)
                return 6

        cb = capi.ALLGATHER_FN(allgather)
        c = C.c_void_p()
        rc = lib.sbx_comm_create(rank, world, cb, None, C.byref(c))
        if rc != capi.SBX_OK:
            raise capi.SbxError(rc, "sbx_comm_create failed")
        return cls(lib, c, keep=cb)

    def close(self):
        if self.c:
            self.lib.sbx_comm_destroy(self.c)
            self.c = None


def _splits(ranges):
    if ranges is None:
        return None
    cuts = [ranges[0][0]] + [hi for _, hi in ranges]
    return (C.c_int64 * len(cuts))(*cuts)


def permute_csr_sharded(comm, n, m, row_ptr, col, val, row_order, col_order, ranges=None, out=None, capacity=None):
    """sbx_permute_csr_sharded: returns (global row_ptr, this rank's col, val slabs, shard offsets list).
    `out` = (row_ptr_out (n + 1), col_out, val_out) pre-allocated slabs (capacity = col_out.numel())."""
    hd = handle_for(_check_dev(row_ptr, col, val, row_order, col_order))
    rank, world = C.c_int(0), C.c_int(0)
    hd.lib.sbx_comm_rank(comm.c, C.byref(rank), C.byref(world))
    if out is None:
        if capacity is None:
            lo, hi = ranges[rank.value] if ranges is not None else _equal_range(n, world.value, rank.value)
            capacity = permute_csr_rows_nnz(n, row_ptr, row_order, lo, hi)
        rpo = torch.empty(n + 1, dtype=row_ptr.dtype, device=row_ptr.device)
        co = torch.empty(max(capacity, 1), dtype=col.dtype, device=col.device)
        vo = None if val is None else torch.empty(max(capacity, 1), dtype=val.dtype, device=val.device)
    else:
        rpo, co, vo = out
        capacity = co.numel()
    offs = (C.c_int64 * (world.value + 1))()
    hd.check(hd.lib.sbx_permute_csr_sharded(hd.h, comm.c, _it(row_ptr), _vt(val), n, m, col.numel(), _p(row_ptr), _p(col),
                                            _p(val), _p(row_order), _p(col_order), _splits(ranges), _p(rpo), _p(co),
                                            _p(vo), capacity, offs))
    offs = list(offs)
    k = offs[rank.value + 1] - offs[rank.value]
    return rpo, co[:k], (None if vo is None else vo[:k]), offs


def coo_to_csr_sharded(comm, n, m, row, col, val, ranges=None, out=None, capacity=None):
    """sbx_coo_to_csr_sharded on a replicated row-sorted COO."""
    hd = handle_for(_check_dev(row, col, val))
    rank, world = C.c_int(0), C.c_int(0)
    hd.lib.sbx_comm_rank(comm.c, C.byref(rank), C.byref(world))
    if out is None:
        if capacity is None:
            lo, hi = ranges[rank.value] if ranges is not None else _equal_range(n, world.value, rank.value)
            b = torch.searchsorted(row, torch.tensor([lo, hi], dtype=row.dtype, device=row.device), right=False)
            capacity = int(b[1] - b[0])
        rpo = torch.empty(n + 1, dtype=row.dtype, device=row.device)
        co = torch.empty(max(capacity, 1), dtype=col.dtype, device=col.device)
        vo = None if val is None else torch.empty(max(capacity, 1), dtype=val.dtype, device=val.device)
    else:
        rpo, co, vo = out
        capacity = co.numel()
    offs = (C.c_int64 * (world.value + 1))()
    hd.check(hd.lib.sbx_coo_to_csr_sharded(hd.h, comm.c, _it(row), _vt(val), n, m, row.numel(), _p(row), _p(col), _p(val),
                                           _splits(ranges), _p(rpo), _p(co), _p(vo), capacity, offs))
    offs = list(offs)
    k = offs[rank.value + 1] - offs[rank.value]
    return rpo, co[:k], (None if vo is None else vo[:k]), offs


def csr_to_coo_sharded(comm, n, m, row_ptr, col, val, ranges=None, out=None, capacity=None):
    """sbx_csr_to_coo_sharded on a replicated CSR: this rank's slab of the COO (global row ids).
    Returns (row, col, val slabs, shard offsets list)."""
    hd = handle_for(_check_dev(row_ptr, col, val))
    rank, world = C.c_int(0), C.c_int(0)
    hd.lib.sbx_comm_rank(comm.c, C.byref(rank), C.byref(world))
    if out is None:
        if capacity is None:
            lo, hi = ranges[rank.value] if ranges is not None else _equal_range(n, world.value, rank.value)
            capacity = int(row_ptr[hi] - row_ptr[lo])
        ro = torch.empty(max(capacity, 1), dtype=row_ptr.dtype, device=row_ptr.device)
        co = torch.empty(max(capacity, 1), dtype=col.dtype, device=col.device)
        vo = None if val is None else torch.empty(max(capacity, 1), dtype=val.dtype, device=val.device)
    else:
        ro, co, vo = out
        capacity = co.numel()
    offs = (C.c_int64 * (world.value + 1))()
    hd.check(hd.lib.sbx_csr_to_coo_sharded(hd.h, comm.c, _it(row_ptr), _vt(val), n, m, col.numel(), _p(row_ptr), _p(col),
                                           _p(val), _splits(ranges), _p(ro), _p(co), _p(vo), capacity, offs))
    offs = list(offs)
    k = offs[rank.value + 1] - offs[rank.value]
    return ro[:k], co[:k], (None if vo is None else vo[:k]), offs


def balanced_row_splits(n, row_ptr, row_order, world):
    """sbx_balanced_row_splits: new-row ranges of (nearly) equal entry counts, as a list of (lo, hi)."""
    hd = handle_for(_check_dev(row_ptr, row_order))
    cuts = (C.c_int64 * (world + 1))()
    hd.check(hd.lib.sbx_balanced_row_splits(hd.h, _it(row_ptr), n, _p(row_ptr), _p(row_order), world, cuts))
    cuts = list(cuts)
    return list(zip(cuts[:-1], cuts[1:]))


def _equal_range(n, world, rank):
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


# ----------------------------------------------------------------------------- text output (include/sbx_text.h)
def _text_vt(val, unsigned):
    vt = _vt(val)
    if unsigned:
        if vt not in (capi.V_I32, capi.V_I64):
            raise TypeError("unsigned=True reads an int32 / int64 tensor as uint32 / uint64")
        vt = capi.V_U32 if vt == capi.V_I32 else capi.V_U64
    return vt


def _text_two_calls(hd, device, call):
    """The formatters' protocol: the sizing call, the allocation, the writing call; a uint8 tensor of the exact length."""
    nbytes = C.c_int64(0)
    hd.check(call(None, 0, nbytes))
    text = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    if nbytes.value:
        wrote = C.c_int64(0)
        hd.check(call(_p(text), nbytes.value, wrote))
        assert wrote.value == nbytes.value
    return text


def text_format_values(vals, precision=6, unsigned=False):
    """One value per line, as `ostream << x` prints it at the given precision (sbx_text_format_values)."""
    dev = _check_dev(vals)
    hd = handle_for(dev)
    vt = _text_vt(vals, unsigned)
    return _text_two_calls(hd, dev, lambda out, cap, nb: hd.lib.sbx_text_format_values(
        hd.h, vt, vals.numel(), _p(vals), precision, out, cap, C.byref(nb)))


def text_format_coordinate(row, col, val=None, index_base=1, precision=6, lower=False, no_diagonal=False, pattern=False,
                           unsigned=False):
    """"<row + base> <col + base>[ <value>]\\n" per kept entry, in input order (sbx_text_format_coordinate)."""
    dev = _check_dev(row, col, val)
    hd = handle_for(dev)
    vt = capi.V_NONE if val is None else _text_vt(val, unsigned)
    flags = (capi.TEXT_LOWER if lower else 0) | (capi.TEXT_NO_DIAGONAL if no_diagonal else 0) | \
        (capi.TEXT_PATTERN if pattern else 0)
    return _text_two_calls(hd, dev, lambda out, cap, nb: hd.lib.sbx_text_format_coordinate(
        hd.h, _it(row), vt, row.numel(), _p(row), _p(col), _p(val), index_base, precision, flags, out, cap, C.byref(nb)))


def text_format_dense(n, m, row, col, val=None, precision=6, unsigned=False):
    """The array format of a COO: n * m value lines in column-major order, "0" where nothing is stored."""
    dev = _check_dev(row, col, val)
    hd = handle_for(dev)
    vt = capi.V_NONE if val is None else _text_vt(val, unsigned)
    return _text_two_calls(hd, dev, lambda out, cap, nb: hd.lib.sbx_text_format_dense(
        hd.h, _it(row), vt, n, m, row.numel(), _p(row), _p(col), _p(val), precision, out, cap, C.byref(nb)))


def coo_symmetry_check(n, row, col, val=None, skew=False, unsigned=False):
    """(every off-diagonal entry has a mirror that passes the value test, diagonal entries, diagonal entries != 0):
    the symmetry check of MTXWriter::WriteCOO (sbx_coo_symmetry_check)."""
    hd = handle_for(_check_dev(row, col, val))
    vt = capi.V_NONE if val is None else _text_vt(val, unsigned)
    res = (C.c_int64 * 3)()
    hd.check(hd.lib.sbx_coo_symmetry_check(hd.h, _it(row), vt, n, row.numel(), _p(row), _p(col), _p(val), int(bool(skew)), res))
    return bool(res[0]), res[1], res[2]


def coo_undirected_unique_(row, col, val=None):
    """In place: row <= col, sorted by (row, col), the first of every run of equal coordinates kept; returns the arrays
    trimmed to what is left (sbx_coo_undirected_unique)."""
    hd = handle_for(_check_dev(row, col, val))
    left = C.c_int64(0)
    hd.check(hd.lib.sbx_coo_undirected_unique(hd.h, _it(row), _vt(val), row.numel(), _p(row), _p(col), _p(val), C.byref(left)))
    k = left.value
    return row[:k], col[:k], (None if val is None else val[:k])


coo_undirected_unique = coo_undirected_unique_


# ----------------------------------------------------------------------------- METIS graph files (include/sbgr.h)
def metis_parse(text, n, m, fmt=0, ncon=0, zero_index=True, index_dtype=torch.int32, value_dtype=None,
                offset_dtype=None, row_ptr=True):
    """text: uint8 device tensor with the bytes after the header line; n, m, fmt, ncon as sparsebase_amd.metis.parse_header
    gives them.  Returns (n_dim, row, col, val, vwgt, row_ptr): the COO sorted by (row, col), the edge weights (None unless
    the file has them and value_dtype is given), the n_dim x ncon vertex weights (None likewise) and the row offsets
    (sbgr_metis_parse).  offset_dtype=torch.int64 over int32 ids is the <32-bit ids, 64-bit offsets> tuple."""
    dev = _check_dev(text)
    hd = handle_for(dev)
    offset_dtype = index_dtype if offset_dtype is None else offset_dtype
    it = _it(torch.empty(0, dtype=offset_dtype), torch.empty(0, dtype=index_dtype))
    n_dim, nnz = n + (0 if zero_index else 1), 2 * m
    edge_weighted, vertex_weighted = fmt in (1, 11), fmt >= 10 and ncon > 0
    row = torch.empty(max(1, nnz), dtype=index_dtype, device=dev)
    col = torch.empty(max(1, nnz), dtype=index_dtype, device=dev)
    val = torch.empty(max(1, nnz), dtype=value_dtype, device=dev) if (edge_weighted and value_dtype is not None) else None
    vwgt = torch.empty((max(0, n_dim), ncon), dtype=value_dtype, device=dev) \
        if (vertex_weighted and value_dtype is not None) else None
    rp = torch.empty(max(0, n_dim) + 1, dtype=offset_dtype, device=dev) if row_ptr else None
    vt = capi.V_NONE if value_dtype is None else _VT[value_dtype]
    dims = (C.c_int64 * 2)()
    hd.check(hd.lib.sbgr_metis_parse(hd.h, it, vt, _p(text), text.numel(), n, m, fmt, ncon,
                                     capi.GR_ZERO_INDEX if zero_index else 0, max(1, nnz), _p(row), _p(col), _p(val),
                                     _p(vwgt), _p(rp), dims))
    k = dims[1]
    return dims[0], row[:k], col[:k], (None if val is None else val[:k]), vwgt, rp


def metis_format(row_ptr, col, val=None, vwgt=None, row_begin=0, row_end=None, index_base=1, precision=6,
                 edge_weights=False, vertex_weights=False, unsigned=False):
    """The vertex lines of rows [row_begin, row_end) of a device CSR as MetisGraphWriter::WriteGraph writes them, a uint8
    device tensor (sbgr_metis_format).  vwgt: rows x ncon values of val's dtype."""
    dev = _check_dev(row_ptr, col, val, vwgt)
    hd = handle_for(dev)
    row_end = row_ptr.numel() - 1 if row_end is None else row_end
    weights = val if val is not None else vwgt
    if val is not None and vwgt is not None and val.dtype != vwgt.dtype:
        raise TypeError("edge and vertex weights share one value type")
    vt = capi.V_NONE if weights is None else _text_vt(weights, unsigned)
    ncon = 0 if vwgt is None else (vwgt.shape[1] if vwgt.dim() == 2 else 1)
    flags = (capi.GR_EDGE_WEIGHTS if edge_weights else 0) | (capi.GR_VERTEX_WEIGHTS if vertex_weights else 0)
    return _text_two_calls(hd, dev, lambda out, cap, nb: hd.lib.sbgr_metis_format(
        hd.h, _it(row_ptr, col), vt, row_begin, row_end, _p(row_ptr), _p(col), _p(val), _p(vwgt), ncon, index_base,
        precision, flags, out, cap, C.byref(nb)))


# ----------------------------------------------------------------------------- PaToH hypergraph files (include/sbhg.h)
def patoh_parse(text, cells, nets, pins, base=0, scheme=0, index_dtype=torch.int32, value_dtype=None, offset_dtype=None,
                transpose=True):
    """text: uint8 device tensor with the bytes after the header line; cells, nets, pins, base, scheme as
    sparsebase_amd.patoh.parse_header gives them.  Returns (xpin, pin, xnet, net, net_wgt, cell_wgt): the nets x cells CSR
    in file order and file base, the cells x nets CSR (None with transpose=False) and the weights (None unless value_dtype
    is given; 1 where the file has none) (sbhg_patoh_parse)."""
    dev = _check_dev(text)
    hd = handle_for(dev)
    offset_dtype = index_dtype if offset_dtype is None else offset_dtype
    it = _it(torch.empty(0, dtype=offset_dtype), torch.empty(0, dtype=index_dtype))
    xpin = torch.empty(max(0, nets) + 1, dtype=offset_dtype, device=dev)
    pin = torch.empty(max(1, pins), dtype=index_dtype, device=dev)
    xnet = torch.empty(max(0, cells) + 1, dtype=offset_dtype, device=dev) if transpose else None
    net = torch.empty(max(1, pins), dtype=index_dtype, device=dev) if transpose else None
    nw = torch.empty(max(0, nets), dtype=value_dtype, device=dev) if value_dtype is not None else None
    cw = torch.empty(max(0, cells), dtype=value_dtype, device=dev) if value_dtype is not None else None
    vt = capi.V_NONE if value_dtype is None else _VT[value_dtype]
    counts = (C.c_int64 * 3)()
    hd.check(hd.lib.sbhg_patoh_parse(hd.h, it, vt, _p(text), text.numel(), cells, nets, pins, base, scheme, max(1, pins),
                                     _p(xpin), _p(pin), _p(xnet), _p(net), _p(nw), _p(cw), counts))
    return xpin, pin[:pins], xnet, (None if net is None else net[:pins]), nw, cw


def cells_to_nets(xpin, pin, cells, base=0):
    """(xnet, net) of the nets x cells CSR (xpin, pin): row c lists, in ascending pin position, the net (+ base) of every
    pin equal to c + base (sbhg_cells_to_nets)."""
    dev = _check_dev(xpin, pin)
    hd = handle_for(dev)
    xnet = torch.empty(cells + 1, dtype=xpin.dtype, device=dev)
    net = torch.empty(pin.numel(), dtype=pin.dtype, device=dev)
    hd.check(hd.lib.sbhg_cells_to_nets(hd.h, _it(xpin, pin), cells, xpin.numel() - 1, _p(xpin), _p(pin), base, _p(xnet),
                                       _p(net)))
    return xnet, net


def patoh_format(xpin, pin, net_wgt=None, net_begin=0, net_end=None, index_delta=0, precision=6, net_weights=False,
                 last_newline=True, unsigned=False):
    """The lines of nets [net_begin, net_end) as PatohWriter writes them, a uint8 device tensor (sbhg_patoh_format)."""
    dev = _check_dev(xpin, pin, net_wgt)
    hd = handle_for(dev)
    net_end = xpin.numel() - 1 if net_end is None else net_end
    vt = capi.V_NONE if net_wgt is None else _text_vt(net_wgt, unsigned)
    flags = (capi.HG_NET_WEIGHTS if net_weights else 0) | (0 if last_newline else capi.HG_NO_LAST_NEWLINE)
    return _text_two_calls(hd, dev, lambda out, cap, nb: hd.lib.sbhg_patoh_format(
        hd.h, _it(xpin, pin), vt, net_begin, net_end, _p(xpin), _p(pin), _p(net_wgt), index_delta, precision, flags, out,
        cap, C.byref(nb)))


def patoh_format_weights(wgt, begin=0, end=None, precision=6, unsigned=False):
    """The cell-weight line: wgt[begin:end] joined by single blanks, a uint8 device tensor (sbhg_patoh_format_weights)."""
    dev = _check_dev(wgt)
    hd = handle_for(dev)
    end = wgt.numel() if end is None else end
    vt = _text_vt(wgt, unsigned)
    return _text_two_calls(hd, dev, lambda out, cap, nb: hd.lib.sbhg_patoh_format_weights(
        hd.h, vt, begin, end, _p(wgt), precision, out, cap, C.byref(nb)))
