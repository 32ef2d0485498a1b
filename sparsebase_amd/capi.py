"""ctypes binding of the C ABI in include/sbx.h, include/sbx_text.h, include/sbx_stats.h, include/sbio.h, include/sbgr.h,
include/sbhg.h, include/sbfx.h, include/sbsym.h, include/sbmv.h, include/sbmm.h, include/sbdd.h, include/sbsm.h and include/sbmt.h
(sparsebase_amd/lib/libsbx.so).

There is deliberately NO fallback: if the library is missing or no GPU is
usable, loading / handle creation raises.  torch is used only as the owner of
device memory and streams; every pointer handed to the ABI is a raw device
pointer.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsbx.so")

SBX_OK = 0
SBX_I32, SBX_I64, SBX_I32_N64 = 0, 1, 2
V_NONE, V_I32, V_U32, V_F32, V_I64, V_U64, V_F64 = range(7)
FLAG_MOVE, FLAG_ROWS_SORTED = 1, 2
TC_DIRECTED, TC_EXACT = 1, 2
SB_GREEDY, SB_HUB_ORDER = 1, 2
TEXT_LOWER, TEXT_NO_DIAGONAL, TEXT_PATTERN = 1, 2, 4
STAT_MEDIAN, STAT_LOG = 1, 2
GR_ZERO_INDEX, GR_EDGE_WEIGHTS, GR_VERTEX_WEIGHTS = 1, 2, 4
HG_NET_WEIGHTS, HG_NO_LAST_NEWLINE = 1, 2
SYM_NO_DIAGONAL, SYM_SKIP_IF_SYMMETRIC = 1, 2

_STATUS = {0: "ok", 1: "bad argument", 2: "no usable HIP device", 3: "HIP runtime error",
           4: "out of device memory", 5: "unsupported type tuple or shape", 6: "internal error"}


class SbxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"sbx status {status} ({_STATUS.get(status, '?')}): {msg}")
        self.status = status


class RcmStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("components", "isolated", "small_components", "large_components",
                                         "bfs_sweeps", "bfs_levels", "edges_scanned", "edges_scanned_bottom_up",
                                         "largest_component", "reference_sweeps", "unordered_sweeps")]


class SlashburnStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("rounds", "hubs", "spoke_components", "initial_components", "final_gcc")]


class StatDegrees(C.Structure):
    _fields_ = ([(k, C.c_int64) for k in ("count", "sum", "min", "max", "zeros")] +
                [("sumsq_lo", C.c_uint64), ("sumsq_hi", C.c_uint64), ("median_lo", C.c_int64), ("median_hi", C.c_int64),
                 ("sum_log", C.c_double)])


# every symbol include/sbx.h declares (tests/test_abi.py checks header <-> library <-> this table)
_i64, _int, _u, _vp, _sz = C.c_int64, C.c_int, C.c_uint, C.c_void_p, C.c_size_t
_H = C.c_void_p
COMM_ID_BYTES = 128
# int (*sbx_allgather_fn)(void *user, const void *send_dev, void *recv_dev, size_t bytes, void *stream)
ALLGATHER_FN = C.CFUNCTYPE(_int, _vp, _vp, _vp, _sz, _vp)
# int (*sbx_oom_hook)(void *user, size_t bytes_wanted)
OOM_HOOK_FN = C.CFUNCTYPE(_int, _vp, _sz)
PROTOTYPES = {
    "sbx_version": ([], _int),
    "sbx_status_string": ([_int], C.c_char_p),
    "sbx_device_count": ([C.POINTER(_int)], _int),
    "sbx_can_access_peer": ([_int, _int, C.POINTER(_int)], _int),
    "sbx_create": ([_int, C.POINTER(_H)], _int),
    "sbx_destroy": ([_H], _int),
    "sbx_set_stream": ([_H, _vp], _int),
    "sbx_get_device": ([_H, C.POINTER(_int)], _int),
    "sbx_reserve": ([_H, _sz], _int),
    "sbx_sync": ([_H], _int),
    "sbx_last_error": ([_H], C.c_char_p),
    "sbx_set_oom_hook": ([_H, OOM_HOOK_FN, _vp], _int),
    "sbx_profile_enable": ([_H, _int], _int),
    "sbx_profile_kernel_count": ([], _int),
    "sbx_profile_kernel_name": ([_int], C.c_char_p),
    "sbx_profile_query": ([_H, _int, C.POINTER(C.c_double), C.POINTER(_i64)], _int),
    "sbx_profile_query_bytes": ([_H, _int, C.POINTER(_i64)], _int),
    "sbx_malloc": ([_H, _sz, C.POINTER(_vp)], _int),
    "sbx_free": ([_H, _vp], _int),
    "sbx_host_alloc": ([_H, _sz, C.POINTER(_vp)], _int),
    "sbx_host_free": ([_H, _vp], _int),
    "sbx_memcpy_h2d": ([_H, _vp, _vp, _sz], _int),
    "sbx_memcpy_d2h": ([_H, _vp, _vp, _sz], _int),
    "sbx_memcpy_d2d": ([_H, _vp, _vp, _sz], _int),
    "sbx_memcpy_peer": ([_H, _vp, _int, _vp, _int, _sz], _int),
    "sbx_coo_is_sorted": ([_H, _int, _i64, _vp, _vp, C.POINTER(_int)], _int),
    "sbx_coo_sort": ([_H, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp], _int),
    "sbx_csr_rows_sorted": ([_H, _int, _i64, _vp, _vp, C.POINTER(_int)], _int),
    "sbx_csr_sort_rows": ([_H, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp], _int),
    "sbx_coo_to_csr": ([_H, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _u], _int),
    "sbx_csr_to_coo": ([_H, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _u], _int),
    "sbx_coo_to_csc": ([_H, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp], _int),
    "sbx_csr_to_csc": ([_H, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp], _int),
    "sbx_mtx_parse_coordinate": ([_H, _int, _int, _vp, _i64, _i64, _i64, _i64, _int, _int, _u, _i64, _vp, _vp, _vp,
                                 C.POINTER(_i64)], _int),
    "sbx_text_count_tokens": ([_H, _vp, _i64, C.POINTER(_i64)], _int),
    "sbx_edge_list_parse": ([_H, _int, _int, _vp, _i64, _i64, _int, _u, _i64, _vp, _vp, _vp, C.POINTER(_i64)], _int),
    "sbx_csr_degrees": ([_H, _int, _i64, _vp, _vp], _int),
    "sbx_csr_degree_distribution": ([_H, _int, _i64, _i64, _vp, _int, _vp], _int),
    "sbx_csr_bandwidth": ([_H, _int, _i64, _i64, _vp, _vp, C.POINTER(_i64)], _int),
    "sbx_csr_profile": ([_H, _int, _i64, _i64, _vp, _vp, C.POINTER(_i64)], _int),
    "sbx_csr_jaccard_weights": ([_H, _int, _i64, _i64, _vp, _vp, _int, _vp], _int),
    "sbx_csr_triangle_count": ([_H, _int, _i64, _i64, _vp, _vp, _u, C.POINTER(_i64)], _int),
    "sbx_degree_reorder": ([_H, _int, _i64, _vp, _int, _vp], _int),
    "sbx_rcm_reorder": ([_H, _int, _i64, _i64, _vp, _vp, _vp, C.POINTER(RcmStats)], _int),
    "sbx_slashburn_reorder": ([_H, _int, _i64, _i64, _vp, _vp, _i64, _u, _vp, C.POINTER(SlashburnStats)], _int),
    "sbx_boba_reorder": ([_H, _int, _i64, _i64, _i64, _vp, _vp, _vp], _int),
    "sbx_csr_reorder_heatmap": ([_H, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _int, _vp], _int),
    "sbx_gray_row_keys": ([_H, _int, _i64, _i64, _i64, _vp, _vp, _int, _int, _vp, _vp, C.POINTER(_i64)], _int),
    "sbx_gray_reorder": ([_H, _int, _i64, _i64, _i64, _vp, _vp, _int, _int, _int, _int, _vp], _int),
    "sbx_inverse_permutation": ([_H, _int, _i64, _vp, _vp], _int),
    "sbx_permute_csr": ([_H, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _int),
    "sbx_permute_csr_rows": ([_H, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp,
                              _vp, _i64, C.POINTER(_i64)], _int),
    "sbx_permute_array": ([_H, _int, _int, _i64, _vp, _vp, _vp], _int),
    "sbx_comm_create": ([_int, _int, ALLGATHER_FN, _vp, C.POINTER(_vp)], _int),
    "sbx_comm_unique_id": ([_vp], _int),
    "sbx_comm_create_rccl": ([_int, _int, _int, _vp, C.POINTER(_vp)], _int),
    "sbx_comm_rank": ([_vp, C.POINTER(_int), C.POINTER(_int)], _int),
    "sbx_comm_destroy": ([_vp], _int),
    "sbx_permute_csr_rows_nnz": ([_H, _int, _i64, _vp, _vp, _i64, _i64, C.POINTER(_i64)], _int),
    "sbx_permute_csr_sharded": ([_H, _vp, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), _vp,
                                 _vp, _vp, _i64, C.POINTER(_i64)], _int),
    "sbx_coo_to_csr_sharded": ([_H, _vp, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, C.POINTER(_i64), _vp, _vp, _vp,
                                _i64, C.POINTER(_i64)], _int),
    "sbx_csr_to_coo_sharded": ([_H, _vp, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, C.POINTER(_i64), _vp, _vp, _vp,
                                _i64, C.POINTER(_i64)], _int),
    "sbx_balanced_row_splits": ([_H, _int, _i64, _vp, _vp, _int, C.POINTER(_i64)], _int),
}

# every symbol include/sbx_text.h declares (tests/test_text_abi.py checks header <-> library <-> this table); a table of
# its own, as the header is a header of its own: PROTOTYPES stays the table of include/sbx.h
TEXT_PROTOTYPES = {
    "sbx_text_format_values": ([_H, _int, _i64, _vp, _int, _vp, _i64, C.POINTER(_i64)], _int),
    "sbx_text_format_coordinate": ([_H, _int, _int, _i64, _vp, _vp, _vp, _i64, _int, _u, _vp, _i64, C.POINTER(_i64)], _int),
    "sbx_coo_symmetry_check": ([_H, _int, _int, _i64, _i64, _vp, _vp, _vp, _int, C.POINTER(_i64)], _int),
    "sbx_coo_undirected_unique": ([_H, _int, _int, _i64, _vp, _vp, _vp, C.POINTER(_i64)], _int),
    "sbx_text_format_dense": ([_H, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _int, _vp, _i64, C.POINTER(_i64)], _int),
}

# every symbol include/sbx_stats.h declares (tests/test_stats_abi.py checks header <-> library <-> this table): the
# `sbx_` prefix is closed, these carry `sbxstat_`
STATS_PROTOTYPES = {
    "sbxstat_degree_stats": ([_H, _int, _i64, _vp, _u, C.POINTER(StatDegrees)], _int),
    "sbxstat_csr_off_diag_block_nnz": ([_H, _int, _i64, _i64, _i64, _vp, _vp, _i64, _i64, C.POINTER(_i64)], _int),
}

# every symbol include/sbio.h declares (tests/test_io_abi.py checks header <-> library <-> this table): the dense side of
# the Matrix Market path, prefix `sbio_`
IO_PROTOTYPES = {
    "sbio_mtx_parse_values": ([_H, _int, _vp, _i64, _i64, _vp], _int),
    "sbio_dense_to_coo": ([_H, _int, _int, _i64, _i64, _vp, _i64, _vp, _vp, _vp, C.POINTER(_i64)], _int),
    "sbio_coo_to_dense_vector": ([_H, _int, _int, _i64, _i64, _vp, _vp, _vp, _vp], _int),
}

# every symbol include/sbgr.h declares (tests/test_graph_abi.py checks header <-> library <-> this table): the METIS graph
# format, prefix `sbgr_`
GRAPH_PROTOTYPES = {
    "sbgr_metis_parse": ([_H, _int, _int, _vp, _i64, _i64, _i64, _int, _int, _u, _i64, _vp, _vp, _vp, _vp, _vp,
                          C.POINTER(_i64)], _int),
    "sbgr_metis_format": ([_H, _int, _int, _i64, _i64, _vp, _vp, _vp, _vp, _int, _i64, _int, _u, _vp, _i64,
                           C.POINTER(_i64)], _int),
}

# every symbol include/sbhg.h declares (tests/test_hypergraph_abi.py checks header <-> library <-> this table): the PaToH
# hypergraph format, prefix `sbhg_`
HYPERGRAPH_PROTOTYPES = {
    "sbhg_patoh_parse": ([_H, _int, _int, _vp, _i64, _i64, _i64, _i64, _int, _int, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                          C.POINTER(_i64)], _int),
    "sbhg_cells_to_nets": ([_H, _int, _i64, _i64, _vp, _vp, _int, _vp, _vp], _int),
    "sbhg_patoh_format": ([_H, _int, _int, _i64, _i64, _vp, _vp, _vp, _i64, _int, _u, _vp, _i64, C.POINTER(_i64)], _int),
    "sbhg_patoh_format_weights": ([_H, _int, _i64, _i64, _vp, _int, _vp, _i64, C.POINTER(_i64)], _int),
}

# every symbol include/sbfx.h declares (tests/test_extract_abi.py checks header <-> library <-> this table): the fused
# feature classes, prefix `sbfx_`
EXTRACT_PROTOTYPES = {
    "sbfx_csr_degrees_degree_distribution": ([_H, _int, _i64, _i64, _vp, _int, _vp, _vp], _int),
    "sbfx_csr_bandwidth_profile": ([_H, _int, _i64, _i64, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)], _int),
}

# every symbol include/sbsym.h declares (tests/test_sym_abi.py checks header <-> library <-> this table): the pattern
# symmetrization A + A^T of a CSR, prefix `sbsym_`
SYM_PROTOTYPES = {
    "sbsym_csr_missing_mirrors": ([_H, _int, _i64, _i64, _vp, _vp, C.POINTER(_i64)], _int),
    "sbsym_csr_symmetrize": ([_H, _int, _int, _i64, _i64, _vp, _vp, _vp, _u, _i64, _vp, _vp, _vp, C.POINTER(_i64),
                              C.POINTER(_i64)], _int),
}

# every symbol include/sbmv.h declares (tests/test_mv_abi.py checks header <-> library <-> this table): the CSR
# matrix-vector product and its input check, prefix `sbmv_`
MV_PROTOTYPES = {
    "sbmv_csr_check": ([_H, _int, _i64, _i64, _i64, _vp, _vp], _int),
    "sbmv_csr_spmv": ([_H, _int, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp], _int),
}

# every symbol include/sbmm.h declares (tests/test_mm_abi.py checks header <-> library <-> this table): the CSR times
# dense block product, prefix `sbmm_`
MM_PROTOTYPES = {
    "sbmm_csr_spmm": ([_H, _int, _int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64], _int),
}

# every symbol include/sbdd.h declares (tests/test_dd_abi.py checks header <-> library <-> this table): the sampled
# dense-dense product on a CSR pattern, prefix `sbdd_`
DD_PROTOTYPES = {
    "sbdd_csr_sddmm": ([_H, _int, _int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp], _int),
}

# every symbol include/sbsm.h declares (tests/test_sm_abi.py checks header <-> library <-> this table): the row softmax
# over a CSR's stored values and its backward, prefix `sbsm_`
SM_PROTOTYPES = {
    "sbsm_csr_row_softmax": ([_H, _int, _int, _i64, _i64, _vp, _vp, _vp], _int),
    "sbsm_csr_row_softmax_backward": ([_H, _int, _int, _i64, _i64, _vp, _vp, _vp, _vp], _int),
}

# every symbol include/sbmt.h declares (tests/test_mt_abi.py checks header <-> library <-> this table): the plan of the
# transpose and the transposed product from it, prefix `sbmt_`
MT_PROTOTYPES = {
    "sbmt_csr_transpose_plan": ([_H, _int, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp], _int),
    "sbmt_csr_spmm_t": ([_H, _int, _int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64], _int),
}

_lib = None


def load():
    """Load libsbx.so (building is __graft_entry__.build()'s job, not an import side effect)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -m sparsebase_amd.build` "
                              "(there is no CPU fallback for the HIP hot path)")
        lib = C.CDLL(LIB_PATH)
        for name, (argtypes, restype) in (list(PROTOTYPES.items()) + list(TEXT_PROTOTYPES.items()) +
                                           list(STATS_PROTOTYPES.items()) + list(IO_PROTOTYPES.items()) +
                                           list(GRAPH_PROTOTYPES.items()) + list(HYPERGRAPH_PROTOTYPES.items()) +
                                           list(EXTRACT_PROTOTYPES.items()) + list(SYM_PROTOTYPES.items()) +
                                           list(MV_PROTOTYPES.items()) + list(MM_PROTOTYPES.items()) +
                                           list(DD_PROTOTYPES.items()) + list(SM_PROTOTYPES.items()) +
                                           list(MT_PROTOTYPES.items())):
            fn = getattr(lib, name)  # AttributeError here == header/library drift: fail loudly
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
    return _lib
