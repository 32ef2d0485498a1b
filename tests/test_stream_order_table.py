"""The case table of tests/test_stream_order_gpu.py stays complete (no GPU needed): every entry point the C ABI binds
(capi.PROTOTYPES) is the target of a stream-order case or is listed, with its reason, as no stream work — an entry
point added later fails here until it has a case."""
from sparsebase_amd import capi

import test_stream_order_gpu as so


def test_every_entry_point_has_a_stream_order_case_or_a_reason():
    targets = {entry for _, entry, _, _ in so.CASES}
    names = set(capi.PROTOTYPES)
    assert targets <= names, sorted(targets - names)
    assert set(so.NOT_STREAM_WORK) <= names, sorted(set(so.NOT_STREAM_WORK) - names)
    assert not targets & set(so.NOT_STREAM_WORK), sorted(targets & set(so.NOT_STREAM_WORK))
    missing = names - targets - set(so.NOT_STREAM_WORK)
    assert not missing, f"no stream-order case and no entry in NOT_STREAM_WORK: {sorted(missing)}"
    assert all(isinstance(r, str) and r.strip() for r in so.NOT_STREAM_WORK.values())
    # the blocking copies are work on the handle's stream: never exempt
    assert {"sbx_memcpy_h2d", "sbx_memcpy_d2h", "sbx_memcpy_d2d"} <= targets
    # the synchronous / asynchronous table covers exactly the entry points that have cases
    assert set(so.SYNCHRONOUS) == targets, sorted(set(so.SYNCHRONOUS) ^ targets)


def test_every_index_tuple_and_source_file_has_a_case():
    ids = [cid for cid, _, _, _ in so.CASES]
    assert len(ids) == len(set(ids))
    by_entry = {}
    for cid, entry, _, _ in so.CASES:
        by_entry.setdefault(entry, []).append(cid)
    no_offsets = {"sbx_coo_is_sorted", "sbx_coo_sort", "sbx_mtx_parse_coordinate", "sbx_edge_list_parse", "sbx_boba_reorder",
                  "sbx_inverse_permutation", "sbx_permute_array",            # SBX_I32_N64 is SBX_I32 there (include/sbx.h)
                  "sbx_csr_degree_distribution",                             # no id array: SBX_I32_N64 is SBX_I64 there
                  "sbx_balanced_row_splits"}                                 # a sharded entry point: does not take it
    untyped = {"sbx_text_count_tokens", "sbx_memcpy_h2d", "sbx_memcpy_d2h", "sbx_memcpy_d2d", "sbx_memcpy_peer"}
    for entry, cids in by_entry.items():
        if entry in untyped:
            continue
        for tup in ("i32", "i64") if entry in no_offsets else ("i32", "i64", "i32_n64"):
            assert any(f"-{tup}-" in c + "-" for c in cids), (entry, tup)
    # the second read-out mode (a consumer on another stream) at least once per source file with entry points
    other = {entry for _, entry, _, modes in so.CASES if "other" in modes}
    per_file = {"sbx_handle.hip": {"sbx_memcpy_d2d"}, "sbx_convert.hip": {"sbx_coo_sort", "sbx_coo_to_csr", "sbx_coo_to_csc"},
                "sbx_mtx.hip": {"sbx_mtx_parse_coordinate"}, "sbx_features.hip": {"sbx_csr_degrees"},
                "sbx_jaccard.hip": {"sbx_csr_jaccard_weights"}, "sbx_triangles.hip": {"sbx_csr_triangle_count"},
                "sbx_degree.hip": {"sbx_degree_reorder"}, "sbx_rcm.hip / sbx_rcm64.hip": {"sbx_rcm_reorder"},
                "sbx_slashburn.hip": {"sbx_slashburn_reorder"}, "sbx_boba.hip": {"sbx_boba_reorder"},
                "sbx_heatmap.hip": {"sbx_csr_reorder_heatmap"}, "sbx_gray.hip / sbx_gray64.hip": {"sbx_gray_row_keys"},
                "sbx_gray_order.hip": {"sbx_gray_reorder"}, "sbx_permute.hip": {"sbx_permute_csr"},
                "sbx_sharded.hip": {"sbx_permute_csr_rows_nnz"}, "sbx_i64.hip": {"sbx_coo_to_csc", "sbx_permute_csr"}}
    for f, entries in per_file.items():
        assert entries & other, f
