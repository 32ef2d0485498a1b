/*
 * sbmv.h — C ABI of the sparse matrix-vector product y = A x of a CSR matrix: the operation a reordering is meant to
 * speed up, and the kernel the experiment harness of the host layer (sparsebase/experiment/) times over
 * data x preprocessing x kernel.
 *
 *   sbmv_csr_check   is (row_ptr, col) a well-formed n x m CSR of nnz entries?
 *   sbmv_csr_spmv    y[i] = sum of val[p] * x[col[p]] over the stored entries p of row i
 *
 * A header of its own, as sbx_text.h, sbx_stats.h, sbio.h, sbgr.h, sbhg.h, sbfx.h and sbsym.h are: the other headers and
 * their versions do not change when this one does.  The entry points of this header carry the prefix `sbmv_`.  They live
 * in the same library and work on the same handle, arena and stream.  The conventions are those of sbx.h: device pointers
 * unless the name ends in `_host`, nothing allocated and handed back, scratch from the handle's arena, work enqueued on
 * the handle's stream, sbx_status return codes, sbx_last_error text for every refusal.
 *
 * Scratch.  Nothing per row.  sbmv_csr_spmv takes 24 bytes for every 2048 stored entries (under 0.012 bytes per entry:
 * a first row and one partial sum per tile of the entries) plus 128 bytes; sbmv_csr_check takes 128 bytes.
 *
 * Index types.  All three tuples read their arrays at their own width; rows, columns and positions are 64-bit inside.
 * No limit is added to what the tuple can express up to nnz < 2^42 (beyond it SBX_ERR_UNSUPPORTED).  Tested up to
 * n = 70 000 rows, m = 70 000 columns and nnz = 648 558 entries in every tuple, and timed at n = m = 2^22 with
 * nnz = 105 M under SBX_I32 (tools/spmv_probe.py).
 *
 * Determinism.  The same arrays give the same bits in y on every call, handle and stream: there is no floating-point
 * atomic and no sum whose order depends on which wave arrives first.  The order in which the products of a row are
 * added is a function of where the row's entries lie in the array of the stored entries (tiles of 2048 entries, eight
 * consecutive entries per thread, a fixed scan tree over the threads, the partial sums of a row that crosses tiles added
 * in tile order); it is NOT claimed to be the left-to-right sum.  A floating-point sum that is exactly zero is +0.
 * Integer value types are added and multiplied modulo 2^32 or 2^64; the signed and the unsigned enumerator of a width
 * are the same computation.
 *
 * Malformed input never faults.  An entry whose column lies outside [0, m) contributes nothing (as the ids outside
 * [0, n) of sbx_csr_jaccard_weights read as rows without entries).  Row bounds are clamped to [0, nnz], a decreasing
 * pair of row bounds is an empty row, and every entry is added to one row at most; which y a row_ptr that is not a
 * non-decreasing sequence from 0 to nnz gives is otherwise unspecified, but no access leaves the arrays.  A caller that
 * wants a refusal instead calls sbmv_csr_check once.
 *
 * Out of scope: y = alpha A x + beta y, the transposed product (sbmt.h has it for k columns, k = 1 among them), several
 * right-hand sides, CSC and COO inputs, sharded matrices.
 */
#ifndef SBMV_H_
#define SBMV_H_

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBMV_VERSION 100 /* 1.0.0 */

/* SBX_OK when row_ptr[0] == 0, row_ptr is non-decreasing, row_ptr[n] == nnz and every column lies in [0, m).
 * Otherwise SBX_ERR_BAD_ARG; the message names what failed and the first offending row or position.  The values are
 * compared only: nothing is indexed by them.  The order of the columns inside a row and duplicate columns are not
 * checked.
 *   - n, m or nnz negative, nnz > 0 with n == 0, a NULL pointer (row_ptr where n > 0, col where nnz > 0), an unknown index
 *     type: SBX_ERR_BAD_ARG.
 * Synchronous: one read-back (none where n == 0). */
int sbmv_csr_check(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t m, int64_t nnz,
                   const void *row_ptr, const void *col);

/* y = A x.  row_ptr: n + 1 offsets, col: nnz columns, val: nnz values or NULL, x: m values, y: n values; val, x and y
 * are of type vt: SBX_V_F32, SBX_V_F64, SBX_V_I32 / SBX_V_U32 or SBX_V_I64 / SBX_V_U64.
 * val == NULL is a pattern matrix: every stored value is 1.
 * Every one of the n values of y is written, a row without entries as 0, whatever y held before.  y must not overlap
 * an input.
 *   - the refusals of sbmv_csr_check's arguments; SBX_V_NONE or an unknown value type; a NULL x where m > 0 and nnz > 0;
 *     a NULL y where n > 0: SBX_ERR_BAD_ARG.
 * Asynchronous: no read-back; y is complete in stream order, as sbx.h defines it. */
int sbmv_csr_spmv(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz,
                  const void *row_ptr, const void *col, const void *val, const void *x, void *y);

#ifdef __cplusplus
}
#endif
#endif /* SBMV_H_ */
