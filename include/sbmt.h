/*
 * sbmt.h — C ABI of the transposed product Y = Aᵀ X of a CSR matrix A (n x m) and a dense row-major X (n x k), from a
 * plan that is built once per sparsity pattern and reused for every array of values: the backward of sbmm.h's Y = A X
 * with respect to X, and of sbdd.h's product with respect to V.
 *
 *   sbmt_csr_transpose_plan   the pattern of Aᵀ (col_ptr, row) and, for every entry of it, its position in the CSR arrays
 *   sbmt_csr_spmm_t           Y[c*ldy + j] = sum of val[perm[q]] * X[row[q]*ldx + j] over col_ptr[c] <= q < col_ptr[c+1]
 *
 * A header of its own, as sbx_text.h, sbx_stats.h, sbio.h, sbgr.h, sbhg.h, sbfx.h, sbsym.h, sbmv.h, sbmm.h, sbdd.h and
 * sbsm.h are: the other headers and their versions do not change when this one does.  The entry points of this header
 * carry the prefix `sbmt_`.  They live in the same library and work on the same handle, arena and stream.  The
 * conventions are those of sbx.h: device pointers unless the name ends in `_host`, nothing allocated and handed back,
 * scratch from the handle's arena, work enqueued on the handle's stream, sbx_status return codes, sbx_last_error text for
 * every refusal.
 *
 * The plan is three device arrays that the caller owns: there is no object behind them, no state in the handle and no
 * lifetime rule beyond the arrays' own.  A plan depends on (row_ptr, col) alone.  A training step that changes the
 * values of A passes the new val to sbmt_csr_spmm_t with the old plan: nothing is sorted again and no value is moved.
 *
 * The product is sbmm_csr_spmm (sbmm.h) of the m x n CSR matrix (col_ptr, row) whose q-th value is val[perm[q]], and is
 * held to it bit for bit: for k >= 2, and for k == 1 wherever sbmm_csr_spmm does not hand over to the kernels of
 * sbmv_csr_spmv (that is unless ldx == 1 and ldy == 1), the bits of Y are those of
 *     sbmm_csr_spmm(h, it, vt, m, n, nnz, k, col_ptr, row, w, x, ldx, y, ldy)      with w[q] = val[perm[q]]
 * at the same alignment of x and y (and whatever alignment of w).  The indirection changes where a value comes from,
 * never the order of a sum: everything sbmm.h says about determinism, the order of the sums, +0, the integer types,
 * the padding, alignment and the 16-byte path holds here with "row" read as "column of A".  For k == 1 at unit strides
 * this header keeps the span kernel too (sbmv.h has no indirection): the result is deterministic, is the exact sum
 * wherever every product and partial sum is exact, and meets sbmm.h's order of the sums at k == 1, so that its error is
 * bounded as a sum of len terms in any order is; it is not claimed to carry the bits of sbmv_csr_spmv.
 *
 * Scratch.  sbmt_csr_spmm_t: what sbmm.h states for this nnz and k, ceil(nnz / 2048) * (16 + k * sizeof(value)) bytes
 * plus at most 1 KiB; nothing per entry: the values are read through perm inside the product's kernel and never
 * gathered into a copy.  sbmt_csr_transpose_plan: that of sbx_csr_to_csc without values on the same arrays (the row
 * of every entry, and two (column key, position) records per entry for the sort).
 *
 * Out of scope: Y = alpha Aᵀ X + beta Y and accumulation into Y, a matrix-vector fast path for k == 1, CSC or COO as
 * the primary input, column-major X or Y, 2-byte value types, sharded matrices.
 */
#ifndef SBMT_H_
#define SBMT_H_

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBMT_VERSION 100 /* 1.0.0 */

/* The plan of Aᵀ.  row_ptr: n + 1 offsets, col: nnz columns of the CSR matrix A (n x m).
 *   col_ptr_out  m + 1 offsets at the width of row_ptr: column c of A holds the entries col_ptr_out[c] <= q < col_ptr_out[c+1]
 *   row_out      nnz row ids at the width of col: the row of A of entry q
 *   perm_out     nnz positions at the width of row_ptr: entry q is the entry perm_out[q] of the CSR arrays,
 *                col[perm_out[q]] == c for every q of column c
 * The order is fully specified: the positions of a column ascend, that is perm_out is the stable order of the positions
 * 0 ... nnz - 1 by column.  So for a well-formed CSR the rows of a column ascend (whether or not the columns inside a row
 * of A are sorted), and duplicated (row, column) entries keep their order.  (col_ptr_out, row_out) is what
 * sbx_csr_to_csc gives on the same arrays, and val[perm_out[q]] is its val_out[q].
 * Limits: those of sbx_csr_to_csc, nnz < 2^31 and n, m < 2^31 - 1 in every tuple (the positions travel through the
 * sort as 4-byte payloads); beyond them SBX_ERR_UNSUPPORTED, and the message names the argument.
 * Refused before any array is read, with SBX_ERR_BAD_ARG and the argument's name in the message: n, m or nnz negative;
 * a NULL row_ptr or col_ptr_out (whatever n and m are, as sbx_csr_to_csc); a NULL col, row_out or perm_out where
 * nnz > 0; an unknown index type.
 * Malformed input.  A column outside [0, m): SBX_ERR_BAD_ARG ("a column lies outside [0, m)"), found by a check of col
 * that is read back before anything is sorted; the outputs are then unspecified.  (sbx_csr_to_csc does the same under
 * SBX_I64, where the message names sbx_coo_to_csr and "a row id": the columns are the row ids of the transpose.  Under
 * 32-bit column ids sbx_csr_to_csc has no such check and a column in range is its caller's precondition; this call does
 * not inherit that.)  row_ptr is read by sbx_csr_to_coo, exactly as sbx_csr_to_csc has it read, and a well-formed row_ptr
 * (non-decreasing from 0 to nnz) is this call's precondition as it is that one's: sbmv_csr_check (sbmv.h) is the
 * checker.  col_ptr_out and perm_out depend on col alone.
 * Synchronous for status, as sbx_csr_to_csc is (the check of col and the conversions inside read back); the outputs are
 * complete in stream order. */
int sbmt_csr_transpose_plan(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t m, int64_t nnz,
                            const void *row_ptr, const void *col,
                            void *col_ptr_out, void *row_out, void *perm_out);

/* Y (m x k) = Aᵀ X.  col_ptr: m + 1 offsets, row: nnz row ids, perm: nnz positions (the three arrays of
 * sbmt_csr_transpose_plan, at the widths given there), val: the nnz values of the CSR matrix in CSR order or NULL,
 * x: n rows of k values at a leading dimension of ldx elements, y: m rows of k values at a leading dimension of ldy
 * elements; val, x and y are of type vt: SBX_V_F32, SBX_V_F64, SBX_V_I32 / SBX_V_U32 or SBX_V_I64 / SBX_V_U64.
 * val == NULL is a pattern matrix: every stored value is 1, perm is not read and may be NULL.
 * Every Y[c, 0:k] of every column c of A is written, a column without entries as +0, whatever Y held before; nothing is
 * written at Y[c, k:ldy]: the padding is the caller's.  y must not overlap an input.
 * x and y need only the alignment of their element type.  Where x and y are 16-byte aligned, ldx and ldy are multiples
 * of 16 bytes and k is a multiple of 16 bytes of values, a lane moves 16 bytes at a time: a faster path, not a
 * precondition.
 * Malformed input never faults.  An entry whose perm[q] lies outside [0, nnz) contributes nothing and val is never
 * loaded through it; an entry whose row[q] lies outside [0, n) contributes nothing and x is never loaded through it;
 * col_ptr is treated as sbmm.h treats row_ptr (bounds clamped to [0, nnz], a decreasing pair is an empty column, every
 * entry is added to one column at most, no access leaves the arrays).
 * Refused before any array is read:
 *   - n, m, nnz or k negative; ldx < k or ldy < k; nnz > 0 with m == 0; a NULL pointer (col_ptr where m > 0, row where
 *     nnz > 0, perm where nnz > 0 and val is not NULL, x where n > 0 and nnz > 0, y where m > 0); SBX_V_NONE or an unknown
 *     value type; an unknown index type: SBX_ERR_BAD_ARG.
 *   - k > 2^20, nnz >= 2^42: SBX_ERR_UNSUPPORTED.
 * The message names the argument.  k == 0 and m == 0 are SBX_OK and write nothing.
 * Asynchronous: no read-back; Y is complete in stream order, as sbx.h defines it. */
int sbmt_csr_spmm_t(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, int64_t k,
                    const void *col_ptr, const void *row, const void *perm, const void *val,
                    const void *x, int64_t ldx, void *y, int64_t ldy);

#ifdef __cplusplus
}
#endif
#endif /* SBMT_H_ */
