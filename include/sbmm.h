/*
 * sbmm.h — C ABI of the sparse matrix times dense block product Y = A X of a CSR matrix A (n x m) and a dense row-major
 * X (m x k): the product of sbmv.h for k right-hand sides at once, the form in which a graph's adjacency meets a block of
 * features, and the one in which an ordering's locality pays most (every stored entry gathers one contiguous row of X).
 *
 *   sbmm_csr_spmm    Y[i*ldy + j] = sum of val[p] * X[col[p]*ldx + j] over the stored entries p of row i, 0 <= j < k
 *
 * A header of its own, as sbx_text.h, sbx_stats.h, sbio.h, sbgr.h, sbhg.h, sbfx.h, sbsym.h and sbmv.h are: the other
 * headers and their versions do not change when this one does.  The entry point of this header carries the prefix
 * `sbmm_`.  It lives in the same library and works on the same handle, arena and stream.  The conventions are those of
 * sbx.h: device pointers unless the name ends in `_host`, nothing allocated and handed back, scratch from the handle's
 * arena, work enqueued on the handle's stream, sbx_status return codes, sbx_last_error text for every refusal.
 *
 * Scratch.  Nothing per row and nothing that grows with nnz * k: for every span of 2048 stored entries (the last one may
 * be shorter) 16 bytes and one partial row of k values, that is ceil(nnz / 2048) * (16 + k * sizeof(value)) bytes, plus
 * at most 1 KiB (8 bytes and the arena's rounding of three arrays).  None where nnz == 0.
 *
 * Index types.  All three tuples read their arrays at their own width; rows, columns and positions are 64-bit inside and
 * nothing is narrowed into scratch.  No limit is added to what the tuple can express up to nnz < 2^42 and k <= 2^20
 * (beyond them SBX_ERR_UNSUPPORTED).  Tested up to n = 70 000 rows, m = 70 000 columns, nnz = 648 558 entries and
 * k = 513 under SBX_I32 with f32 values, and up to n = m = 8192, nnz = 648 558 and k = 260 in every other tuple and value
 * type; timed at n = m = 2^22 with nnz = 105 M under SBX_I32 (tools/spmm_probe.py).
 *
 * Determinism.  The same arrays and the same k give the same bits in Y on every call, handle and stream: there is no
 * floating-point atomic and no sum whose order depends on which wave arrives first.  The order in which the products of
 * a row are added is a function of where the row's entries lie in the array of the stored entries and of k (with the
 * alignment of x and y and ldx, ldy, which choose between one column and 16 bytes of columns per lane): spans of 2048
 * entries, every span cut into as many equal runs of consecutive entries as groups of lanes fit into a wave for this k,
 * a run added left to right, the runs of a row combined by a fixed scan tree over the groups, the partial sums of a row
 * that crosses spans added in span order.  It is NOT a function of the column j, it is NOT claimed to be the
 * left-to-right sum, nor to be the order of sbmv_csr_spmv.  A floating-point sum that is exactly zero is +0.  Integer
 * value types are added and multiplied modulo 2^32 or 2^64; the signed and the unsigned enumerator of a width are the
 * same computation.
 *
 * Malformed input never faults.  An entry whose column lies outside [0, m) contributes nothing and is never loaded
 * from.  Row bounds are clamped to [0, nnz], a decreasing pair of row bounds is an empty row, and every entry is added
 * to one row at most; which Y a row_ptr that is not a non-decreasing sequence from 0 to nnz gives is otherwise
 * unspecified, but no access leaves the arrays.  A caller that wants a refusal instead calls sbmv_csr_check (sbmv.h)
 * once: there is no second checker.
 *
 * Out of scope: Y = alpha A X + beta Y, the transposed product (a header of its own: sbmt.h), column-major X or Y, CSC and
 * COO inputs, 2-byte value types, sharded matrices.
 */
#ifndef SBMM_H_
#define SBMM_H_

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBMM_VERSION 100 /* 1.0.0 */

/* Y = A X.  row_ptr: n + 1 offsets, col: nnz columns, val: nnz values or NULL, x: m rows of k values at a leading
 * dimension of ldx elements, y: n rows of k values at a leading dimension of ldy elements; val, x and y are of type vt:
 * SBX_V_F32, SBX_V_F64, SBX_V_I32 / SBX_V_U32 or SBX_V_I64 / SBX_V_U64.
 * val == NULL is a pattern matrix: every stored value is 1.
 * Every Y[i, 0:k] of every row is written, a row without entries as 0, whatever Y held before; nothing is written at
 * Y[i, k:ldy]: the padding is the caller's.  y must not overlap an input.
 * x and y need only the alignment of their element type: a slice that begins at an odd element offset is legal.  Where
 * x and y are 16-byte aligned, ldx and ldy are multiples of 16 bytes and k is a multiple of 16 bytes of values, a lane
 * moves 16 bytes at a time; that is a faster path, not a precondition.
 * Refused before any array is read:
 *   - n, m, nnz or k negative; ldx < k or ldy < k; nnz > 0 with n == 0; a NULL pointer (row_ptr where n > 0, col where
 *     nnz > 0, x where m > 0 and nnz > 0, y where n > 0: the cases of sbmv_csr_spmv); SBX_V_NONE or an unknown value
 *     type; an unknown index type: SBX_ERR_BAD_ARG.
 *   - k > 2^20, nnz >= 2^42: SBX_ERR_UNSUPPORTED.
 * The message names the argument.  k == 0 and n == 0 are SBX_OK and write nothing.
 * Asynchronous: no read-back; Y is complete in stream order, as sbx.h defines it. */
int sbmm_csr_spmm(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, int64_t k,
                  const void *row_ptr, const void *col, const void *val, const void *x, int64_t ldx, void *y, int64_t ldy);

#ifdef __cplusplus
}
#endif
#endif /* SBMM_H_ */
