/*
 * sbdd.h — C ABI of the sampled dense-dense product on the pattern of a CSR matrix A (n x m), with dense row-major
 * U (n x k) and V (m x k): the third of the products that read a sparse matrix against dense data, after y = A x (sbmv.h)
 * and Y = A X (sbmm.h).  It is the gradient of Y = A X with respect to A's values (U = dY, V = X), the edge score of an
 * attention-style graph model, and the "sample a low-rank product on a sparsity pattern" step of a factorization.
 *
 *   sbdd_csr_sddmm    out[p] = val[p] * sum over j < k of U[row(p)*ldu + j] * V[col[p]*ldv + j], for every stored entry p
 *
 * A header of its own, as sbx_text.h, sbx_stats.h, sbio.h, sbgr.h, sbhg.h, sbfx.h, sbsym.h, sbmv.h and sbmm.h are: the
 * other headers and their versions do not change when this one does.  The entry point of this header carries the prefix
 * `sbdd_`.  It lives in the same library and works on the same handle, arena and stream.  The conventions are those of
 * sbx.h: device pointers unless the name ends in `_host`, nothing allocated and handed back, scratch from the handle's
 * arena, work enqueued on the handle's stream, sbx_status return codes, sbx_last_error text for every refusal.
 *
 * Scratch.  Nothing per row, nothing per entry and nothing that grows with k: the first row of every span of 2048 stored
 * entries (the last one may be shorter) and one more, that is (ceil(nnz / 2048) + 1) * 8 bytes, plus at most 256 bytes of
 * the arena's rounding of that one array.  None where nnz == 0 or k == 0.
 *
 * Index types.  All three tuples read their arrays at their own width; rows, columns and positions are 64-bit inside and
 * nothing is narrowed into scratch.  No limit is added to what the tuple can express up to nnz < 2^42 and k <= 2^20
 * (beyond them SBX_ERR_UNSUPPORTED).  Tested up to n = 70 000 rows, m = 70 000 columns, nnz = 648 558 entries and
 * k = 513 under SBX_I32 with f32 values, and up to n = m = 8192, nnz = 648 558 and k = 260 in every other tuple and value
 * type; timed at n = m = 2^22 with nnz = 105 M under SBX_I32 (tools/sddmm_probe.py).
 *
 * The value.  The dot product is summed first, from +0, in the value type; out[p] is then the one IEEE product
 * val[p] * dot, so a negative val[p] times a zero dot is -0, and for a pattern out[p] is the dot itself.  A dot that is
 * exactly zero is +0.  Integer value types are added and multiplied modulo 2^32 or 2^64; the signed and the unsigned
 * enumerator of a width are the same computation.
 *
 * The order of the sum.  With VEC = 16 / sizeof(value) columns per lane in the 16-byte form and VEC = 1 otherwise,
 * L = ceil(k / VEC) lanes cover the k columns (k is a multiple of VEC in the 16-byte form).
 *   - L <= 64: lane l holds the columns l * VEC ... l * VEC + VEC - 1 and adds their products to +0 in ascending order
 *     of the column: s = ((0 + u0 v0) + u1 v1) + ...
 *   - L > 64: lane l (0 <= l < 64) holds, of every block b = 0 ... ceil(L / 64) - 1, the columns (b * 64 + l) * VEC ...
 *     + VEC - 1 that lie below k, and adds their products to the same sum s, block after block, ascending inside a block.
 *   - The lanes are then added by a butterfly over G lanes, G the power of two >= L (64 where L > 32), the lanes from L
 *     on holding +0: in step d = 1, 2, 4, ... G / 2, lane i becomes s[i] + s[i ^ d] (both partners compute the same
 *     commutative sum).  Written as a tree: the dot is T(0, G) with T(i, 1) = s[i] and T(i, w) = T(i, w / 2) +
 *     T(i + w / 2, w / 2).
 * For the float types every step s + u v is one fused multiply-add (one rounding), written out as such in both forms: it
 * is not left to the compiler, and it is the same for every entry.
 *
 * Determinism and position independence.  There is no atomic, and every out[p] is written exactly once.  out[p] is a
 * function of val[p], the k values of U's row, the k values of V's row, k, and the form (16 bytes or one column per
 * lane) that the alignment selects.  It is NOT a function of p, of the length of the row, of where the entry lies in a
 * span, of the index tuple, of the handle or of the stream: two stored entries with the same row, column and value get
 * the same bits, and the same entry of a permuted matrix with U and V permuted alike gets the same bits.
 *
 * Malformed input never faults.  An entry whose column lies outside [0, m) gets out[p] = +0 and nothing is loaded from
 * V for it.  The row of an entry is found as sbmv_csr_spmv and sbmm_csr_spmm find it: the first rows of the spans, each
 * clamped to [0, n - 1], then a search between them; with a row_ptr that is not a non-decreasing sequence from 0 to nnz,
 * which row an entry is given is unspecified, but it is a row in [0, n - 1], no access leaves the arrays and every
 * out[p] is still written.  A caller that wants a refusal instead calls sbmv_csr_check (sbmv.h) once: there is no
 * second checker.
 *
 * Out of scope: out = alpha val (U V^T) + beta out and accumulation into out, column-major U or V, 2-byte value types,
 * CSC and COO patterns, sharded matrices.  (The gradient with respect to V is a product with the transpose: sbmt.h.)
 */
#ifndef SBDD_H_
#define SBDD_H_

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBDD_VERSION 100 /* 1.0.0 */

/* out = val (.) (U V^T) on the pattern.  row_ptr: n + 1 offsets, col: nnz columns, val: nnz values or NULL, u: n rows
 * of k values at a leading dimension of ldu elements, v: m rows of k values at a leading dimension of ldv elements, out:
 * nnz values; val, u, v and out are of type vt: SBX_V_F32, SBX_V_F64, SBX_V_I32 / SBX_V_U32 or SBX_V_I64 / SBX_V_U64.
 * val == NULL is a pattern matrix: every stored value is 1.
 * Every out[p], 0 <= p < nnz, is written, whatever out held before.  out must not overlap an input.  k == 0 writes +0
 * everywhere (an empty sum is 0); n == 0 (then nnz == 0) and nnz == 0 are SBX_OK and write nothing.
 * u, v and out need only the alignment of their element type: a slice that begins at an odd element offset is legal.
 * Where u and v are 16-byte aligned, ldu and ldv are multiples of 16 bytes and k is a multiple of 16 bytes of values, a
 * lane moves 16 bytes at a time; that is a faster path, not a precondition.
 * Refused before any array is read:
 *   - n, m, nnz or k negative; ldu < k or ldv < k; nnz > 0 with n == 0; a NULL pointer (row_ptr where n > 0, col or out
 *     where nnz > 0, u or v where nnz > 0 and k > 0); SBX_V_NONE or an unknown value type; an unknown index type:
 *     SBX_ERR_BAD_ARG.
 *   - k > 2^20, nnz >= 2^42: SBX_ERR_UNSUPPORTED.
 * The message names the argument.
 * Asynchronous: no read-back; out is complete in stream order, as sbx.h defines it. */
int sbdd_csr_sddmm(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, int64_t k,
                   const void *row_ptr, const void *col, const void *val, const void *u, int64_t ldu, const void *v,
                   int64_t ldv, void *out);

#ifdef __cplusplus
}
#endif
#endif /* SBDD_H_ */
