/*
 * sbsm.h — C ABI of the row softmax over the stored values of a CSR matrix, forward and backward: the step between the
 * edge scores of an attention-style graph model (sbdd.h: out = val (.) (U V^T)) and the aggregation they weight (sbmm.h:
 * Y = A X).  With a pattern it is the row normalisation D^-1 A.
 *
 *   sbsm_csr_row_softmax            out[p] = exp(val[p] - m_i) / s_i,  m_i = max of row i's values, s_i = sum of its exps
 *   sbsm_csr_row_softmax_backward   dz[p] = s[p] * (g[p] - d_i),       d_i = sum over row i of s[q] * g[q]
 *
 * A header of its own, as sbx_text.h, sbx_stats.h, sbio.h, sbgr.h, sbhg.h, sbfx.h, sbsym.h, sbmv.h, sbmm.h and sbdd.h
 * are: the other headers and their versions do not change when this one does.  The entry points of this header carry the
 * prefix `sbsm_`.  They live in the same library and work on the same handle, arena and stream.  The conventions are
 * those of sbx.h: device pointers, nothing allocated and handed back, scratch from the handle's arena, work enqueued on
 * the handle's stream, sbx_status return codes, sbx_last_error text for every refusal.
 *
 * Neither call takes the columns or the number of columns: the operation never looks at a column.
 *
 * Scratch.  Nothing per row and nothing per entry.  With T = ceil(nnz / 2048) spans of 2048 stored entries:
 * (T + 1) * 8 bytes (the first row of every span and one more) and, per span, two slots of 8 bytes (a row), 4 bytes (an
 * offset into the span) and one value (a sum) each; the forward with values adds one more value per slot (a maximum).
 * That is (T + 1) * 8 + T * (24 + 4 V) bytes for the forward with values and (T + 1) * 8 + T * (24 + 2 V) bytes for the
 * pattern form and the backward, V the size of a value, plus at most 256 bytes of the arena's rounding for each of the
 * five (four) arrays.  None where nnz == 0.
 *
 * Index types.  `it` selects the width of row_ptr alone: SBX_I32 reads 32-bit offsets, SBX_I64 and SBX_I32_N64 read the
 * same 64-bit offsets.  Rows and positions are 64-bit inside and nothing is narrowed into scratch.  nnz < 2^42 (beyond it
 * SBX_ERR_UNSUPPORTED).  Tested up to n = 70 000 rows and nnz = 648 558 entries in every tuple, with rows
 * of 1 to 70 000 entries; timed at n = 2^22 with nnz = 105 M under SBX_I32 with f32 values (tools/softmax_probe.py).
 *
 * One pair per row.  There is one (m_i, s_i) per row, however many spans the row crosses, and every entry of the row is
 * exp(val[p] - m_i) / s_i from that pair: two entries of one row with equal values get equal bits.  exp is the device
 * library's expf (not the fast intrinsic), the division is the correctly rounded one.
 *
 * Special values of the forward.  -inf is the mask value: a -inf entry gets +0, and a row whose entries are all -inf gets
 * +0 everywhere (not NaN).  A row that holds a NaN or a +inf gets NaN in every entry (inf - inf and exp(NaN) reach s_i);
 * no other row is affected.  Finite values of any magnitude never overflow: every exponent is <= 0, a row of two entries
 * 3e38 gives 0.5 and 0.5, a difference beyond the type's range is -inf and its entry +0.  val == NULL is a pattern: every
 * stored value is equal, out[p] = 1 / len_i, and no exp is evaluated (exact while len_i <= 2^24).
 * The backward has no rules beyond IEEE's: d_i is built from fused multiply-adds, then dz[p] is one subtraction and one
 * product.
 *
 * Determinism.  There is no atomic and every out[p] / dz[p] is written exactly once: the same arrays give the same bits
 * on every call, handle and stream.  m_i does not depend on any order.  The order in which s_i and d_i are added is a
 * function of where the row's entries lie in the entry array (which spans, which groups of 8 inside a span), and of
 * nothing else; DESIGN §4.26 writes it down.  It is not left to right, and it is not independent of the position.
 *
 * Malformed input never faults.  The row of an entry is found as sbmv_csr_spmv finds it: the first rows of the spans,
 * each clamped to [0, n - 1], then a search between them; with a row_ptr that is not a non-decreasing sequence from 0 to
 * nnz, which row an entry is given is unspecified, but it is a row in [0, n - 1], no access leaves the arrays and every
 * out[p] is still written, once.  A caller that wants a refusal instead calls sbmv_csr_check (sbmv.h) once: there is no
 * second checker.
 *
 * Out of scope: a temperature or scale factor, LeakyReLU or any other fused activation, log-softmax, a softmax over the
 * columns, 2-byte value types, f64 (SBX_ERR_UNSUPPORTED until it is built: DESIGN 4.26), CSC and COO inputs, sharded matrices, a fused SDDMM -> softmax -> SpMM kernel.
 */
#ifndef SBSM_H_
#define SBSM_H_

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBSM_VERSION 100 /* 1.0.0 */

/* The softmax of every row's stored values.  row_ptr: n + 1 offsets at the width `it` selects, val: nnz values or NULL
 * (a pattern: out[p] = 1 / len_i), out: nnz values; val and out are of type vt: SBX_V_F32.
 * Every out[p], 0 <= p < nnz, is written once, whatever out held before, and nothing else is written.  out == val (the
 * same pointer exactly) is legal; any other overlap is the caller's error.  n == 0 (then nnz == 0) and nnz == 0 are
 * SBX_OK and write nothing.
 * Refused before any array is read:
 *   - n or nnz negative; nnz > 0 with n == 0; a NULL row_ptr where n > 0; a NULL out where nnz > 0; SBX_V_NONE or an
 *     unknown value type; an unknown index type: SBX_ERR_BAD_ARG.
 *   - SBX_V_F64 (not built yet) or an integer value type; nnz >= 2^42: SBX_ERR_UNSUPPORTED.
 * The message names the argument.
 * Asynchronous: no read-back; out is complete in stream order, as sbx.h defines it. */
int sbsm_csr_row_softmax(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t nnz,
                         const void *row_ptr, const void *val, void *out);

/* The backward of the call above.  s: the nnz values the forward wrote, g: the nnz gradients with respect to them, dz:
 * nnz values, the gradient with respect to val; all of type vt: SBX_V_F32.
 * Every dz[p] is written once.  dz == g (the same pointer exactly) is legal; any other overlap is the caller's error.
 * Refused as above, and a NULL s or g where nnz > 0: SBX_ERR_BAD_ARG.
 * Asynchronous: no read-back; dz is complete in stream order. */
int sbsm_csr_row_softmax_backward(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t nnz,
                                  const void *row_ptr, const void *s, const void *g, void *dz);

#ifdef __cplusplus
}
#endif
#endif /* SBSM_H_ */
