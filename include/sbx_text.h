/*
 * sbx_text.h — C ABI of the text OUTPUT path: a COO on the device to Matrix Market / edge-list text on the device.
 *
 * The counterpart of the parsers of sbx.h (sbx_mtx_parse_coordinate, sbx_edge_list_parse) for the reference's two text
 * writers, io/mtx_writer.cc (MTXWriter) and io/edge_list_writer.cc (EdgeListWriter).  Both write one `ofstream <<` per
 * token there; MTXWriter checks the symmetry with a double loop over the entries and EdgeListWriter sorts and
 * deduplicates on the host.  Here that is a sort, a search and a formatting pass on the device.
 *
 * A header of its own with a version of its own: sbx.h and SBX_VERSION do not change when the text path does.  The
 * conventions are those of sbx.h: device pointers unless the name ends in `_host`, nothing allocated and handed back,
 * scratch from the handle's arena, work enqueued on the handle's stream, sbx_status return codes, SBX_I32_N64 treated
 * as SBX_I32 (no entry point here takes an offset array).
 *
 * Numbers print as `ostream <<` prints them:
 *   SBX_V_I32 / SBX_V_I64   signed decimal          SBX_V_U32 / SBX_V_U64   unsigned decimal
 *   SBX_V_F32 / SBX_V_F64   what printf("%.*g", precision, (double)x) gives under glibc, which is what the stream
 *                           prints at its default precision 6 (a float widens to double exactly): the exact value
 *                           rounded once, half to even, to `precision` significant digits; fixed notation when the
 *                           decimal exponent X after rounding has -4 <= X < precision, else d[.ddd]e+-XX with at least
 *                           two exponent digits; trailing zeros and a bare point stripped; 0, -0, inf, -inf, nan, and
 *                           -nan for a NaN whose sign bit is set.  precision is 1..17 (else SBX_ERR_BAD_ARG): 9 / 17
 *                           read back bit-identical through sbx_mtx_parse_coordinate, which the reference's writers
 *                           have no way to ask for.  The conversion is exact integer arithmetic (csrc/sbx_bin2dec.h).
 *   indices                 signed decimal of id + index_base
 *
 * The formatters (sbx_text_format_*) share one protocol:
 *   - text_out == NULL is the sizing call: *bytes_host receives the exact length, nothing is written;
 *   - otherwise capacity < length is SBX_ERR_BAD_ARG with nothing written (*bytes_host still receives the length);
 *   - not one byte at or beyond the length is touched;
 *   - lengths and offsets are 64-bit (the text may exceed 2^32 bytes); one call takes fewer than 2^32 entries;
 *   - a caller may pass any sub-range of the entries by offsetting the pointers: the concatenated chunk outputs are the
 *     output of the whole (that is how the host layer bounds its device text and its pinned staging);
 *   - synchronous (the length is read back); the text is complete in stream order.
 */
#ifndef SBX_TEXT_H_
#define SBX_TEXT_H_

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBX_TEXT_VERSION 100 /* 1.0.0 */

/* ------------------------------------------------------------------ *
 * the values of an array, one per line                                *
 * io/mtx_writer.cc:248-256 (array format of a COO), :399-407 (WriteArray)
 * ------------------------------------------------------------------ */
/* `count` lines "<value>\n".  vt must not be SBX_V_NONE.  Synchronous. */
int sbx_text_format_values(sbx_handle_t h, sbx_value_type vt, int64_t count, const void *vals, int precision,
                           void *text_out, int64_t capacity, int64_t *bytes_host);

/* ------------------------------------------------------------------ *
 * coordinate lines                                                    *
 * io/mtx_writer.cc:261-352 (coordinate section), io/edge_list_writer.cc:52-54, :92-97
 * ------------------------------------------------------------------ */
/* One line per KEPT entry, in input order: "<row + index_base> <col + index_base>", then " <value>" when
 * vt != SBX_V_NONE and val != NULL and SBX_TEXT_PATTERN is not set, then "\n".
 *   SBX_TEXT_LOWER          keeps the entries with col <= row (:287-340: what a symmetric file stores)
 *   SBX_TEXT_NO_DIAGONAL    drops the entries with col == row (with SBX_TEXT_LOWER: col < row, a skew-symmetric file)
 *   SBX_TEXT_PATTERN        drops the value even when val is given (field "pattern")
 * Unknown flag bits are SBX_ERR_BAD_ARG.  The ids are not checked against a dimension (none is given), as in the
 * reference.  Synchronous. */
#define SBX_TEXT_LOWER 1u
#define SBX_TEXT_NO_DIAGONAL 2u
#define SBX_TEXT_PATTERN 4u
int sbx_text_format_coordinate(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t nnz, const void *row,
                               const void *col, const void *val, int64_t index_base, int precision, unsigned flags,
                               void *text_out, int64_t capacity, int64_t *bytes_host);

/* ------------------------------------------------------------------ *
 * the symmetry check of MTXWriter::WriteCOO                           *
 * io/mtx_writer.cc:116-186                                            *
 * ------------------------------------------------------------------ */
/* result_host[0]: 1 iff every entry (i, j, v) with i != j has SOME entry (j, i, w) that passes the value test, else 0
 *                 (the reference throws "Matrix is not symmetric!" at the first entry without one, :166);
 * result_host[1]: the number of entries with i == j (count_diagonal);
 * result_host[2]: the number of those whose value is != 0 (is_diagonal_all_zero is result_host[2] == 0).
 * Value test: skew == 0: w == v; skew != 0: w == -v (two's-complement wrap for the integer types, as the C++
 * expression).  vt == SBX_V_NONE or val == NULL: coordinates only — and with skew != 0 nothing matches, as in the
 * reference (:127-130, "pattern cannot be skew-symmetric").  The comparisons are the C++ ones: -0 == +0, a NaN equals
 * nothing (and is != 0).  The entries may come in any order and hold duplicates; if they are not (row, col)-sorted a
 * scratch copy is sorted to search in — the caller's arrays are never modified.  n is the (square) dimension.
 * Deliberate divergences:
 *   - an id outside [0, n) is SBX_ERR_BAD_ARG (the reference compares whatever is there);
 *   - the reference's count_symmetric (the number of matched entries) is nnz - result_host[1] whenever
 *     result_host[0] is 1, which is the only case the reference uses it in; it is not returned;
 *   - counts are 64-bit (the reference loops over int).
 * Quadratic in nnz in the reference; here a sort and one binary search per entry.  Synchronous. */
int sbx_coo_symmetry_check(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t nnz,
                           const void *row, const void *col, const void *val, int skew, int64_t *result_host);

/* ------------------------------------------------------------------ *
 * the undirected edge list of EdgeListWriter                          *
 * io/edge_list_writer.cc:26-51 (:58-90 weighted; :104-190 the CSR twins)
 * ------------------------------------------------------------------ */
/* In place: every entry swapped so that row <= col, the entries sorted by (row, col), the first of every run of equal
 * coordinates kept; *nnz_host receives how many are left (the arrays' tails are unspecified).
 * Deliberate divergences:
 *   - the sort is stable, so the weight that survives is that of the first duplicate in input order; the reference's
 *     std::sort leaves it unspecified (the divergence sbx_edge_list_parse documents for the reader);
 *   - a negative id is SBX_ERR_BAD_ARG; ids of 2^31 and more need SBX_I64, where the bits of the largest id, twice,
 *     must fit the 64-bit key of sbx_coo_sort (SBX_ERR_UNSUPPORTED beyond); nnz must be below 2^31.
 * Synchronous. */
int sbx_coo_undirected_unique(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t nnz, void *row, void *col,
                              void *val, int64_t *nnz_host);

/* ------------------------------------------------------------------ *
 * the array format of a COO                                           *
 * io/mtx_writer.cc:213-259                                            *
 * ------------------------------------------------------------------ */
/* n * m lines in column-major order: line c * n + r holds the value stored at (r, c), "0" where nothing is stored.
 * vt == SBX_V_NONE or val == NULL: every line is "0", as in the reference (:222-233).  The protocol of the
 * formatters above.
 * Deliberate divergences:
 *   - the reference walks the entries with one cursor and misaligns every later line after a duplicate coordinate
 *     (and prints nothing sensible for entries that are not column-major sorted); here the entries may come in any
 *     order and a duplicate coordinate is SBX_ERR_BAD_ARG;
 *   - an id outside [0, n) x [0, m) is SBX_ERR_BAD_ARG;
 *   - n * m >= 2^31 is SBX_ERR_UNSUPPORTED (a dense text of that size is no use to anybody).
 * Synchronous. */
int sbx_text_format_dense(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz,
                          const void *row, const void *col, const void *val, int precision, void *text_out,
                          int64_t capacity, int64_t *bytes_host);

#ifdef __cplusplus
}
#endif
#endif /* SBX_TEXT_H_ */
