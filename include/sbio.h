/*
 * sbio.h — C ABI of the dense side of the Matrix Market path: what the reference's MTXReader does for array-format
 * files and for ReadArray (io/mtx_reader.cc:121-166 ReadArrayIntoCOO, :265-305 ReadCoordinateIntoArray, :496-539
 * ReadArrayIntoArray) in `fin >> w` loops on the host.
 *
 * A header of its own, as sbx_text.h and sbx_stats.h are: sbx.h, sbx_text.h and sbx_stats.h and their versions do not
 * change when this one does.  The `sbx` prefix is closed (every export that begins with `sbx` is declared in one of
 * those three headers, and the tests hold each to its table): the entry points of this header carry the prefix
 * `sbio_`.  They live in the same library and work on the same handle, arena and stream.  The conventions are those
 * of sbx.h: device pointers unless the name ends in `_host`, nothing allocated and handed back, scratch from the
 * handle's arena, work enqueued on the handle's stream, sbx_status return codes, SBX_I32_N64 taken as SBX_I32 (there
 * is no offset array here).
 */
#ifndef SBIO_H_
#define SBIO_H_

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBIO_VERSION 100 /* 1.0.0 */

/* ------------------------------------------------------------------ *
 * the value section of an array-format file                            *
 * io/mtx_reader.cc:141-143, :522-526 (`fin >> w`, total_values times)  *
 * ------------------------------------------------------------------ */
/* `text_dev` holds the `bytes` bytes behind the size line.  The first `count` whitespace-separated tokens are parsed
 * as values of type `vt`, in file order, into val_out[0 .. count).  Tokenization, integer parsing and the exact
 * decimal -> float / double conversion are those of sbx_mtx_parse_coordinate: the bits are what strtof / strtod give.
 * Tokens behind the first `count` are ignored, as the reference ignores them.
 *   - fewer than `count` tokens: SBX_ERR_BAD_ARG (the reference repeats the last value it read);
 *   - a malformed token (hex, inf / nan, garbage, a '.' in an integer type, an integer out of range):
 *     SBX_ERR_BAD_ARG (the reference's stream fails and every later value is stale);
 *   - more than 38 significant digits with a non-zero tail: SBX_ERR_UNSUPPORTED;
 *   - vt == SBX_V_NONE: SBX_ERR_BAD_ARG;  bytes >= 4 GiB: SBX_ERR_BAD_ARG (32-bit token offsets).
 * Synchronous: the token count and the status word are read back. */
int sbio_mtx_parse_values(sbx_handle_t h, sbx_value_type vt, const void *text_dev, int64_t bytes, int64_t count,
                          void *val_out);

/* ------------------------------------------------------------------ *
 * dense, column-major -> COO in (row, col) order                      *
 * io/mtx_reader.cc:141-165 and the COO constructor's sort behind it    *
 * ------------------------------------------------------------------ */
/* `dense` is an n x m matrix in column-major order, cell (r, c) at dense[c * n + r]: the layout of the array format.
 * The cells with value != 0 (the C++ comparison: -0.0 is dropped like +0, a NaN is kept) come out as a COO ordered by
 * (row, col), the order the COO constructor's sort leaves: its is-sorted check passes and no sort runs.
 *   - row_out == NULL: count mode, only *nnz_host is written;
 *   - otherwise capacity < nnz is SBX_ERR_BAD_ARG (and nothing is written); val_out may be NULL (coordinates only);
 *   - `it` selects 32- or 64-bit words in row_out / col_out;
 *   - n * m >= 2^31: SBX_ERR_UNSUPPORTED (the limit of sbx_text_format_dense); n == 0 or m == 0 gives 0 entries;
 *   - vt == SBX_V_NONE: SBX_ERR_BAD_ARG.
 * Synchronous: nnz is read back; the kernel that fills the outputs is enqueued behind that, and they are complete in
 * stream order. */
int sbio_dense_to_coo(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, const void *dense,
                      int64_t capacity, void *row_out, void *col_out, void *val_out, int64_t *nnz_host);

/* ------------------------------------------------------------------ *
 * sorted COO of a 1 x N or N x 1 matrix -> dense vector                *
 * io/mtx_reader.cc:296-301                                             *
 * ------------------------------------------------------------------ */
/* out[0 .. len) is zero-filled, then out[row[k] + col[k]] = val[k] for 0 <= k < nnz.  The COO is sorted, so equal
 * positions are adjacent: an entry writes only if its successor has another position — the last of a run wins, as in
 * the reference's loop, and the result does not depend on the launch.
 *   - row[k] + col[k] outside [0, len): SBX_ERR_BAD_ARG (the reference writes out of bounds there); the contents of
 *     `out` are unspecified then;
 *   - vt == SBX_V_NONE: SBX_ERR_BAD_ARG.
 * Synchronous: the range check is read back. */
int sbio_coo_to_dense_vector(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t len, int64_t nnz,
                             const void *row, const void *col, const void *val, void *out);

#ifdef __cplusplus
}
#endif
#endif /* SBIO_H_ */
