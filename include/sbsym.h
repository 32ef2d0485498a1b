/*
 * sbsym.h — C ABI of the pattern symmetrization of a square CSR: B = A ∪ Aᵀ, what MATLAB's symrcm, SciPy's
 * reverse_cuthill_mckee(symmetric_mode=False) and HSL MC60 order when a matrix is not structurally symmetric, and what
 * turns a directed edge list into the undirected graph the graph features and the partition-file writers expect.
 * sbx_rcm_reorder (sbx.h) refuses a structurally unsymmetric pattern; a caller symmetrizes first with this header.
 *
 *   sbsym_csr_missing_mirrors   how many entries A lacks to be structurally symmetric (0: it is)
 *   sbsym_csr_symmetrize        B: every stored entry of A plus one entry for every missing mirror
 *
 * A header of its own, as sbx_text.h, sbx_stats.h, sbio.h, sbgr.h, sbhg.h and sbfx.h are: the other headers and their
 * versions do not change when this one does.  The entry points of this header carry the prefix `sbsym_`.  They live in
 * the same library and work on the same handle, arena and stream.  The conventions are those of sbx.h: device pointers
 * unless the name ends in `_host`, nothing allocated and handed back, scratch from the handle's arena (32 bytes per
 * stored entry plus 16 per row), work enqueued on the handle's stream, sbx_status return codes, sbx_last_error text for
 * every refusal.
 *
 * The matrix.  A is n x n, its rows column-sorted (non-decreasing) as the CSR constructor leaves them; duplicates are
 * allowed.  Values are opaque 0-, 4- or 8-byte payloads: they are copied, never added or compared.
 *
 * B.  Row i of B holds every stored entry of A's row i verbatim — duplicates too, in stored order, with their values —
 * and, for every DISTINCT (j, i) stored in A with j != i whose mirror (i, j) is not stored, one entry with column j that
 * carries the value of the FIRST stored (j, i).  The rows of B are column-sorted.  `added` is the number of such
 * entries, and it is exactly what sbsym_csr_missing_mirrors returns.
 *
 * Refusals found on the device (SBX_ERR_BAD_ARG, before any search uses the offending id, never a fault; no output
 * array is written): a column outside [0, n); a row whose columns decrease; row_ptr[0] != 0 or row_ptr[n] != nnz.
 *
 * Limits, for every index tuple (ids, offsets and positions are 32-bit inside): n < 2^31 - 1, nnz < 2^31 and
 * nnz_out < 2^31; beyond them SBX_ERR_UNSUPPORTED, the message names the count.
 *
 * Stream order.  Both entry points are synchronous for their status and their `_host` counts, with one read-back each.
 * The output arrays of sbsym_csr_symmetrize are written by kernels enqueued behind that read-back: they are complete in
 * stream order, as sbx.h defines it, and not necessarily when the call returns.
 */
#ifndef SBSYM_H_
#define SBSYM_H_

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBSYM_VERSION 100 /* 1.0.0 */

#define SBSYM_NO_DIAGONAL        1u  /* drop stored (i, i) entries from the output */
#define SBSYM_SKIP_IF_SYMMETRIC  2u  /* nothing missing and nothing dropped: leave the outputs untouched, *added_host = 0 */

/* *missing_host = the number of distinct off-diagonal (j, i) stored in A whose mirror (i, j) is not stored.
 * A structurally symmetric A takes a fast path: its transposed key sequence equals its own, one streaming comparison
 * finds that and no search runs.
 *   - n or nnz negative, nnz > 0 with n == 0, a NULL pointer (row_ptr where n > 0, col where nnz > 0, missing_host), an
 *     unknown index type: SBX_ERR_BAD_ARG.
 * Synchronous: one read-back. */
int sbsym_csr_missing_mirrors(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t nnz,
                              const void *row_ptr, const void *col, int64_t *missing_host);

/* B = A ∪ Aᵀ into (row_ptr_out: n + 1 offsets, col_out and val_out: out_capacity entries).
 *   *added_host   = the entries added (what sbsym_csr_missing_mirrors returns)
 *   *nnz_out_host = nnz + added, minus the stored diagonal entries under SBSYM_NO_DIAGONAL
 * Either `_host` pointer may be NULL.  `val` and `val_out` are read and written when vt != SBX_V_NONE.
 * With col_out == NULL the call only counts: row_ptr_out is written if given, and both counts are set.
 * With SBSYM_SKIP_IF_SYMMETRIC and nothing to add and nothing to drop no output array is touched (the caller goes on with
 * A); without the flag B is then a copy of A.
 * The outputs must not overlap the inputs.
 *   - the refusals of sbsym_csr_missing_mirrors; an unknown flag or value type; vt != SBX_V_NONE with a NULL val (nnz > 0)
 *     or a NULL val_out beside a col_out: SBX_ERR_BAD_ARG.
 *   - col_out given and out_capacity < nnz_out: SBX_ERR_BAD_ARG, the message names the count needed, both counts are set
 *     and no output array is written.
 * Synchronous for the status and both counts: one read-back; the arrays are complete in stream order. */
int sbsym_csr_symmetrize(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t nnz,
                         const void *row_ptr, const void *col, const void *val, unsigned flags,
                         int64_t out_capacity, void *row_ptr_out, void *col_out, void *val_out,
                         int64_t *nnz_out_host, int64_t *added_host);

#ifdef __cplusplus
}
#endif
#endif /* SBSYM_H_ */
