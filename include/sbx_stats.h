/*
 * sbx_stats.h — C ABI of the scalar statistics of an offset array and of a block partition: what the reference's
 * feature::AvgDegree, MinDegree, MaxDegree, MinMaxAvgDegree, the seven *DegreeColumn classes (feature/avg_degree.cc,
 * min_degree.cc, max_degree.cc, min_max_avg_degree.cc, *_degree_column.cc) and feature::OffDiagBlockNNZ
 * (feature/off_diag_block_nnz.cc) compute in loops on the host.
 *
 * A header of its own, as sbx_text.h is: sbx.h and sbx_text.h, SBX_VERSION and SBX_TEXT_VERSION do not change when
 * this one does.  The `sbx_` prefix is closed (every `sbx_` export is declared in sbx.h or sbx_text.h, and the tests
 * hold both to their tables): the entry points of this header carry the prefix `sbxstat_`.  They live in the same
 * library and work on the same handle, arena and stream.  The conventions are those of sbx.h: device pointers unless
 * the name ends in `_host`, nothing allocated and handed back, scratch from the handle's arena, work enqueued on the
 * handle's stream, sbx_status return codes.
 */
#ifndef SBX_STATS_H_
#define SBX_STATS_H_

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBX_STATS_VERSION 100 /* 1.0.0 */

/* ------------------------------------------------------------------ *
 * every statistic of the degrees d_i = ptr[i + 1] - ptr[i], 0 <= i < n *
 * ------------------------------------------------------------------ */
typedef struct sbxstat_degrees {
  int64_t  count;                 /* n                                                     */
  int64_t  sum;                   /* ptr[n] - ptr[0]                                       */
  int64_t  min, max;              /* over d_i = ptr[i+1] - ptr[i], 0 <= i < n              */
  int64_t  zeros;                 /* number of i with d_i == 0                             */
  uint64_t sumsq_lo, sumsq_hi;    /* sum of d_i^2, exact, 128 bits                         */
  int64_t  median_lo, median_hi;  /* ascending order statistics (n-1)/2 and n/2            */
  double   sum_log;               /* sum over d_i > 0 of log(d_i), in double               */
} sbxstat_degrees;
#define SBXSTAT_MEDIAN 0x1u   /* fill median_lo / median_hi (else both -1) */
#define SBXSTAT_LOG    0x2u   /* fill sum_log (else 0)                     */
/* `ptr` is any offset array of n + 1 words, a CSR's row_ptr or a CSC's col_ptr: 32-bit words for SBX_I32, 64-bit
 * words for SBX_I64 and SBX_I32_N64 (there is no id array, as in sbx_csr_degree_distribution).
 *   - 1 <= n < 2^31; n == 0 is SBX_ERR_BAD_ARG (the reference reads ptr[1] there).
 *   - A decreasing ptr (some d_i < 0) is SBX_ERR_BAD_ARG, found from the signed minimum; nothing else is validated.
 *   - Degrees may be anything in [0, 2^63): sumsq carries into its high word.
 *   - The order statistics come from a radix select over 12-bit digits on the device, both ranks at once; the
 *     degrees are recomputed from ptr in every pass and never stored.
 *   - sum_log is deterministic: the same input gives the same bits on every run, handle and launch shape (fixed
 *     tiles of the array, a fixed order inside a tile and over the tiles, no floating-point atomics).
 *   - Unknown flag bits are SBX_ERR_BAD_ARG.
 * Synchronous: one read-back, at the end. */
int sbxstat_degree_stats(sbx_handle_t h, sbx_index_type it, int64_t n, const void *ptr, unsigned flags,
                         sbxstat_degrees *out_host);

/* ------------------------------------------------------------------ *
 * nonzeros outside the diagonal blocks of a block partition           *
 * feature/off_diag_block_nnz.cc:94-116                                *
 * ------------------------------------------------------------------ */
/* The rows are cut into block_rows (h) contiguous blocks and the columns into block_cols (w); every product below is
 * taken in 64 bits.  For p in [0, h):
 *   rs_p = min(n, p * (n / h) + min(p, n % h)),  re_p the same with p + 1,
 *   cs_p = min(m, p * (m / w) + min(p, m % w)),  ce_p the same with p + 1,
 * and *count_host receives the number of entries in rows [rs_p, re_p) whose column is below cs_p or at least ce_p,
 * summed over p.  What follows from the rule and is kept:
 *   - h <= 0 gives 0; w <= 0 with h > 0 is SBX_ERR_BAD_ARG (the reference divides by zero);
 *   - for p >= w the column range is empty: every entry of those rows counts;
 *   - columns outside [0, m) always count;
 *   - the count is exact in 64 bits (the reference's counter is an IDType).
 * All three index tuples; under SBX_I32_N64 the offsets are 64-bit and the columns 32-bit.  `nnz` is the length of
 * `col`: positions of row_ptr at or beyond it are not read.  n < 2^31 - 1.  Synchronous. */
int sbxstat_csr_off_diag_block_nnz(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t m, int64_t nnz,
                                   const void *row_ptr, const void *col, int64_t block_rows, int64_t block_cols,
                                   int64_t *count_host);

#ifdef __cplusplus
}
#endif
#endif /* SBX_STATS_H_ */
