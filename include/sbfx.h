/*
 * sbfx.h — C ABI of the fused feature classes: what feature::Extractor (the host layer's feature/extractor.h) picks when
 * several features of one matrix are asked for at once.  Each entry point computes in one pass what two entry points of
 * sbx.h compute in two:
 *
 *   sbfx_csr_degrees_degree_distribution   sbx_csr_degrees + sbx_csr_degree_distribution
 *                                          (the reference's Degrees_DegreeDistribution::GetCSR,
 *                                          feature/degrees_degree_distribution.cc:146-164)
 *   sbfx_csr_bandwidth_profile             sbx_csr_bandwidth + sbx_csr_profile (a fused class of this project's own)
 *
 * A header of its own, as sbx_text.h, sbx_stats.h, sbio.h, sbgr.h and sbhg.h are: the other headers and their versions do
 * not change when this one does.  The entry points of this header carry the prefix `sbfx_`.  They live in the same
 * library and work on the same handle, arena and stream.  The conventions are those of sbx.h: device pointers unless the
 * name ends in `_host`, nothing allocated and handed back, scratch from the handle's arena, work enqueued on the handle's
 * stream, sbx_status return codes, sbx_last_error text for every refusal.
 *
 * Every result is defined as the two entry points of sbx.h define it, bit for bit.
 */
#ifndef SBFX_H_
#define SBFX_H_

#include "sbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBFX_VERSION 100 /* 1.0.0 */

/* One pass over row_ptr (n + 1 offsets of `it`'s offset width):
 *   degrees_out[i] = row_ptr[i + 1] - row_ptr[i]      n ids of `it`'s id width (32-bit under SBX_I32_N64)
 *   dist_out[i]    = (F)degree / (F)nnz               n values of F = float (feature_bytes 4) or double (8): one IEEE
 *                                                     division per row; with nnz == 0 every value is 0 / 0
 * Both outputs are required (a caller that wants one of them calls sbx.h).  No alignment beyond that of the element types
 * is assumed.
 *   - n or nnz negative, a NULL pointer where n > 0, feature_bytes outside {4, 8}: SBX_ERR_BAD_ARG.
 * Not synchronous: returns with the kernel enqueued on the handle's stream. */
int sbfx_csr_degrees_degree_distribution(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t nnz, const void *row_ptr,
                                         int feature_bytes, void *degrees_out, void *dist_out);

/* One nonzero-parallel pass over col:
 *   *bandwidth_host = max |i - j| + 1 over the nonzeros (i, j), 0 without nonzeros
 *   *profile_host   = the sum over the rows i of i - min(i, smallest column of row i), exact in 64 bits
 * Rows may be unsorted (a CSR built with ignore_sort): the pass notices, its bandwidth is final and the profile alone is
 * computed again from the smallest column of every row, as sbx_csr_profile does.
 * The limits are those of sbx_csr_bandwidth and sbx_csr_profile: n < 2^31 - 1; nnz < 2^31 for SBX_I32; under
 * SBX_I32_N64 the offsets are narrowed to 32 bits and nnz >= 2^31 is SBX_ERR_UNSUPPORTED.
 *   - n or nnz negative, a NULL pointer (col may be NULL where nnz == 0): SBX_ERR_BAD_ARG.
 * Synchronous: both results and the sortedness flag are read back, once. */
int sbfx_csr_bandwidth_profile(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t nnz, const void *row_ptr,
                               const void *col, int64_t *bandwidth_host, int64_t *profile_host);

#ifdef __cplusplus
}
#endif
#endif /* SBFX_H_ */
