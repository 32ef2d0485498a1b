// sbx_text.hip — COO on the device -> Matrix Market / edge-list text on the device (include/sbx_text.h).
//
//   io/mtx_writer.cc:116-186       the symmetry check of MTXWriter::WriteCOO     sbx_coo_symmetry_check
//   io/mtx_writer.cc:213-259       the array format of a COO                     sbx_text_format_dense
//   io/mtx_writer.cc:261-352       the coordinate lines                          sbx_text_format_coordinate
//   io/mtx_writer.cc:399-407       WriteArray's value lines                      sbx_text_format_values
//   io/edge_list_writer.cc:26-51   swap, sort, unique of an undirected list      sbx_coo_undirected_unique
//
// The reference writes one `ofstream <<` per token.  Here a formatter is four steps:
//   1. k_text_records    floating-point values -> 16-byte decimal records (digits, count, exponent: sbx_bin2dec.h) by the
//                        128-bit fast path; the few values it does not reach are appended to a list
//   2. k_text_long       the listed values through the multi-limb path (per-thread limb arrays: scratch memory, which
//                        is why it is a kernel of its own and not a branch of the kernel every value goes through)
//   3. k_tx_lengths      the length of every line, summed per workgroup; a 64-bit scan of the sums gives every
//                        workgroup's offset in the text and the total, which is read back (the sizing call ends here)
//   4. k_tx_write        the lengths again, scanned inside the workgroup; every thread writes its line into LDS at its
//                        offset, and the workgroup's span goes to global memory in aligned 16-byte words — the LDS image
//                        is shifted by the span's misalignment so that LDS words and global words coincide — with at
//                        most 15 single bytes at either end.  Nothing at or beyond the text's length is touched.
// Steps 3 and 4 are the emit back end of sbx_text_emit.h (tx_emit) over a TextJob, whose items are the lines.
// The conversion runs once (the records are kept between 3 and 4); the digits of the indices are produced twice.
#include "sbx_bin2dec.h"
#include "sbx_device.h"
#include "sbx_internal.h"
#include "sbx_text.h"
#include "sbx_text_emit.h"  // integer and value printing, decimal records, the emit back end: shared with sbx_metis.hip, sbx_patoh.hip

namespace {

struct TextJob {
  const void *row, *col, *val;
  const int32_t *slot;    // dense: the entry stored in cell i, -1 where none is
  const sbx_decrec *rec;  // TI_RECORD: one per line
  int64_t items, base;
  int idx64, coords, vkind, vb, precision;
  unsigned flags;
  __device__ __forceinline__ int64_t id(const void *a, int64_t i) const {
    return idx64 ? ((const int64_t *)a)[i] : (int64_t)((const int32_t *)a)[i];
  }
  __device__ __forceinline__ bool keep(int64_t r, int64_t c) const {
    if ((flags & SBX_TEXT_LOWER) && c > r) return false;
    if ((flags & SBX_TEXT_NO_DIAGONAL) && c == r) return false;
    return true;
  }
  __device__ __forceinline__ void locate(int64_t k, int64_t *line, int64_t *sub) const {
    *line = k;
    *sub = 0;
  }
  // the value of line i: a record as it is (an empty dense cell's is +0 already); "0" for the zero kind and for a dense
  // cell that holds nothing
  __device__ __forceinline__ int value_length(int64_t i) const {
    if (vkind == TI_RECORD) return tx_item_value_length(TI_RECORD, vb, precision, val, rec, i, i);
    int64_t src = i;
    if (vkind == TI_ZERO || (slot && (src = slot[i]) < 0)) return 1;
    return tx_item_value_length(vkind, vb, precision, val, rec, src, i);
  }
  __device__ __forceinline__ int value_emit(int64_t i, char *dst) const {
    if (vkind == TI_RECORD) return tx_item_value_emit(TI_RECORD, vb, precision, val, rec, i, i, dst);
    int64_t src = i;
    if (vkind == TI_ZERO || (slot && (src = slot[i]) < 0)) {
      dst[0] = '0';
      return 1;
    }
    return tx_item_value_emit(vkind, vb, precision, val, rec, src, i, dst);
  }
  // line i with its '\n'; 0 for an entry that is not kept.  One decision on dst: the length pass carries no stores and
  // the write pass no tests
  __device__ __forceinline__ unsigned item(int64_t i, int64_t, char *dst) const {
    return dst ? line<true>(i, dst) : line<false>(i, nullptr);
  }
  template <bool EMIT>
  __device__ __forceinline__ unsigned line(int64_t i, char *dst) const {
    int o = 0;
    if (coords) {
      const int64_t r = id(row, i), c = id(col, i);
      if (!keep(r, c)) return 0;
      o = EMIT ? tx_emit_signed(r + base, dst) : tx_len_signed(r + base);
      if (EMIT) dst[o] = ' ';
      o++;
      o += EMIT ? tx_emit_signed(c + base, dst + o) : tx_len_signed(c + base);
      if (vkind != TI_NONE) {
        if (EMIT) dst[o] = ' ';
        o++;
      }
    }
    if (vkind != TI_NONE) o += EMIT ? value_emit(i, dst + o) : value_length(i);
    if (EMIT) dst[o] = '\n';
    return (unsigned)(o + 1);
  }
};
static_assert(20 + 1 + 20 + 1 + SBX_DEC_MAX_CHARS + 1 <= TX_LINE_MAX, "a line fits its LDS slot");

// ---- symmetry check
struct SymCounts {
  unsigned long long unmatched, diagonal, diagonal_nonzero, out_of_range;
};

template <typename I>
__global__ __launch_bounds__(TX_THREADS) void k_ids_in_range(const I *__restrict__ row, const I *__restrict__ col, int64_t nnz,
                                                             int64_t n, int64_t m, SymCounts *__restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * TX_THREADS + threadIdx.x;
  unsigned bad = 0;
  if (i < nnz) {
    const int64_t r = (int64_t)row[i], c = (int64_t)col[i];
    bad = (r < 0 || r >= n || c < 0 || c >= m) ? 1u : 0u;
  }
  bad = sbx_wave_sum(bad);
  if (sbx_lane() == 0 && bad) atomicAdd(&counts->out_of_range, (unsigned long long)bad);
}

// VK: 0 no values, 1 32-bit integers, 2 64-bit integers, 3 float, 4 double
template <int VK>
__device__ __forceinline__ bool sym_value_match(const void *sval, int64_t k, const void *val, int64_t i, int skew) {
  if (VK == 0) return !skew;  // (:127-130: a pattern cannot be skew-symmetric)
  if (VK == 1) {
    const uint32_t w = ((const uint32_t *)sval)[k], v = ((const uint32_t *)val)[i];
    return skew ? w == 0u - v : w == v;
  }
  if (VK == 2) {
    const uint64_t w = ((const uint64_t *)sval)[k], v = ((const uint64_t *)val)[i];
    return skew ? w == 0ull - v : w == v;
  }
  if (VK == 3) {
    const float w = ((const float *)sval)[k], v = ((const float *)val)[i];
    return skew ? w == -v : w == v;
  }
  const double w = ((const double *)sval)[k], v = ((const double *)val)[i];
  return skew ? w == -v : w == v;
}
template <int VK>
__device__ __forceinline__ bool sym_nonzero(const void *val, int64_t i) {
  if (VK == 0) return false;
  if (VK == 1) return ((const uint32_t *)val)[i] != 0u;
  if (VK == 2) return ((const uint64_t *)val)[i] != 0ull;
  if (VK == 3) return ((const float *)val)[i] != 0.0f;
  return ((const double *)val)[i] != 0.0;
}

// (row, col, val): the entries as given; (srow, scol, sval): the same entries sorted by (row, col)
template <typename I, int VK>
__global__ __launch_bounds__(TX_THREADS) void k_symmetry(const I *__restrict__ row, const I *__restrict__ col,
                                                         const void *__restrict__ val, const I *__restrict__ srow,
                                                         const I *__restrict__ scol, const void *__restrict__ sval, int64_t nnz,
                                                         int skew, SymCounts *__restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * TX_THREADS + threadIdx.x;
  unsigned unmatched = 0, diag = 0, diag_nz = 0;
  if (i < nnz) {
    const I r = row[i], c = col[i];
    if (r == c) {
      diag = 1;
      diag_nz = sym_nonzero<VK>(val, i) ? 1u : 0u;
    } else {
      int64_t lo = 0, hi = nnz;  // first position whose coordinate is >= (c, r)
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const I mr = srow[mid];
        if (mr < c || (mr == c && scol[mid] < r)) lo = mid + 1;
        else hi = mid;
      }
      bool found = false;
      for (int64_t k = lo; k < nnz && !found && srow[k] == c && scol[k] == r; k++) found = sym_value_match<VK>(sval, k, val, i, skew);
      unmatched = found ? 0u : 1u;
    }
  }
  unmatched = sbx_wave_sum(unmatched);
  diag = sbx_wave_sum(diag);
  diag_nz = sbx_wave_sum(diag_nz);
  if (sbx_lane() == 0) {
    if (unmatched) atomicAdd(&counts->unmatched, (unsigned long long)unmatched);
    if (diag) atomicAdd(&counts->diagonal, (unsigned long long)diag);
    if (diag_nz) atomicAdd(&counts->diagonal_nonzero, (unsigned long long)diag_nz);
  }
}

// ---- undirected edges
struct UndStats {
  unsigned long long max_id;
  unsigned negative;
};

template <typename I>
__global__ __launch_bounds__(TX_THREADS) void k_undirected_swap(I *__restrict__ row, I *__restrict__ col, int64_t nnz,
                                                                UndStats *__restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * TX_THREADS + threadIdx.x;
  unsigned long long mx = 0;
  unsigned neg = 0;
  if (i < nnz) {
    I u = row[i], v = col[i];
    if (u > v) {  // edge_list_writer.cc:27-30
      row[i] = v;
      col[i] = u;
      const I t = u;
      u = v;
      v = t;
    }
    if (u < 0) neg = 1;
    else mx = (unsigned long long)v;
  }
  mx = sbx_wave_max(mx);
  neg = sbx_wave_max(neg);
  if (sbx_lane() == 0) {
    if (mx) atomicMax(&stats->max_id, mx);
    if (neg) atomicOr(&stats->negative, 1u);
  }
}

template <typename I>
__global__ __launch_bounds__(TX_THREADS) void k_run_first(const I *__restrict__ row, const I *__restrict__ col, int64_t count,
                                                          unsigned *__restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * TX_THREADS + threadIdx.x;
  if (i < count) first[i] = (i == 0 || row[i] != row[i - 1] || col[i] != col[i - 1]) ? 1u : 0u;
}

template <typename I, int VB>
__global__ __launch_bounds__(TX_THREADS) void k_run_compact(const I *__restrict__ row, const I *__restrict__ col,
                                                            const char *__restrict__ val, const unsigned *__restrict__ first,
                                                            const unsigned *__restrict__ before, int64_t count,
                                                            I *__restrict__ row_out, I *__restrict__ col_out,
                                                            char *__restrict__ val_out) {
  const int64_t i = (int64_t)blockIdx.x * TX_THREADS + threadIdx.x;
  if (i >= count || !first[i]) return;
  const int64_t o = before[i];
  row_out[o] = row[i];
  col_out[o] = col[i];
  if (VB == 4) ((uint32_t *)val_out)[o] = ((const uint32_t *)val)[i];
  if (VB == 8) ((uint64_t *)val_out)[o] = ((const uint64_t *)val)[i];
}

// ---- dense: which entry sits in which cell
enum : unsigned { DN_RANGE = 1u, DN_DUPLICATE = 2u };

template <typename I>
__global__ __launch_bounds__(TX_THREADS) void k_dense_slots(const I *__restrict__ row, const I *__restrict__ col, int64_t nnz,
                                                            int64_t n, int64_t m, int32_t *__restrict__ slot,
                                                            unsigned *__restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * TX_THREADS + threadIdx.x;
  if (i >= nnz) return;
  const int64_t r = (int64_t)row[i], c = (int64_t)col[i];
  if (r < 0 || r >= n || c < 0 || c >= m) {
    atomicOr(status, DN_RANGE);
    return;
  }
  if (atomicCAS(&slot[c * n + r], -1, (int32_t)i) != -1) atomicOr(status, DN_DUPLICATE);
}

}  // namespace

// steps 1 to 4 for a job whose arrays are set; the caller has begun the arena and holds a NestGuard
static int tx_format(sbx_handle_t h, const char *who, TextJob job, void *text_out, int64_t capacity, int64_t *bytes_host) {
  *bytes_host = 0;
  if (job.items == 0) return SBX_OK;
  if (job.items >= ((int64_t)1 << 32))
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: 2^32 lines and more in one call (pass the entries in sub-ranges)", who);
  if (job.vkind == TI_RECORD) {
    sbx_decrec *rec = nullptr;
    SBX_TRY(tx_records(h, job.val, job.slot, job.items, job.vb, job.precision, &rec));
    job.rec = rec;
  }
  const int64_t line_in = (job.coords ? 2 * (job.idx64 ? 8 : 4) : 0) + (job.slot ? 4 : 0) +
                          (job.vkind == TI_RECORD ? (int64_t)sizeof(sbx_decrec) : job.vkind == TI_NONE ? 0 : job.vb);
  SBX_PROF_BYTES(h, SBX_K_TEXT_WRITE, job.items * line_in);  // the lengths pass reads the lines too
  return tx_emit(h, who, job, job.items * line_in, text_out, capacity, bytes_host);
}

extern "C" int sbx_text_format_values(sbx_handle_t h, sbx_value_type vt, int64_t count, const void *vals, int precision,
                                      void *text_out, int64_t capacity, int64_t *bytes_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, bytes_host && count >= 0 && capacity >= 0 && (count == 0 || vals), "bad argument");
  SBX_REQUIRE(h, precision >= 1 && precision <= 17, "precision: 1..17");
  const int vkind = tx_item_kind(vt);
  SBX_REQUIRE(h, vkind > TI_NONE, "a value type is needed");
  SBX_TRY(sbx_arena_begin(h));
  NestGuard guard(h);
  TextJob job = {};
  job.val = vals;
  job.items = count;
  job.vkind = vkind;
  job.vb = sbx_value_bytes(vt);
  job.precision = precision;
  return tx_format(h, __func__, job, text_out, capacity, bytes_host);
}

extern "C" int sbx_text_format_coordinate(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t nnz, const void *row,
                                          const void *col, const void *val, int64_t index_base, int precision,
                                          unsigned flags, void *text_out, int64_t capacity, int64_t *bytes_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  if (it == SBX_I32_N64) it = SBX_I32;  // (no offset array)
  SBX_REQUIRE(h, bytes_host && nnz >= 0 && capacity >= 0 && (nnz == 0 || (row && col)), "bad argument");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64, "unknown index type");
  SBX_REQUIRE(h, precision >= 1 && precision <= 17, "precision: 1..17");
  SBX_REQUIRE(h, (flags & ~(SBX_TEXT_LOWER | SBX_TEXT_NO_DIAGONAL | SBX_TEXT_PATTERN)) == 0, "unknown flag");
  int vkind = tx_item_kind(vt);
  SBX_REQUIRE(h, vkind >= 0, "unknown value type");
  if (!val || (flags & SBX_TEXT_PATTERN)) vkind = TI_NONE;
  SBX_TRY(sbx_arena_begin(h));
  NestGuard guard(h);
  TextJob job = {};
  job.row = row;
  job.col = col;
  job.val = val;
  job.items = nnz;
  job.base = index_base;
  job.idx64 = it == SBX_I64 ? 1 : 0;
  job.coords = 1;
  job.vkind = vkind;
  job.vb = vkind == TI_NONE ? 0 : sbx_value_bytes(vt);
  job.precision = precision;
  job.flags = flags;
  return tx_format(h, __func__, job, text_out, capacity, bytes_host);
}

template <typename I>
static int dense_typed(sbx_handle_t h, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, const void *row, const void *col,
                       const void *val, int precision, void *text_out, int64_t capacity, int64_t *bytes_host) {
  const int64_t cells = n * m;
  *bytes_host = 0;
  if (cells == 0) {
    SBX_REQUIRE(h, nnz == 0, "an id outside the matrix");
    return SBX_OK;
  }
  int32_t *slot = nullptr;
  unsigned *status = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)cells, &slot));
  SBX_TRY(sbx_salloc(h, 1, &status));
  SBX_TRY(sbx_fill_i32(h, slot, -1, cells));
  SBX_HIP(h, hipMemsetAsync(status, 0, sizeof(unsigned), h->stream));
  if (nnz > 0) {
    SBX_KLAUNCH(h, SBX_K_TEXT_CHECK, k_dense_slots<I>, dim3(tx_grid(nnz)), dim3(TX_THREADS), (const I *)row, (const I *)col,
                nnz, n, m, slot, status);
    SBX_LAUNCH_CHECK(h);
    SBX_PROF_BYTES(h, SBX_K_TEXT_CHECK, nnz * (int64_t)(2 * sizeof(I) + 4));
  }
  unsigned st = 0;
  SBX_TRY(sbx_readback(h, &st, status, sizeof(unsigned)));
  if (st & DN_RANGE) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbx_text_format_dense: an id outside [0, n) x [0, m)");
  if (st & DN_DUPLICATE) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbx_text_format_dense: a coordinate is stored twice");
  TextJob job = {};
  job.val = val;
  job.slot = slot;
  job.items = cells;
  job.vkind = (val && vt != SBX_V_NONE) ? tx_item_kind(vt) : TI_ZERO;
  job.vb = job.vkind == TI_ZERO ? 0 : sbx_value_bytes(vt);
  job.precision = precision;
  return tx_format(h, "sbx_text_format_dense", job, text_out, capacity, bytes_host);
}

extern "C" int sbx_text_format_dense(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz,
                                     const void *row, const void *col, const void *val, int precision, void *text_out,
                                     int64_t capacity, int64_t *bytes_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  if (it == SBX_I32_N64) it = SBX_I32;  // (no offset array)
  SBX_REQUIRE(h, bytes_host && n >= 0 && m >= 0 && nnz >= 0 && capacity >= 0 && (nnz == 0 || (row && col)), "bad argument");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64, "unknown index type");
  SBX_REQUIRE(h, precision >= 1 && precision <= 17, "precision: 1..17");
  SBX_REQUIRE(h, tx_item_kind(vt) >= 0, "unknown value type");
  if ((n > 0 && m > 0 && n > (((int64_t)1 << 31) - 1) / m) || nnz >= ((int64_t)1 << 31))
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbx_text_format_dense: n * m (and nnz) must be below 2^31");
  SBX_TRY(sbx_arena_begin(h));
  NestGuard guard(h);
  if (it == SBX_I64) return dense_typed<int64_t>(h, vt, n, m, nnz, row, col, val, precision, text_out, capacity, bytes_host);
  return dense_typed<int32_t>(h, vt, n, m, nnz, row, col, val, precision, text_out, capacity, bytes_host);
}

template <typename I>
static int symmetry_typed(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t nnz, const void *row,
                          const void *col, const void *val, int skew, int64_t *result_host) {
  const int vb = val ? sbx_value_bytes(vt) : 0;
  SymCounts *counts = nullptr;
  SBX_TRY(sbx_salloc(h, 1, &counts));
  SBX_HIP(h, hipMemsetAsync(counts, 0, sizeof(SymCounts), h->stream));
  const unsigned grid = tx_grid(nnz);
  SBX_KLAUNCH(h, SBX_K_TEXT_CHECK, k_ids_in_range<I>, dim3(grid), dim3(TX_THREADS), (const I *)row, (const I *)col, nnz, n, n,
              counts);
  SBX_LAUNCH_CHECK(h);
  SymCounts hc;
  SBX_TRY(sbx_readback(h, &hc, counts, sizeof(SymCounts)));
  if (hc.out_of_range) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbx_coo_symmetry_check: %llu entries with an id outside [0, n)", hc.out_of_range);
  // the sorted entries to search in: the caller's arrays if they are sorted, a sorted scratch copy otherwise
  int sorted = 0;
  SBX_TRY(sbx_coo_is_sorted(h, it, nnz, row, col, &sorted));
  const void *srow = row, *scol = col, *sval = val;
  if (!sorted) {
    I *r2 = nullptr, *c2 = nullptr;
    char *v2 = nullptr;
    SBX_TRY(sbx_salloc(h, (size_t)nnz, &r2));
    SBX_TRY(sbx_salloc(h, (size_t)nnz, &c2));
    SBX_HIP(h, hipMemcpyAsync(r2, row, (size_t)nnz * sizeof(I), hipMemcpyDeviceToDevice, h->stream));
    SBX_HIP(h, hipMemcpyAsync(c2, col, (size_t)nnz * sizeof(I), hipMemcpyDeviceToDevice, h->stream));
    if (vb) {
      SBX_TRY(sbx_salloc(h, (size_t)nnz * vb, &v2));
      SBX_HIP(h, hipMemcpyAsync(v2, val, (size_t)nnz * vb, hipMemcpyDeviceToDevice, h->stream));
    }
    SBX_TRY(sbx_coo_sort(h, it, vb ? vt : SBX_V_NONE, n, n, nnz, r2, c2, v2));
    srow = r2;
    scol = c2;
    sval = v2;
  }
  const int vk = vb == 0 ? 0 : (vt == SBX_V_F32 ? 3 : vt == SBX_V_F64 ? 4 : vb == 4 ? 1 : 2);
#define SYM(VK)                                                                                                          \
  SBX_KLAUNCH(h, SBX_K_TEXT_CHECK, (k_symmetry<I, VK>), dim3(grid), dim3(TX_THREADS), (const I *)row, (const I *)col, val, \
              (const I *)srow, (const I *)scol, sval, nnz, skew ? 1 : 0, counts)
  if (vk == 0) SYM(0);
  else if (vk == 1) SYM(1);
  else if (vk == 2) SYM(2);
  else if (vk == 3) SYM(3);
  else SYM(4);
#undef SYM
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_TEXT_CHECK, nnz * (int64_t)(4 * sizeof(I) + 2 * vb));
  SBX_TRY(sbx_readback(h, &hc, counts, sizeof(SymCounts)));
  result_host[0] = hc.unmatched == 0 ? 1 : 0;
  result_host[1] = (int64_t)hc.diagonal;
  result_host[2] = (int64_t)hc.diagonal_nonzero;
  return SBX_OK;
}

extern "C" int sbx_coo_symmetry_check(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t nnz,
                                      const void *row, const void *col, const void *val, int skew, int64_t *result_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  if (it == SBX_I32_N64) it = SBX_I32;  // (no offset array)
  SBX_REQUIRE(h, result_host && n >= 0 && nnz >= 0 && (nnz == 0 || (row && col)), "bad argument");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64, "unknown index type");
  SBX_REQUIRE(h, tx_item_kind(vt) >= 0, "unknown value type");
  if (vt == SBX_V_NONE) val = nullptr;
  result_host[0] = 1;
  result_host[1] = result_host[2] = 0;
  SBX_TRY(sbx_arena_begin(h));
  if (nnz == 0) return SBX_OK;
  NestGuard guard(h);
  if (it == SBX_I64) return symmetry_typed<int64_t>(h, it, vt, n, nnz, row, col, val, skew, result_host);
  return symmetry_typed<int32_t>(h, it, vt, n, nnz, row, col, val, skew, result_host);
}

template <typename I>
static int undirected_typed(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t nnz, void *row, void *col, void *val,
                            int64_t *nnz_host) {
  const int vb = val ? sbx_value_bytes(vt) : 0;
  UndStats *stats = nullptr;
  SBX_TRY(sbx_salloc(h, 1, &stats));
  SBX_HIP(h, hipMemsetAsync(stats, 0, sizeof(UndStats), h->stream));
  const unsigned grid = tx_grid(nnz);
  SBX_KLAUNCH(h, SBX_K_TEXT_CHECK, k_undirected_swap<I>, dim3(grid), dim3(TX_THREADS), (I *)row, (I *)col, nnz, stats);
  SBX_LAUNCH_CHECK(h);
  UndStats hs;
  SBX_TRY(sbx_readback(h, &hs, stats, sizeof(UndStats)));
  if (hs.negative) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbx_coo_undirected_unique: a negative id");
  const int64_t dim = (int64_t)hs.max_id + 1;
  SBX_TRY(sbx_coo_sort(h, it, vb ? vt : SBX_V_NONE, dim, dim, nnz, row, col, val));  // stable
  unsigned *first = nullptr, *before = nullptr;
  I *r2 = nullptr, *c2 = nullptr;
  char *v2 = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)nnz + 1, &first));
  SBX_TRY(sbx_salloc(h, (size_t)nnz + 1, &before));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &r2));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &c2));
  if (vb) SBX_TRY(sbx_salloc(h, (size_t)nnz * vb, &v2));
  SBX_HIP(h, hipMemsetAsync(first + nnz, 0, sizeof(unsigned), h->stream));
  SBX_KLAUNCH(h, SBX_K_TEXT_CHECK, k_run_first<I>, dim3(grid), dim3(TX_THREADS), (const I *)row, (const I *)col, nnz, first);
  SBX_TRY(sbx_exclusive_scan_u32(h, first, before, nnz + 1, nullptr));
#define COMPACT(VBX)                                                                                                       \
  SBX_KLAUNCH(h, SBX_K_TEXT_CHECK, (k_run_compact<I, VBX>), dim3(grid), dim3(TX_THREADS), (const I *)row, (const I *)col,   \
              (const char *)val, (const unsigned *)first, (const unsigned *)before, nnz, r2, c2, v2)
  if (vb == 0) COMPACT(0);
  else if (vb == 4) COMPACT(4);
  else COMPACT(8);
#undef COMPACT
  SBX_LAUNCH_CHECK(h);
  unsigned uniq = 0;
  SBX_TRY(sbx_readback(h, &uniq, before + nnz, sizeof(unsigned)));
  SBX_HIP(h, hipMemcpyAsync(row, r2, (size_t)uniq * sizeof(I), hipMemcpyDeviceToDevice, h->stream));
  SBX_HIP(h, hipMemcpyAsync(col, c2, (size_t)uniq * sizeof(I), hipMemcpyDeviceToDevice, h->stream));
  if (vb) SBX_HIP(h, hipMemcpyAsync(val, v2, (size_t)uniq * vb, hipMemcpyDeviceToDevice, h->stream));
  SBX_PROF_BYTES(h, SBX_K_TEXT_CHECK, nnz * (int64_t)(6 * sizeof(I) + 2 * vb + 8));
  *nnz_host = uniq;
  return SBX_OK;
}

extern "C" int sbx_coo_undirected_unique(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t nnz, void *row,
                                         void *col, void *val, int64_t *nnz_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  if (it == SBX_I32_N64) it = SBX_I32;  // (no offset array)
  SBX_REQUIRE(h, nnz_host && nnz >= 0 && (nnz == 0 || (row && col)), "bad argument");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64, "unknown index type");
  SBX_REQUIRE(h, tx_item_kind(vt) >= 0, "unknown value type");
  if (nnz >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbx_coo_undirected_unique: nnz must be below 2^31");
  if (vt == SBX_V_NONE) val = nullptr;
  *nnz_host = 0;
  SBX_TRY(sbx_arena_begin(h));
  if (nnz == 0) return SBX_OK;
  NestGuard guard(h);
  if (it == SBX_I64) return undirected_typed<int64_t>(h, it, vt, nnz, row, col, val, nnz_host);
  return undirected_typed<int32_t>(h, it, vt, nnz, row, col, val, nnz_host);
}
