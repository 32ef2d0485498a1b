// sbx_text_emit.h — what the text formatters share: integer and value printing, floating-point values -> decimal records
// (sbx_bin2dec.h), and the emit back end, tx_emit<Job>: the lengths of a job's items summed per workgroup, scanned and
// read back, then the items written through LDS, a workgroup's text image going out in aligned 16-byte words.  A formatter
// is a job (items, locate, item) and what it does before tx_emit.  Used by the Matrix Market / edge-list formatters
// (sbx_text.hip: TextJob), the METIS graph formatter (sbx_metis.hip: GrJob) and the PaToH formatters (sbx_patoh.hip:
// HgNetJob, HgWeightJob).
#pragma once
#include "sbx_bin2dec.h"
#include "sbx_device.h"
#include "sbx_internal.h"

namespace {  // (kernels in a header shared by several translation units: internal linkage)

constexpr int TX_THREADS = 256;
constexpr int TX_LINE_MAX = 68;  // the LDS slot of an item (every job asserts that its longest one fits): a coordinate line
                                 // is 2 x 20 index characters, 2 blanks, SBX_DEC_MAX_CHARS, '\n', rounded up
constexpr int TX_LDS = TX_THREADS * TX_LINE_MAX + 16;

__device__ __forceinline__ int tx_len_signed(int64_t v) {
  return v < 0 ? 1 + sbx_b2d::length_u64(0ull - (uint64_t)v) : sbx_b2d::length_u64((uint64_t)v);
}
__device__ __forceinline__ int tx_emit_signed(int64_t v, char *dst) {
  if (v < 0) {
    dst[0] = '-';
    return 1 + sbx_b2d::emit_u64(0ull - (uint64_t)v, dst + 1);
  }
  return sbx_b2d::emit_u64((uint64_t)v, dst);
}

// ---- a value of the formatters' items: how it is kept (vkind) and its text.  TI_RECORD: floating point, printed from the
// decimal record rec[irel] (tx_records); the integer kinds print arr[i], a value of vb bytes, in full.  TI_ZERO is the
// array format's alone (sbx_text.hip): no value is kept, every cell prints "0"
enum : int { TI_NONE = 0, TI_SIGNED, TI_UNSIGNED, TI_RECORD, TI_ZERO };
static inline int tx_item_kind(sbx_value_type vt) {  // -1: no value type
  switch (vt) {
    case SBX_V_NONE: return TI_NONE;
    case SBX_V_I32: case SBX_V_I64: return TI_SIGNED;
    case SBX_V_U32: case SBX_V_U64: return TI_UNSIGNED;
    case SBX_V_F32: case SBX_V_F64: return TI_RECORD;
  }
  return -1;
}
__device__ __forceinline__ int tx_item_value_length(int vkind, int vb, int precision, const void *arr, const sbx_decrec *rec,
                                               int64_t i, int64_t irel) {
  if (vkind == TI_RECORD) return sbx_b2d::text_length(rec[irel], precision);
  if (vkind == TI_SIGNED) return tx_len_signed(vb == 4 ? (int64_t)((const int32_t *)arr)[i] : ((const int64_t *)arr)[i]);
  return sbx_b2d::length_u64(vb == 4 ? (uint64_t)((const uint32_t *)arr)[i] : ((const uint64_t *)arr)[i]);
}
__device__ __forceinline__ int tx_item_value_emit(int vkind, int vb, int precision, const void *arr, const sbx_decrec *rec,
                                             int64_t i, int64_t irel, char *dst) {
  if (vkind == TI_RECORD) return sbx_b2d::emit(rec[irel], precision, dst);
  if (vkind == TI_SIGNED) return tx_emit_signed(vb == 4 ? (int64_t)((const int32_t *)arr)[i] : ((const int64_t *)arr)[i], dst);
  return sbx_b2d::emit_u64(vb == 4 ? (uint64_t)((const uint32_t *)arr)[i] : ((const uint64_t *)arr)[i], dst);
}

// ---- values -> decimal records
template <int BITS>
__device__ __forceinline__ uint64_t tx_bits(const void *val, const int32_t *slot, int64_t i, bool *stored) {
  int64_t src = i;
  *stored = true;
  if (slot) {
    const int32_t s = slot[i];
    if (s < 0) {
      *stored = false;
      return 0;
    }
    src = s;
  }
  return BITS == 64 ? ((const uint64_t *)val)[src] : (uint64_t)((const uint32_t *)val)[src];
}

template <int BITS>
__global__ __launch_bounds__(TX_THREADS) void k_text_records(const void *__restrict__ val, const int32_t *__restrict__ slot,
                                                             int64_t count, int precision,
                                                             const uint64_t *__restrict__ pow5, sbx_decrec *__restrict__ rec,
                                                             unsigned *__restrict__ long_list, unsigned *__restrict__ long_count) {
  const int64_t i = (int64_t)blockIdx.x * TX_THREADS + threadIdx.x;
  bool lng = false;
  if (i < count) {
    bool stored;
    const uint64_t bits = tx_bits<BITS>(val, slot, i, &stored);  // (an empty cell: +0, which prints as "0")
    const sbx_decrec r = sbx_b2d::to_record<false, BITS>(bits, precision, pow5);
    lng = (r.kind >> 1) == SBX_DEC_LONG;
    rec[i] = r;
  }
  const unsigned pos = sbx_wave_append(long_count, lng);  // (every lane calls it)
  if (lng) long_list[pos] = (unsigned)i;
}

template <int BITS>
__global__ __launch_bounds__(TX_THREADS) void k_text_long(const void *__restrict__ val, const int32_t *__restrict__ slot,
                                                          int precision, const uint64_t *__restrict__ pow5,
                                                          sbx_decrec *__restrict__ rec, const unsigned *__restrict__ long_list,
                                                          const unsigned *__restrict__ long_count) {
  const unsigned total = *long_count;
  for (unsigned k = blockIdx.x * TX_THREADS + threadIdx.x; k < total; k += gridDim.x * TX_THREADS) {
    const int64_t i = long_list[k];
    bool stored;
    const uint64_t bits = tx_bits<BITS>(val, slot, i, &stored);
    rec[i] = sbx_b2d::to_record<true, BITS>(bits, precision, pow5);
  }
}

// The workgroup's `total` bytes of text, which lie in s_text from byte `phase` = dst & 15 on (so that LDS words and global
// words coincide), go to dst in aligned 16-byte words, with at most 15 single bytes at either end.  Every thread of the
// workgroup calls it behind the barrier that ends the writes to s_text; nothing at or beyond dst + total is touched.
__device__ __forceinline__ void tx_block_store(const char *s_text, unsigned phase, unsigned total, char *dst) {
  unsigned head = (16u - phase) & 15u;
  if (head > total) head = total;
  const unsigned words = (total - head) >> 4, tail = (total - head) & 15u;
  if (threadIdx.x < head) dst[threadIdx.x] = s_text[phase + threadIdx.x];
  const uint4 *src16 = (const uint4 *)(s_text + phase + head);
  uint4 *dst16 = (uint4 *)(dst + head);
  for (unsigned w = threadIdx.x; w < words; w += TX_THREADS) dst16[w] = src16[w];
  const unsigned t0 = head + (words << 4);
  if (threadIdx.x < tail) dst[t0 + threadIdx.x] = s_text[phase + t0 + threadIdx.x];
}

static unsigned tx_grid(int64_t count) { return (unsigned)((count + TX_THREADS - 1) / TX_THREADS); }

// the offsets of a row range's ends; whether the offsets of the range descend somewhere (the formatters over CSR rows
// search their items in the offsets, which relies on their order)
template <typename T>
__global__ __launch_bounds__(TX_THREADS) void k_tx_range_ends(const T *__restrict__ rp, int64_t rb, int64_t re,
                                                              int64_t *__restrict__ ends, unsigned *__restrict__ descending) {
  const int64_t r = rb + (int64_t)blockIdx.x * TX_THREADS + threadIdx.x;
  if (r == rb) {
    ends[0] = (int64_t)rp[rb];
    ends[1] = (int64_t)rp[re];
  }
  if (r < re && rp[r + 1] < rp[r]) atomicOr(descending, 1u);
}
// (the read-back of both: *desc_host is set where the range cannot be formatted; the caller has begun the arena)
template <typename T>
static int tx_range_ends(sbx_handle_t h, const T *rp, int64_t rb, int64_t re, int64_t ends_host[2], bool *desc_host) {
  int64_t *ends = nullptr;
  unsigned *descending = nullptr;
  SBX_TRY(sbx_salloc(h, 2, &ends));
  SBX_TRY(sbx_salloc(h, 1, &descending));
  SBX_HIP(h, hipMemsetAsync(descending, 0, sizeof(unsigned), h->stream));
  SBX_KLAUNCH(h, SBX_K_TEXT_CHECK, k_tx_range_ends<T>, dim3(tx_grid(re - rb)), dim3(TX_THREADS), rp, rb, re, ends, descending);
  SBX_LAUNCH_CHECK(h);
  unsigned hdesc = 0;
  SBX_TRY(sbx_readback(h, ends_host, ends, 2 * sizeof(int64_t)));
  SBX_TRY(sbx_readback(h, &hdesc, descending, sizeof(unsigned)));
  *desc_host = hdesc != 0 || ends_host[0] < 0;
  return SBX_OK;
}

// the decimal records of `count` floating-point values of vb bytes (steps 1 and 2 of a formatter): the 128-bit fast path,
// then the listed values through the multi-limb path; the caller has begun the arena
static int tx_records(sbx_handle_t h, const void *val, const int32_t *slot, int64_t count, int vb, int precision,
                      sbx_decrec **rec_out) {
  const uint64_t *pow5 = nullptr;
  SBX_TRY(sbx_pow5_table(h, &pow5));
  sbx_decrec *rec = nullptr;
  unsigned *long_list = nullptr, *long_count = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)count, &rec));
  SBX_TRY(sbx_salloc(h, (size_t)count, &long_list));
  SBX_TRY(sbx_salloc(h, 1, &long_count));
  SBX_HIP(h, hipMemsetAsync(long_count, 0, sizeof(unsigned), h->stream));
  const unsigned grid = tx_grid(count);
  const unsigned lgrid = grid < 1024u ? grid : 1024u;
  if (vb == 8) {
    SBX_KLAUNCH(h, SBX_K_TEXT_FORMAT, k_text_records<64>, dim3(grid), dim3(TX_THREADS), val, slot, count, precision, pow5,
                rec, long_list, long_count);
    SBX_KLAUNCH(h, SBX_K_TEXT_LONG, k_text_long<64>, dim3(lgrid), dim3(TX_THREADS), val, slot, precision, pow5, rec,
                (const unsigned *)long_list, (const unsigned *)long_count);
  } else {
    SBX_KLAUNCH(h, SBX_K_TEXT_FORMAT, k_text_records<32>, dim3(grid), dim3(TX_THREADS), val, slot, count, precision, pow5,
                rec, long_list, long_count);
    SBX_KLAUNCH(h, SBX_K_TEXT_LONG, k_text_long<32>, dim3(lgrid), dim3(TX_THREADS), val, slot, precision, pow5, rec,
                (const unsigned *)long_list, (const unsigned *)long_count);
  }
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_TEXT_FORMAT, count * (int64_t)(vb + sizeof(sbx_decrec)));
  *rec_out = rec;
  return SBX_OK;
}

// ---- the emit back end (steps 3 and 4 of a formatter).  A job gives item k of its `items` a place, locate(k, &row,
// &sub), and a text, item(row, sub, dst): the length; written at dst unless dst is null.  An item of length 0 is left out.
template <typename Job>
__global__ __launch_bounds__(TX_THREADS) void k_tx_lengths(const Job j, int64_t *__restrict__ block_len) {
  __shared__ unsigned s_red[TX_THREADS / 64 + 1];
  const int64_t k = (int64_t)blockIdx.x * TX_THREADS + threadIdx.x;
  unsigned len = 0;
  if (k < j.items) {
    int64_t r, sub;
    j.locate(k, &r, &sub);
    len = j.item(r, sub, nullptr);
  }
  const unsigned tot = sbx_block_sum<unsigned, TX_THREADS>(len, s_red);
  if (threadIdx.x == 0) block_len[blockIdx.x] = (int64_t)tot;
}

template <typename Job>
__global__ __launch_bounds__(TX_THREADS) void k_tx_write(const Job j, const int64_t *__restrict__ block_off,
                                                         char *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) char s_text[TX_LDS];
  __shared__ unsigned s_scan[TX_THREADS / 64 + 1];
  const int64_t k = (int64_t)blockIdx.x * TX_THREADS + threadIdx.x;
  unsigned len = 0;
  int64_t r = 0, sub = 0;
  if (k < j.items) {
    j.locate(k, &r, &sub);
    len = j.item(r, sub, nullptr);
  }
  unsigned total;
  const unsigned off = sbx_block_exclusive_sum<unsigned, TX_THREADS>(len, s_scan, &total);
  char *dst = out + block_off[blockIdx.x];
  const unsigned phase = (unsigned)((uintptr_t)dst & 15u);  // the LDS image starts at the same offset inside a 16-byte word
  if (len) j.item(r, sub, s_text + phase + off);
  __syncthreads();
  tx_block_store(s_text, phase, total, dst);
}

// The lengths summed per workgroup, a 64-bit scan of the sums (every workgroup's offset in the text, and the total, which
// is read back: the sizing call ends here), the write.  job.items >= 1; in_bytes: what the job reads, for the profiler;
// the caller has begun the arena and holds a NestGuard.
template <typename Job>
static int tx_emit(sbx_handle_t h, const char *who, const Job &job, int64_t in_bytes, void *text_out, int64_t capacity,
                   int64_t *bytes_host) {
  const unsigned grid = tx_grid(job.items);
  int64_t *block_len = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)grid + 1, &block_len));
  SBX_HIP(h, hipMemsetAsync(block_len + grid, 0, sizeof(int64_t), h->stream));
  SBX_KLAUNCH(h, SBX_K_TEXT_WRITE, k_tx_lengths<Job>, dim3(grid), dim3(TX_THREADS), job, block_len);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_exclusive_scan_i64(h, block_len, block_len, (int64_t)grid + 1, nullptr));
  int64_t total = 0;
  SBX_TRY(sbx_readback(h, &total, block_len + grid, sizeof(int64_t)));
  *bytes_host = total;
  if (!text_out) return SBX_OK;  // the sizing call
  if (capacity < total)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: the text has %lld bytes, text_out holds %lld", who, (long long)total,
             (long long)capacity);
  if (total == 0) return SBX_OK;
  SBX_KLAUNCH(h, SBX_K_TEXT_WRITE, k_tx_write<Job>, dim3(grid), dim3(TX_THREADS), job, (const int64_t *)block_len,
              (char *)text_out);
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_TEXT_WRITE, in_bytes + total);
  return SBX_OK;
}

}  // namespace
