// sbx_symmetrize.hip — B = A ∪ Aᵀ of a square CSR with column-sorted rows (include/sbsym.h).  Every id,
// offset and position inside is 32-bit (n < 2^31 - 1, nnz < 2^31, nnz_out < 2^31).
//
//   T        the entries transposed by the library's stable radix sort: keys col << 32 | row sorted by their column bits
//            (the rows are in order already), the source position as payload.  The pass that makes the keys checks the
//            columns (range, order inside a row), counts the stored diagonal and keeps every entry's row.
//   equal    A is pattern-symmetric exactly when T's keys, read in order, are A's own (row, col) sequence: one streaming
//            comparison and one flag.  The keep pass reads the flag on the device and leaves at once when it is clear.
//   keep     nonzero-parallel over T: the entry (i <- j) is kept when it is the first of its run of equal keys and j is
//            not found by a binary search in A's row i.  The kept count is what the one read-back carries.
//   emit     after the read-back (counts known, capacity checked): offsets of T's segments, an exclusive scan of the keep
//            flags, row lengths, a scan into row_ptr_out, and two nonzero-parallel passes with positions in closed form:
//              A's entry at rank p of row i with column c    row_ptr_out[i] + p + kept_before(lower_bound_T(i, c))
//              a kept entry of T's segment i with column x   row_ptr_out[i] + kept_rank + lower_bound_A(i, x)
//            SBSYM_NO_DIAGONAL: one n-parallel pass counts each row's diagonal run (two searches per row); entries
//            right of it move left by that count.
// No kernel gives a lane or a wave a whole row: the work of a hub row is that of as many entries of short rows.
// Counters are reduced per workgroup and sit on 128-byte lines of their own.
#include <cstddef>

#include "sbsym.h"
#include "sbx_device.h"
#include "sbx_internal.h"

#ifndef SBSYM_FASTPATH
#define SBSYM_FASTPATH 1  // 0: the keep pass searches whatever the comparison found (the A/B of tools/symmetrize_probe.py)
#endif

namespace {

constexpr int SY = 256;  // threads per workgroup; every kernel is a grid-stride loop of one item (four in k_sym_equal)

struct alignas(128) SymLine {
  unsigned v;
};
struct SymDev {  // device state of a call, zeroed once; one line per word that workgroups add to or raise
  SymLine bad_col;    // a column outside [0, n)
  SymLine bad_order;  // a row whose columns decrease
  SymLine bad_ptr;    // row_ptr[0] != 0 or row_ptr[n] != nnz
  SymLine differ;     // T's key sequence is not A's (row, col) sequence
  SymLine added;      // kept entries of T
  SymLine ndiag;      // stored (i, i)
};

#define SY_GRID_LOOP(i, count) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)(count); i += (int64_t)gridDim.x * blockDim.x)

// first position in [lo, hi) of a non-decreasing arr with arr[pos] >= x
template <typename T, typename X>
__device__ __forceinline__ uint32_t sy_lower_bound(const T *__restrict__ arr, uint32_t lo, uint32_t hi, X x) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((X)arr[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// transposed keys col << 32 | row with the source position as payload, every entry's row, the checks and the diagonal
// count.  An entry that fails a check gets the harmless key 0: no later search sees its id.
template <typename I, typename N>
__global__ __launch_bounds__(SY) void k_sym_tkeys(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                  int64_t nnz, uint64_t *__restrict__ tkey, uint32_t *__restrict__ tpos,
                                                  uint32_t *__restrict__ rowid, SymDev *__restrict__ dv) {
  __shared__ unsigned lds[SY / 64 + 1];
  __shared__ int64_t span[2];  // the rows of a step's first and last entry: two full searches per workgroup and step
  unsigned nd = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && ((int64_t)rp[0] != 0 || (int64_t)rp[n] != nnz)) dv->bad_ptr.v = 1;
  for (int64_t base = (int64_t)blockIdx.x * SY; base < nnz; base += (int64_t)gridDim.x * SY) {
    const int64_t last = (base + SY < nnz ? base + SY : nnz) - 1;
    if (threadIdx.x < 2) span[threadIdx.x] = sbx_row_of(rp, n, threadIdx.x ? last : base);
    __syncthreads();
    const int64_t r0 = span[0], r1 = span[1];
    __syncthreads();
    const int64_t p = base + threadIdx.x;
    if (p > last) continue;
    const int64_t c = (int64_t)col[p];
    const int64_t r = sbx_row_of(rp, p, r0, r1);
    uint64_t key = 0;
    if (c < 0 || c >= n) {
      dv->bad_col.v = 1;
    } else {
      if (p > (int64_t)rp[r] && (int64_t)col[p - 1] > c) dv->bad_order.v = 1;
      key = (uint64_t)c << 32 | (uint64_t)r;
      nd += c == r;
    }
    tkey[p] = key;
    tpos[p] = (uint32_t)p;
    rowid[p] = (uint32_t)r;
  }
  const unsigned tot = sbx_block_sum<unsigned, SY>(nd, lds);
  if (threadIdx.x == 0 && tot) atomicAdd(&dv->ndiag.v, tot);
}

// the streaming comparison: sorted T against A read in order, four entries per thread in 16-byte loads (the scratch
// arrays are aligned; vec_ok says that col is)
template <typename I>
__global__ __launch_bounds__(SY) void k_sym_equal(const uint64_t *__restrict__ tkey, const uint32_t *__restrict__ rowid,
                                                  const I *__restrict__ col, int64_t nnz, bool vec_ok,
                                                  SymDev *__restrict__ dv) {
  bool differ = false;
  const int64_t quads = nnz >> 2;
  SY_GRID_LOOP(g, quads) {
    const int64_t q = g << 2;
    const ulonglong2 k0 = *(const ulonglong2 *)(tkey + q), k1 = *(const ulonglong2 *)(tkey + q + 2);
    const uint4 r = *(const uint4 *)(rowid + q);
    uint64_t c[4];
    if (vec_ok) {
      if (sizeof(I) == 4) {
        const uint4 a = *(const uint4 *)(col + q);
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w;
      } else {
        const ulonglong2 a = *(const ulonglong2 *)(col + q), b = *(const ulonglong2 *)(col + q + 2);
        c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) c[k] = (uint64_t)col[q + k];
    }
    differ |= k0.x != ((uint64_t)r.x << 32 | c[0]) || k0.y != ((uint64_t)r.y << 32 | c[1]) ||
              k1.x != ((uint64_t)r.z << 32 | c[2]) || k1.y != ((uint64_t)r.w << 32 | c[3]);
  }
  if (blockIdx.x == 0) {
    const int64_t q = (quads << 2) + threadIdx.x;
    if (q < nnz) differ |= tkey[q] != ((uint64_t)rowid[q] << 32 | (uint64_t)col[q]);
  }
  if (differ) dv->differ.v = 1;
}

// keep[q] = 1 when T's entry (i <- j) is the first of its run and A's row i stores no column j.  (A diagonal entry is its
// own mirror: found.)  With `fast` and a clear `differ` nothing is written and nothing searched.
template <typename I, typename N>
__global__ __launch_bounds__(SY) void k_sym_keep(const uint64_t *__restrict__ tkey, int64_t nnz, const N *__restrict__ rp,
                                                 const I *__restrict__ col, uint32_t *__restrict__ keep, bool fast,
                                                 SymDev *__restrict__ dv) {
  __shared__ unsigned lds[SY / 64 + 1];
  if (fast && dv->differ.v == 0) return;  // (the same word for every thread of the grid)
  unsigned cnt = 0;
  SY_GRID_LOOP(q, nnz) {
    const uint64_t k = tkey[q];
    unsigned kept = 0;
    if (q == 0 || tkey[q - 1] != k) {
      const uint32_t i = (uint32_t)(k >> 32), j = (uint32_t)k;
      const uint32_t end = (uint32_t)rp[i + 1];
      const uint32_t lo = sy_lower_bound(col, (uint32_t)rp[i], end, (int64_t)j);
      kept = !(lo < end && (int64_t)col[lo] == (int64_t)j);
    }
    keep[q] = kept;
    cnt += kept;
  }
  const unsigned tot = sbx_block_sum<unsigned, SY>(cnt, lds);
  if (threadIdx.x == 0 && tot) atomicAdd(&dv->added.v, tot);
}

// off[r] = the first position of the sorted keys with key >= r << 32, r in [0, n]
__global__ __launch_bounds__(SY) void k_sym_offsets(const uint64_t *__restrict__ tkey, int64_t nnz, int64_t n,
                                                    uint32_t *__restrict__ off) {
  SY_GRID_LOOP(r, n + 1) off[r] = sy_lower_bound(tkey, 0u, (uint32_t)nnz, (uint64_t)r << 32);
}

// dcnt[i] = the stored (i, i) of row i: the run of column i in the sorted row, two searches
template <typename I, typename N>
__global__ __launch_bounds__(SY) void k_sym_diag(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                 uint32_t *__restrict__ dcnt) {
  SY_GRID_LOOP(i, n) {
    const uint32_t b = (uint32_t)rp[i], e = (uint32_t)rp[i + 1];
    const uint32_t lo = sy_lower_bound(col, b, e, (int64_t)i);
    dcnt[i] = sy_lower_bound(col, lo, e, (int64_t)i + 1) - lo;
  }
}

template <typename N>
__global__ __launch_bounds__(SY) void k_sym_rowlen(const N *__restrict__ rp, int64_t n, const uint32_t *__restrict__ tptr,
                                                   const uint32_t *__restrict__ kscan, const uint32_t *__restrict__ dcnt,
                                                   uint32_t *__restrict__ len) {
  SY_GRID_LOOP(i, n) {
    len[i] = (uint32_t)((int64_t)rp[i + 1] - (int64_t)rp[i]) + kscan[tptr[i + 1]] - kscan[tptr[i]] - (dcnt ? dcnt[i] : 0u);
  }
}

template <typename N>
__global__ __launch_bounds__(SY) void k_sym_offsets_out(const uint32_t *__restrict__ srp, int64_t n, N *__restrict__ out) {
  SY_GRID_LOOP(i, n + 1) out[i] = (N)srp[i];
}

template <typename V>
__device__ __forceinline__ void sy_copy_value(const void *__restrict__ val, uint32_t from, void *__restrict__ val_out,
                                              uint32_t to) {
  ((V *)val_out)[to] = ((const V *)val)[from];
}
struct SyNoValue {};
template <>
__device__ __forceinline__ void sy_copy_value<SyNoValue>(const void *__restrict__, uint32_t, void *__restrict__, uint32_t) {}

// A's entries: rank in the row plus the kept entries of T's segment i with a smaller column
template <typename I, typename N, typename V>
__global__ __launch_bounds__(SY) void k_sym_emit_stored(const N *__restrict__ rp, const I *__restrict__ col,
                                                        const void *__restrict__ val, int64_t nnz,
                                                        const uint32_t *__restrict__ rowid, const uint64_t *__restrict__ tkey,
                                                        const uint32_t *__restrict__ tptr, const uint32_t *__restrict__ kscan,
                                                        const uint32_t *__restrict__ dcnt, const uint32_t *__restrict__ srp,
                                                        uint32_t nnz_out, I *__restrict__ col_out, void *__restrict__ val_out) {
  SY_GRID_LOOP(p, nnz) {
    const uint32_t i = rowid[p];
    const I c = col[p];
    uint32_t shift = 0;
    if (dcnt) {
      if ((int64_t)c == (int64_t)i) continue;
      if ((int64_t)c > (int64_t)i) shift = dcnt[i];
    }
    const uint32_t t0 = tptr[i], t1 = tptr[i + 1];
    uint32_t before = 0;
    if (kscan[t1] != kscan[t0])  // (a row that gains nothing: no search)
      before = kscan[sy_lower_bound(tkey, t0, t1, (uint64_t)i << 32 | (uint64_t)c)] - kscan[t0];
    const uint32_t pos = srp[i] + (uint32_t)(p - (int64_t)rp[i]) + before - shift;
    if (pos < nnz_out) {
      col_out[pos] = c;
      sy_copy_value<V>(val, (uint32_t)p, val_out, pos);
    }
  }
}

// the kept entries of T: rank among the kept of the segment plus A's entries of row i with a smaller column
template <typename I, typename N, typename V>
__global__ __launch_bounds__(SY) void k_sym_emit_kept(const N *__restrict__ rp, const I *__restrict__ col,
                                                      const void *__restrict__ val, int64_t nnz,
                                                      const uint64_t *__restrict__ tkey, const uint32_t *__restrict__ tpos,
                                                      const uint32_t *__restrict__ tptr, const uint32_t *__restrict__ kscan,
                                                      const uint32_t *__restrict__ dcnt, const uint32_t *__restrict__ srp,
                                                      uint32_t nnz_out, I *__restrict__ col_out, void *__restrict__ val_out) {
  SY_GRID_LOOP(q, nnz) {
    const uint32_t rank = kscan[q];
    if (kscan[q + 1] == rank) continue;  // not kept
    const uint64_t k = tkey[q];
    const uint32_t i = (uint32_t)(k >> 32), x = (uint32_t)k;
    const uint32_t b = (uint32_t)rp[i];
    const uint32_t smaller = sy_lower_bound(col, b, (uint32_t)rp[i + 1], (int64_t)x) - b;
    const uint32_t shift = (dcnt && x > i) ? dcnt[i] : 0u;
    const uint32_t pos = srp[i] + (rank - kscan[tptr[i]]) + smaller - shift;
    if (pos < nnz_out) {
      col_out[pos] = (I)x;
      sy_copy_value<V>(val, tpos[q], val_out, pos);
    }
  }
}

struct SymCall {
  sbx_handle_t h;
  int64_t n, nnz;
  SymDev *dv;
  uint64_t *tkey;
  uint32_t *tpos, *rowid, *keep;  // keep: nnz + 1 words, the flags and then their exclusive scan
  unsigned added, ndiag;          // what the read-back brought
};

static unsigned sy_grid(sbx_handle_t h, int64_t items) { return sbx_grid_for(items, SY, (int64_t)h->num_cus * 32); }

// everything up to and including the call's one read-back; nnz > 0
template <typename I, typename N>
static int sy_count(SymCall &c, const char *who, const N *rp, const I *col) {
  sbx_handle_t h = c.h;
  const int64_t n = c.n, nnz = c.nnz;
  uint64_t *ttmp = nullptr;
  uint32_t *ptmp = nullptr;
  SBX_TRY(sbx_salloc(h, 1, &c.dv));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &c.tkey));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &ttmp));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &c.tpos));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &ptmp));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &c.rowid));
  SBX_TRY(sbx_salloc(h, (size_t)nnz + 1, &c.keep));
  SBX_HIP(h, hipMemsetAsync(c.dv, 0, sizeof(SymDev), h->stream));
  const unsigned gz = sy_grid(h, nnz);
  SBX_KLAUNCH(h, SBX_K_CSC, (k_sym_tkeys<I, N>), dim3(gz), dim3(SY), rp, col, n, nnz, c.tkey, c.tpos, c.rowid, c.dv);
  SBX_LAUNCH_CHECK(h);
  const int bits = sbx_bits_for((uint64_t)(n - 1));
  // (the keys are made in (row, col) order and the sort is stable: sorting by the column bits alone leaves them in
  // (col, row) order with equal keys in stored order — half the passes of a sort by the whole key)
  SBX_TRY(sbx_sort_pairs(h, &c.tkey, &ttmp, &c.tpos, &ptmp, nnz, 32, 32 + bits));
#if SBSYM_FASTPATH
  SBX_KLAUNCH(h, SBX_K_CSC, (k_sym_equal<I>), dim3(sy_grid(h, (nnz + 3) / 4)), dim3(SY), (const uint64_t *)c.tkey,
              (const uint32_t *)c.rowid, col, nnz, ((uintptr_t)col & 15) == 0, c.dv);
#endif
  SBX_KLAUNCH(h, SBX_K_CSC, (k_sym_keep<I, N>), dim3(gz), dim3(SY), (const uint64_t *)c.tkey, nnz, rp, col, c.keep,
              (bool)SBSYM_FASTPATH, c.dv);
  SBX_LAUNCH_CHECK(h);
  SymDev rb;
  SBX_TRY(sbx_readback(h, &rb, c.dv, sizeof(rb)));
  if (rb.bad_ptr.v) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: row_ptr[0] is not 0 or row_ptr[n] is not nnz", who);
  if (rb.bad_col.v) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: a column lies outside [0, n)", who);
  if (rb.bad_order.v) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: the columns of a row decrease (rows must be column-sorted)", who);
  c.added = rb.added.v;  // (left 0 by the keep pass where the comparison found nothing)
  c.ndiag = rb.ndiag.v;
  return SBX_OK;
}

template <typename I, typename N, typename V>
static int sy_emit(SymCall &c, const N *rp, const I *col, const void *val, const uint32_t *tptr, const uint32_t *dcnt,
                   const uint32_t *srp, int64_t nnz_out, void *col_out, void *val_out) {
  sbx_handle_t h = c.h;
  const unsigned gz = sy_grid(h, c.nnz);
  SBX_KLAUNCH(h, SBX_K_CSC, (k_sym_emit_stored<I, N, V>), dim3(gz), dim3(SY), rp, col, val, c.nnz,
              (const uint32_t *)c.rowid, (const uint64_t *)c.tkey, tptr, (const uint32_t *)c.keep, dcnt, srp,
              (uint32_t)nnz_out, (I *)col_out, val_out);
  if (c.added)
    SBX_KLAUNCH(h, SBX_K_CSC, (k_sym_emit_kept<I, N, V>), dim3(gz), dim3(SY), rp, col, val, c.nnz, (const uint64_t *)c.tkey,
                (const uint32_t *)c.tpos, tptr, (const uint32_t *)c.keep, dcnt, srp, (uint32_t)nnz_out, (I *)col_out,
                val_out);
  SBX_LAUNCH_CHECK(h);
  return SBX_OK;
}

template <typename I, typename N>
static int sy_missing(sbx_handle_t h, int64_t n, int64_t nnz, const void *row_ptr, const void *col, int64_t *missing_host) {
  SBX_TRY(sbx_arena_begin(h));
  SymCall c{};
  c.h = h;
  c.n = n;
  c.nnz = nnz;
  SBX_TRY((sy_count<I, N>(c, "sbsym_csr_missing_mirrors", (const N *)row_ptr, (const I *)col)));
  *missing_host = c.added;
  return SBX_OK;
}

template <typename I, typename N>
static int sy_symmetrize(sbx_handle_t h, int vb, int64_t n, int64_t nnz, const void *row_ptr, const void *col_v,
                         const void *val, unsigned flags, int64_t out_capacity, void *row_ptr_out, void *col_out,
                         void *val_out, int64_t *nnz_out_host, int64_t *added_host) {
  const char *who = "sbsym_csr_symmetrize";
  SBX_TRY(sbx_arena_begin(h));
  const N *rp = (const N *)row_ptr;
  const I *col = (const I *)col_v;
  SymCall c{};
  c.h = h;
  c.n = n;
  c.nnz = nnz;
  SBX_TRY((sy_count<I, N>(c, who, rp, col)));
  const int64_t drop = (flags & SBSYM_NO_DIAGONAL) ? (int64_t)c.ndiag : 0;
  const int64_t nnz_out = nnz + (int64_t)c.added - drop;
  if (nnz_out_host) *nnz_out_host = nnz_out;
  if (added_host) *added_host = c.added;
  if (nnz_out >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: nnz_out = %lld >= 2^31", who, (long long)nnz_out);
  if ((flags & SBSYM_SKIP_IF_SYMMETRIC) && c.added == 0 && drop == 0) return SBX_OK;
  if (col_out && out_capacity < nnz_out)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: out_capacity %lld, the output needs %lld entries", who, (long long)out_capacity,
             (long long)nnz_out);
  if (c.added == 0 && drop == 0) {  // B is A
    if (row_ptr_out)
      SBX_HIP(h, hipMemcpyAsync(row_ptr_out, rp, ((size_t)n + 1) * sizeof(N), hipMemcpyDeviceToDevice, h->stream));
    if (col_out) {
      SBX_HIP(h, hipMemcpyAsync(col_out, col, (size_t)nnz * sizeof(I), hipMemcpyDeviceToDevice, h->stream));
      if (vb) SBX_HIP(h, hipMemcpyAsync(val_out, val, (size_t)nnz * vb, hipMemcpyDeviceToDevice, h->stream));
    }
    return SBX_OK;
  }
  if (!row_ptr_out && !col_out) return SBX_OK;
  uint32_t *tptr = nullptr, *srp = nullptr, *dcnt = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)n + 1, &tptr));
  SBX_TRY(sbx_salloc(h, (size_t)n + 1, &srp));
  const unsigned gn = sy_grid(h, n + 1);
  SBX_KLAUNCH(h, SBX_K_CSC, k_sym_offsets, dim3(gn), dim3(SY), (const uint64_t *)c.tkey, nnz, n, tptr);
  if (drop) {
    SBX_TRY(sbx_salloc(h, (size_t)n, &dcnt));
    SBX_KLAUNCH(h, SBX_K_CSC, (k_sym_diag<I, N>), dim3(gn), dim3(SY), rp, col, n, dcnt);
  }
  SBX_LAUNCH_CHECK(h);
  if (c.added) {
    SBX_TRY(sbx_exclusive_scan_u32(h, c.keep, c.keep, nnz, c.keep + nnz));
  } else {  // (the keep pass left at once: no flag was written)
    SBX_HIP(h, hipMemsetAsync(c.keep, 0, ((size_t)nnz + 1) * sizeof(uint32_t), h->stream));
  }
  SBX_KLAUNCH(h, SBX_K_CSC, (k_sym_rowlen<N>), dim3(gn), dim3(SY), rp, n, (const uint32_t *)tptr, (const uint32_t *)c.keep,
              (const uint32_t *)dcnt, srp);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_exclusive_scan_u32(h, srp, srp, n, srp + n));
  if (row_ptr_out) {
    SBX_KLAUNCH(h, SBX_K_CSC, (k_sym_offsets_out<N>), dim3(gn), dim3(SY), (const uint32_t *)srp, n, (N *)row_ptr_out);
    SBX_LAUNCH_CHECK(h);
  }
  if (!col_out) return SBX_OK;
  if (vb == 0) return sy_emit<I, N, SyNoValue>(c, rp, col, val, tptr, dcnt, srp, nnz_out, col_out, val_out);
  if (vb == 4) return sy_emit<I, N, uint32_t>(c, rp, col, val, tptr, dcnt, srp, nnz_out, col_out, val_out);
  return sy_emit<I, N, uint64_t>(c, rp, col, val, tptr, dcnt, srp, nnz_out, col_out, val_out);
}

// the argument checks both entry points share
static int sy_check_args(sbx_handle_t h, const char *who, sbx_index_type it, int64_t n, int64_t nnz, const void *row_ptr,
                         const void *col) {
  if (!(n >= 0 && nnz >= 0 && (n > 0 || nnz == 0) && (n == 0 || row_ptr) && (nnz == 0 || col)))
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: bad argument", who);
  if (!(it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: unknown index type", who);
  if (n >= ((int64_t)1 << 31) - 1) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: n = %lld >= 2^31 - 1", who, (long long)n);
  if (nnz >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: nnz = %lld >= 2^31", who, (long long)nnz);
  return SBX_OK;
}

}  // namespace

extern "C" int sbsym_csr_missing_mirrors(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t nnz, const void *row_ptr,
                                         const void *col, int64_t *missing_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, missing_host != nullptr, "missing_host is NULL");
  SBX_TRY(sy_check_args(h, __func__, it, n, nnz, row_ptr, col));
  *missing_host = 0;
  if (nnz == 0) return SBX_OK;
  if (it == SBX_I32) return sy_missing<int32_t, int32_t>(h, n, nnz, row_ptr, col, missing_host);
  if (it == SBX_I32_N64) return sy_missing<int32_t, int64_t>(h, n, nnz, row_ptr, col, missing_host);
  return sy_missing<int64_t, int64_t>(h, n, nnz, row_ptr, col, missing_host);
}

extern "C" int sbsym_csr_symmetrize(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t nnz,
                                    const void *row_ptr, const void *col, const void *val, unsigned flags,
                                    int64_t out_capacity, void *row_ptr_out, void *col_out, void *val_out,
                                    int64_t *nnz_out_host, int64_t *added_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_TRY(sy_check_args(h, __func__, it, n, nnz, row_ptr, col));
  SBX_REQUIRE(h, (flags & ~(SBSYM_NO_DIAGONAL | SBSYM_SKIP_IF_SYMMETRIC)) == 0, "unknown flag");
  const int vb = sbx_value_bytes(vt);
  SBX_REQUIRE(h, vb >= 0, "unknown value type");
  SBX_REQUIRE(h, out_capacity >= 0 || !col_out, "negative out_capacity");
  SBX_REQUIRE(h, vb == 0 || ((nnz == 0 || val) && (!col_out || val_out)), "a value type without val or val_out");
  if (nnz_out_host) *nnz_out_host = 0;
  if (added_host) *added_host = 0;
  if (nnz == 0) {  // B is A: n + 1 zero offsets
    if (row_ptr_out && !(flags & SBSYM_SKIP_IF_SYMMETRIC)) {
      SBX_HIP(h, hipSetDevice(h->device));
      SBX_HIP(h, hipMemsetAsync(row_ptr_out, 0, ((size_t)n + 1) * sbx_index_bytes(it), h->stream));  // (offset width)
    }
    return SBX_OK;
  }
  if (it == SBX_I32)
    return sy_symmetrize<int32_t, int32_t>(h, vb, n, nnz, row_ptr, col, val, flags, out_capacity, row_ptr_out, col_out,
                                           val_out, nnz_out_host, added_host);
  if (it == SBX_I32_N64)
    return sy_symmetrize<int32_t, int64_t>(h, vb, n, nnz, row_ptr, col, val, flags, out_capacity, row_ptr_out, col_out,
                                           val_out, nnz_out_host, added_host);
  return sy_symmetrize<int64_t, int64_t>(h, vb, n, nnz, row_ptr, col, val, flags, out_capacity, row_ptr_out, col_out,
                                         val_out, nnz_out_host, added_host);
}
