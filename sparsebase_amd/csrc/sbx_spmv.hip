// sbx_spmv.hip — y = A x of a CSR matrix, deterministic, balanced over the stored entries (include/sbmv.h).
// Rows, columns and positions are 64-bit inside; the arrays are read at the width of their index tuple.
//
//   spans    first[t] = the row of entry t * MV_TILE, one thread per tile (the search in row_ptr a workgroup would
//            otherwise do for itself); first[tiles] = n - 1
//   tile     one workgroup per tile of MV_TILE consecutive entries, MV_ITEMS consecutive entries per thread: columns and
//            values in 16-byte loads, x gathered, the row of an entry searched between the row of the entry before it
//            and the tile's last row (the end of the current row is kept: no load while the entries stay below it).  A thread adds its products run by run (a
//            run: consecutive entries of one row); runs that begin and end inside the thread are rows complete in this
//            tile and go to y; the thread's last run enters a segmented scan over the threads (keyed by row, DPP-free:
//            __shfl_up and a ballot of the segment heads, then the four waves' totals through LDS), which closes the
//            runs that cross threads.  The tile's LAST run never goes to y: (row, sum) goes to the carry arrays.
//   carry    one thread per tile: where a tile's carry row differs from the tile before, the carries of that row are
//            added in tile order and then the part of the row that a tile wrote to y (or the 0 the memset left).
// y is zeroed first: a row without entries is never touched again.  Every row is written once per kernel at most, every
// sum has an order fixed by the positions of the entries: no atomics, the same bits on every call.
// Malformed input: a column outside [0, m) gives a product of 0 without a load; every row a search returns lies between
// first[t] and first[t + 1], both in [0, n - 1], whatever row_ptr holds; carries are indexed by tile.
#include <cstddef>

#include "sbmv.h"
#include "sbx_device.h"
#include "sbx_internal.h"

#ifndef MV_ITEMS
#define MV_ITEMS 8  // consecutive entries per thread: two 16-byte loads of 4-byte columns (sbx_load_items8 is written for 8)
#endif

namespace {

constexpr int MV = 256;                  // threads per workgroup
constexpr int MV_TILE = MV * MV_ITEMS;   // entries per tile: 2048
static_assert(MV_ITEMS == 8, "sbx_load_items8 and sbx_load_values8 load eight entries");

// ---- sbmv_csr_check ------------------------------------------------------------------------------------------------
struct alignas(128) MvCheck {
  unsigned long long dec_row;  // the first row i with row_ptr[i] > row_ptr[i + 1]
  unsigned long long bad_pos;  // the first position p with col[p] outside [0, m)
  long long rp0, rpn;          // row_ptr[0], row_ptr[n]
};
constexpr unsigned long long MV_NONE = ~0ull;

template <typename I, typename N>
__global__ __launch_bounds__(MV) void k_mv_check(const N *__restrict__ rp, const I *__restrict__ col, int64_t n, int64_t m,
                                                 int64_t nnz, MvCheck *__restrict__ dv) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dv->rp0 = (long long)rp[0];
    dv->rpn = (long long)rp[n];
  }
  const int64_t stride = (int64_t)gridDim.x * MV;
  unsigned long long dec = MV_NONE, bad = MV_NONE;
  for (int64_t i = (int64_t)blockIdx.x * MV + threadIdx.x; i < n; i += stride)
    if ((int64_t)rp[i] > (int64_t)rp[i + 1] && (unsigned long long)i < dec) dec = (unsigned long long)i;
  for (int64_t p = (int64_t)blockIdx.x * MV + threadIdx.x; p < nnz; p += stride)
    if ((uint64_t)(int64_t)col[p] >= (uint64_t)m && (unsigned long long)p < bad) bad = (unsigned long long)p;
  dec = sbx_wave_min(dec);
  bad = sbx_wave_min(bad);
  if (sbx_lane() == 0) {
    if (dec != MV_NONE) atomicMin(&dv->dec_row, dec);
    if (bad != MV_NONE) atomicMin(&dv->bad_pos, bad);
  }
}

// ---- sbmv_csr_spmv -------------------------------------------------------------------------------------------------
// the last row r in [ra, rb] with rp[r] <= p, given ra <= rb; a row_ptr that is not ascending gives some row of [ra, rb]
template <typename N>
__device__ __forceinline__ int64_t mv_row_of(const N *__restrict__ rp, int64_t p, int64_t ra, int64_t rb) {
  if (ra == rb || (int64_t)rp[ra + 1] > p) return ra;  // (the common case: the row of the entry before)
  int64_t lo = ra + 1, hi = rb;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if ((int64_t)rp[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <typename I, typename N, typename V>
__global__ __launch_bounds__(MV) void k_spmv_tile(const N *__restrict__ rp, const I *__restrict__ col,
                                                  const V *__restrict__ val, const V *__restrict__ x, int64_t m, int64_t nnz,
                                                  const int64_t *__restrict__ first, bool col_vec, bool val_vec,
                                                  V *__restrict__ y, int64_t *__restrict__ trow, V *__restrict__ tsum) {
  __shared__ int64_t s_head[MV], s_tail[MV];  // the rows of every thread's first and last run
  __shared__ V s_sum[MV];                     // the scanned sum of every thread's last run
  __shared__ V s_wsum[MV / 64];
  __shared__ int s_whead[MV / 64];
  const int tid = (int)threadIdx.x, lane = sbx_lane(), w = sbx_wave_in_block();
  const int64_t t = blockIdx.x;
  const int64_t t0 = t * MV_TILE, t1 = t0 + MV_TILE < nnz ? t0 + MV_TILE : nnz;
  const int64_t r0 = first[t];
  const int64_t r1 = first[t + 1] < r0 ? r0 : first[t + 1];
  const int64_t base = t0 + (int64_t)tid * MV_ITEMS;

  I c[MV_ITEMS];
  V v[MV_ITEMS], prod[MV_ITEMS];
  sbx_load_items8(col, base, t1, col_vec, c);
  if (val) {
    sbx_load_values8(val, base, t1, val_vec, v);
  } else {
#pragma unroll
    for (int k = 0; k < MV_ITEMS; k++) v[k] = (V)1;
  }
#pragma unroll
  for (int k = 0; k < MV_ITEMS; k++) {  // the gathers: eight loads in flight; a slot past t1 and a column outside [0, m) load nothing
    const int64_t cc = (int64_t)c[k];
    const bool ok = base + k < t1 && (uint64_t)cc < (uint64_t)m;
    V xv = (V)0;
    if (ok) xv = x[cc];
    prod[k] = ok ? (V)(v[k] * xv) : (V)0;
  }

  // the thread's runs.  (A sum begins at +0: an exact zero never comes out as -0.)
  int64_t r = mv_row_of(rp, base < t1 ? base : t1 - 1, r0, r1);
  int64_t row_end = r < r1 ? (int64_t)rp[r + 1] : INT64_MAX;  // entries below it stay in row r: no load, no search
  const int64_t head_row = r;
  V acc = (V)0, head_sum = (V)0;
  bool multi = false;  // more than one run: the first has ended inside this thread, the last began inside it
#pragma unroll
  for (int k = 0; k < MV_ITEMS; k++) {
    if (k > 0 && base + k < t1 && base + k >= row_end) {
      const int64_t rk = mv_row_of(rp, base + k, r, r1);
      if (rk != r) {
        if (!multi) {
          head_sum = acc;
          multi = true;
        } else {
          y[r] = acc;  // a row that begins and ends inside this thread
        }
        r = rk;
        acc = (V)0;
      }
      row_end = r < r1 ? (int64_t)rp[r + 1] : INT64_MAX;
    }
    acc = acc + prod[k];
  }

  // segmented inclusive scan of the last runs over the workgroup's threads; a segment begins where a run does
  s_head[tid] = head_row;
  s_tail[tid] = r;
  __syncthreads();
  const bool seg_head = multi || tid == 0 || s_tail[tid - 1] != head_row;
  const uint64_t heads = __ballot(seg_head);
  const uint64_t at_or_before = heads & (sbx_lanemask_lt() | ((uint64_t)1 << lane));
  const int seg_lane = at_or_before ? 63 - __builtin_clzll(at_or_before) : -1;  // -1: the segment began in an earlier wave
  const int from = seg_lane < 0 ? 0 : seg_lane;
  V s = acc;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const V o = __shfl_up(s, d, 64);
    if (lane - d >= from) s = o + s;
  }
  if (lane == 63) {
    s_wsum[w] = s;
    s_whead[w] = heads != 0;
  }
  __syncthreads();
  if (seg_lane < 0) {  // (never in wave 0: thread 0 is a head)
    V before = (V)0;
#pragma unroll
    for (int i = 0; i < MV / 64; i++)
      if (i < w) before = s_whead[i] ? s_wsum[i] : (V)(before + s_wsum[i]);
    s = before + s;
  }
  s_sum[tid] = s;
  __syncthreads();

  if (multi) {  // the first run ended here: what the threads before added to this row, then this thread's part
    const V before = (tid > 0 && s_tail[tid - 1] == head_row) ? s_sum[tid - 1] : (V)0;
    y[head_row] = before + head_sum;
  }
  if (tid == MV - 1) {  // the tile's last run: to the carry arrays, whether or not the row ends here
    trow[t] = r;
    tsum[t] = s;
  } else if (s_head[tid + 1] != r) {
    y[r] = s;
  }
}

// the carries of one row, in tile order, then what a tile wrote to y for that row (its end) or the 0 of the memset
template <typename V>
__global__ __launch_bounds__(MV) void k_spmv_carry(const int64_t *__restrict__ trow, const V *__restrict__ tsum,
                                                   int64_t tiles, V *__restrict__ y) {
  const int64_t t = (int64_t)blockIdx.x * MV + threadIdx.x;
  if (t >= tiles) return;
  const int64_t r = trow[t];
  if (t > 0 && trow[t - 1] == r) return;
  V s = (V)0;
  for (int64_t u = t; u < tiles; u += 8) {  // eight independent loads a round: a hub row's chain is not a chain of misses
    int64_t rr[8];
    V ss[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const bool in = u + k < tiles;
      rr[k] = in ? trow[u + k] : -1;
      ss[k] = in ? tsum[u + k] : (V)0;
    }
    bool more = true;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      more = more && rr[k] == r;
      if (more) s = s + ss[k];
    }
    if (!more) break;
  }
  y[r] = s + y[r];
}

template <typename I, typename N, typename V>
static int mv_spmv(sbx_handle_t h, int64_t n, int64_t m, int64_t nnz, const void *row_ptr, const void *col, const void *val,
                   const void *x, void *y) {
  SBX_HIP(h, hipSetDevice(h->device));
  SBX_HIP(h, hipMemsetAsync(y, 0, (size_t)n * sizeof(V), h->stream));
  if (nnz == 0) return SBX_OK;
  SBX_TRY(sbx_arena_begin(h));
  const int64_t tiles = (nnz + MV_TILE - 1) / MV_TILE;
  int64_t *first = nullptr, *trow = nullptr;
  V *tsum = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)tiles + 1, &first));
  SBX_TRY(sbx_salloc(h, (size_t)tiles, &trow));
  SBX_TRY(sbx_salloc(h, (size_t)tiles, &tsum));
  const unsigned gt = (unsigned)((tiles + 1 + MV - 1) / MV);
  SBX_KLAUNCH(h, SBX_K_SPMV, (k_tile_first_rows<N, MV_TILE, MV>), dim3(gt), dim3(MV), (const N *)row_ptr, n, tiles, first);
  SBX_KLAUNCH(h, SBX_K_SPMV, (k_spmv_tile<I, N, V>), dim3((unsigned)tiles), dim3(MV), (const N *)row_ptr, (const I *)col,
              (const V *)val, (const V *)x, m, nnz, (const int64_t *)first, ((uintptr_t)col & 15) == 0,
              ((uintptr_t)val & 15) == 0, (V *)y, trow, tsum);
  SBX_KLAUNCH(h, SBX_K_SPMV, (k_spmv_carry<V>), dim3(gt), dim3(MV), (const int64_t *)trow, (const V *)tsum, tiles, (V *)y);
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_SPMV, nnz * (int64_t)(sizeof(I) + (val ? sizeof(V) : 0)) + n * (int64_t)(sizeof(N) + sizeof(V)) +
                                    m * (int64_t)sizeof(V));
  return SBX_OK;
}

template <typename I, typename N>
static int mv_spmv_v(sbx_handle_t h, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, const void *row_ptr,
                     const void *col, const void *val, const void *x, void *y) {
  switch (vt) {
    case SBX_V_F32: return mv_spmv<I, N, float>(h, n, m, nnz, row_ptr, col, val, x, y);
    case SBX_V_F64: return mv_spmv<I, N, double>(h, n, m, nnz, row_ptr, col, val, x, y);
    case SBX_V_I32: case SBX_V_U32: return mv_spmv<I, N, uint32_t>(h, n, m, nnz, row_ptr, col, val, x, y);
    default: return mv_spmv<I, N, uint64_t>(h, n, m, nnz, row_ptr, col, val, x, y);  // SBX_V_I64, SBX_V_U64
  }
}

template <typename I, typename N>
static int mv_check(sbx_handle_t h, const char *who, int64_t n, int64_t m, int64_t nnz, const void *row_ptr, const void *col) {
  SBX_HIP(h, hipSetDevice(h->device));
  SBX_TRY(sbx_arena_begin(h));
  MvCheck *dv = nullptr;
  SBX_TRY(sbx_salloc(h, 1, &dv));
  SBX_HIP(h, hipMemsetAsync(dv, 0xFF, sizeof(MvCheck), h->stream));
  const int64_t items = n > nnz ? n : nnz;
  SBX_KLAUNCH(h, SBX_K_SPMV, (k_mv_check<I, N>), dim3(sbx_grid_for(items, MV, (int64_t)h->num_cus * 32)), dim3(MV),
              (const N *)row_ptr, (const I *)col, n, m, nnz, dv);
  SBX_LAUNCH_CHECK(h);
  MvCheck rb;
  SBX_TRY(sbx_readback(h, &rb, dv, sizeof(rb)));
  if (rb.rp0 != 0) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: row_ptr[0] is %lld, not 0", who, rb.rp0);
  if (rb.dec_row != MV_NONE)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: row_ptr decreases at row %llu (row_ptr[%llu] > row_ptr[%llu])", who, rb.dec_row,
             rb.dec_row, rb.dec_row + 1);
  if (rb.rpn != nnz)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: row_ptr[n] = row_ptr[%lld] is %lld, not nnz = %lld", who, (long long)n, rb.rpn,
             (long long)nnz);
  if (rb.bad_pos != MV_NONE)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: the column at position %llu lies outside [0, %lld)", who, rb.bad_pos, (long long)m);
  return SBX_OK;
}

// the argument checks both entry points share
static int mv_check_args(sbx_handle_t h, const char *who, sbx_index_type it, int64_t n, int64_t m, int64_t nnz,
                         const void *row_ptr, const void *col) {
  if (!(n >= 0 && m >= 0 && nnz >= 0 && (n > 0 || nnz == 0) && (n == 0 || row_ptr) && (nnz == 0 || col)))
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: bad argument", who);
  if (!(it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: unknown index type", who);
  if (nnz >= ((int64_t)1 << 42)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: nnz = %lld >= 2^42", who, (long long)nnz);
  return SBX_OK;
}

}  // namespace

extern "C" int sbmv_csr_check(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t m, int64_t nnz, const void *row_ptr,
                              const void *col) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_TRY(mv_check_args(h, __func__, it, n, m, nnz, row_ptr, col));
  if (n == 0) return SBX_OK;
  if (it == SBX_I32) return mv_check<int32_t, int32_t>(h, __func__, n, m, nnz, row_ptr, col);
  if (it == SBX_I32_N64) return mv_check<int32_t, int64_t>(h, __func__, n, m, nnz, row_ptr, col);
  return mv_check<int64_t, int64_t>(h, __func__, n, m, nnz, row_ptr, col);
}

extern "C" int sbmv_csr_spmv(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz,
                             const void *row_ptr, const void *col, const void *val, const void *x, void *y) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_TRY(mv_check_args(h, __func__, it, n, m, nnz, row_ptr, col));
  SBX_REQUIRE(h, vt != SBX_V_NONE && sbx_value_bytes(vt) > 0, "the value type must be one of F32, F64, I32, U32, I64, U64");
  SBX_REQUIRE(h, x != nullptr || m == 0 || nnz == 0, "x is NULL");
  SBX_REQUIRE(h, y != nullptr || n == 0, "y is NULL");
  if (n == 0) return SBX_OK;
  if (it == SBX_I32) return mv_spmv_v<int32_t, int32_t>(h, vt, n, m, nnz, row_ptr, col, val, x, y);
  if (it == SBX_I32_N64) return mv_spmv_v<int32_t, int64_t>(h, vt, n, m, nnz, row_ptr, col, val, x, y);
  return mv_spmv_v<int64_t, int64_t>(h, vt, n, m, nnz, row_ptr, col, val, x, y);
}
