// sbx_softmax.hip — the softmax over the stored entries of every row of a CSR matrix and its backward, deterministic,
// balanced over the stored entries (include/sbsm.h).  No column is read; rows and positions are 64-bit.
//
//   spans    first[t] = the row of entry t * SM_TILE (k_tile_first_rows, shared with the products); first[tiles] = n - 1
//   tile     one workgroup per tile of SM_TILE consecutive entries, SM_ITEMS consecutive entries per thread, their rows
//            searched as sbx_spmv.hip searches them.  A run is a maximal stretch of one row inside the tile; a thread
//            knows where its entries' runs begin (SmRuns) and the index of each run in the tile.  sm_run_totals gives
//            every entry the total of its run under a fold (max, sum of exp, sum of s g): left to right inside the
//            thread, a segmented scan in a fixed tree over the threads, the run's last entry writes the total to a table
//            in LDS, everyone reads it back.  A run whose row begins and ends inside the tile is finished here.  The
//            tile's first run, if its row began earlier, and its last run, if its row goes on, write nothing to `out`:
//            they leave (row, m, s) in the tile's two slots, s relative to the run's own m.
//   carry    one thread per chain of consecutive slots of one row: m = max m_t, s = sum of s_t exp(m_t - m) in slot
//            order, written back into every slot of the chain.
//   fix-up   one workgroup per tile that has an open run: the entries of those runs from the slot's (m, s).  `val` is read
//            here for the second time and `out` written for the first: out == val is safe.
// Every out[p] is written once, by the tile kernel or by the fix-up; every sum has an order fixed by the positions of the
// entries: no atomics, the same bits on every call.
// Malformed input: every row a search returns lies between first[t] and first[t + 1], both in [0, n - 1], whatever
// row_ptr holds; slots are indexed by tile, extents are offsets inside the tile, and which of the two kernels writes an
// entry is decided by the tile kernel alone and read back by the fix-up.
#include <cstddef>

#include "sbsm.h"
#include "sbx_device.h"
#include "sbx_internal.h"

namespace {

constexpr int SM = 256;                 // threads per workgroup
constexpr int SM_ITEMS = 8;             // consecutive entries per thread (sbx_load_values8 is written for 8)
constexpr int SM_TILE = SM * SM_ITEMS;  // entries per tile: 2048
enum { SM_FWD = 0, SM_PATTERN = 1, SM_BWD = 2 };

template <typename V>
__device__ __forceinline__ V sm_exp(V x) {  // the device library's exp, not the fast intrinsic
  if constexpr (sizeof(V) == 4) return expf(x); else return exp(x);
}
template <typename V>
__device__ __forceinline__ V sm_fma(V a, V b, V c) {
  if constexpr (sizeof(V) == 4) return __builtin_fmaf(a, b, c); else return __builtin_fma(a, b, c);
}
template <typename V>
__device__ __forceinline__ V sm_neg_inf() { return -std::numeric_limits<V>::infinity(); }
// what the exponent is taken against: the maximum, or 0 where every entry is -inf (exp(-inf - 0) = 0, no inf - inf)
template <typename V>
__device__ __forceinline__ V sm_shift(V m) { return m == sm_neg_inf<V>() ? (V)0 : m; }

// the two slots of a tile: [2t] its first run, [2t + 1] its last run.  row >= 0: an open run of that row; -1: none;
// -2 - row: the tile is one open run of that row, kept in [2t + 1] (the chain of the row passes through [2t])
template <typename V>
struct SmSlots {
  int64_t *row;
  V *m, *s;  // m: forward with values alone
  int *ext;  // [2t]: where the first run ends, [2t + 1]: where the last run begins, as offsets into the tile
};
__device__ __forceinline__ int64_t sm_slot_key(int64_t raw) { return raw >= -1 ? raw : -2 - raw; }

// where the runs of a thread's eight entries lie
struct SmRuns {
  unsigned heads;  // bit k: entry k begins a run (bit 0: the thread before ended in another row, or there is none)
  int run0;        // the index in the tile of the run of entry 0
  bool last_ends;  // entry 7 ends a run
  __device__ __forceinline__ bool head(int k) const { return (heads >> k) & 1u; }
  __device__ __forceinline__ bool tail(int k) const { return k == SM_ITEMS - 1 ? last_ends : ((heads >> (k + 1)) & 1u) != 0; }
  __device__ __forceinline__ int run(int k) const { return run0 + __popc(heads & ((2u << k) - 2u)); }
};

// The rows of the thread's entries [base, base + 8) of a tile ending at t1, between the tile's rows r0 <= r1; a slot past
// t1 stays in the row of the tile's last entry.  Three barriers.
template <typename N>
__device__ __forceinline__ SmRuns sm_find_runs(const N *__restrict__ rp, int64_t base, int64_t t1, int64_t r0, int64_t r1,
                                               int64_t *s_head, int64_t *s_tail, int *s_cnt, int64_t &head_row,
                                               int64_t &tail_row, int &nruns) {
  const int tid = (int)threadIdx.x;
  int64_t r = r0 == r1 ? r0 : sbx_row_of(rp, base < t1 ? base : t1 - 1, r0, r1);
  int64_t row_end = r < r1 ? (int64_t)rp[r + 1] : INT64_MAX;  // entries below it stay in row r: no load, no search
  head_row = r;
  unsigned heads = 0;
#pragma unroll
  for (int k = 1; k < SM_ITEMS; k++) {
    if (base + k < t1 && base + k >= row_end) {  // (then r < r1)
      r = sbx_row_of(rp, base + k, r, r1);
      heads |= 1u << k;
      row_end = r < r1 ? (int64_t)rp[r + 1] : INT64_MAX;
    }
  }
  tail_row = r;
  s_head[tid] = head_row;
  s_tail[tid] = r;
  __syncthreads();
  if (tid == 0 || s_tail[tid - 1] != head_row) heads |= 1u;
  SmRuns g;
  g.heads = heads;
  g.last_ends = tid == SM - 1 || s_head[tid + 1] != r;
  const int before = sbx_block_exclusive_sum<int, SM>(__popc(heads), s_cnt, &nruns);
  g.run0 = before - 1 + (int)(heads & 1u);  // (thread 0 has bit 0: never negative)
  return g;
}

template <typename V>
struct SmScanLds {
  V *scan;     // SM: the scanned last runs of the threads
  V *wsum;     // SM / 64
  int *whead;  // SM / 64
  V *tab;      // SM_TILE: the total of every run of the tile
};

// tot[k] = the total of the run of entry k.  fold(acc, k, fresh) takes entry k into acc (fresh: k begins the thread's
// part of a run and acc is to be ignored); op joins the parts of a run that crosses threads, earlier part first.
// The order: inside a thread left to right; over the threads of a wave the segmented Hillis-Steele scan of sbx_spmv.hip
// (steps d = 1, 2, ... 32: lane i takes op(lane i - d, lane i) where lane i - d is not before the last thread of the wave
// at or before lane i in which a run begins); the waves' totals in wave order.  Three barriers.
template <typename V, typename Fold, typename Op>
__device__ __forceinline__ void sm_run_totals(const SmRuns &g, Fold fold, Op op, const SmScanLds<V> &L, V (&tot)[SM_ITEMS]) {
  const int tid = (int)threadIdx.x, lane = sbx_lane(), w = sbx_wave_in_block();
  V pre[SM_ITEMS], acc = (V)0;
#pragma unroll
  for (int k = 0; k < SM_ITEMS; k++) {
    acc = fold(acc, k, k == 0 || g.head(k));
    pre[k] = acc;
  }
  const uint64_t heads = __ballot(g.heads != 0);
  const uint64_t at_or_before = heads & (sbx_lanemask_lt() | ((uint64_t)1 << lane));
  const int seg_lane = at_or_before ? 63 - __builtin_clzll(at_or_before) : -1;  // -1: the run began in an earlier wave
  const int from = seg_lane < 0 ? 0 : seg_lane;
  V s = acc;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const V o = __shfl_up(s, d, 64);
    if (lane - d >= from) s = op(o, s);
  }
  if (lane == 63) {
    L.wsum[w] = s;
    L.whead[w] = heads != 0;
  }
  __syncthreads();
  if (seg_lane < 0 && w > 0) {  // (never in wave 0: thread 0 begins a run)
    V before = L.wsum[0];
#pragma unroll
    for (int i = 1; i < SM / 64; i++)
      if (i < w) before = L.whead[i] ? L.wsum[i] : op(before, L.wsum[i]);
    s = op(before, s);
  }
  L.scan[tid] = s;
  __syncthreads();
  bool joined = (g.heads & 1u) == 0;  // the thread's first entries go on a run of the thread before
  const V before = joined ? L.scan[tid - 1] : (V)0;
#pragma unroll
  for (int k = 0; k < SM_ITEMS; k++) {
    if (k > 0 && g.head(k)) joined = false;
    if (g.tail(k)) L.tab[g.run(k)] = joined ? op(before, pre[k]) : pre[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SM_ITEMS; k++) tot[k] = L.tab[g.run(k)];
}

template <typename V>
__device__ __forceinline__ void sm_store_values8(V *out, int64_t base, const V *o) {  // 16-byte stores
  if constexpr (sizeof(V) == 4) {
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = __builtin_bit_cast(uint32_t, o[k]);
    *(uint4 *)(out + base) = make_uint4(w[0], w[1], w[2], w[3]);
    *(uint4 *)(out + base + 4) = make_uint4(w[4], w[5], w[6], w[7]);
  } else {
#pragma unroll
    for (int k = 0; k < 8; k += 2)
      *(ulonglong2 *)(out + base + k) =
          make_ulonglong2(__builtin_bit_cast(uint64_t, o[k]), __builtin_bit_cast(uint64_t, o[k + 1]));
  }
}

// a: val (SM_FWD), nothing (SM_PATTERN), s (SM_BWD); b: g (SM_BWD).  out may be a (SM_FWD) or b (SM_BWD): a thread loads
// its eight entries before it stores any, and no thread reads another's.
template <typename N, typename V, int MODE>
__global__ __launch_bounds__(SM) void k_sm_tile(const N *__restrict__ rp, const V *a, const V *b, int64_t nnz,
                                                const int64_t *__restrict__ first, bool a_vec, bool b_vec, bool out_vec,
                                                V *out, SmSlots<V> slots) {
  __shared__ int64_t s_head[SM], s_tail[SM];
  __shared__ V s_scan[SM], s_wsum[SM / 64], s_tab[SM_TILE];
  __shared__ int s_whead[SM / 64], s_cnt[SM / 64 + 1], s_open[2];
  const int tid = (int)threadIdx.x;
  const int64_t t = blockIdx.x;
  const int64_t t0 = t * SM_TILE, t1 = t0 + SM_TILE < nnz ? t0 + SM_TILE : nnz;
  const int64_t r0 = first[t];
  const int64_t r1 = first[t + 1] < r0 ? r0 : first[t + 1];
  const int64_t base = t0 + (int64_t)tid * SM_ITEMS;

  V x[SM_ITEMS], y[SM_ITEMS];
  if constexpr (MODE != SM_PATTERN) sbx_load_values8(a, base, t1, a_vec, x);
  if constexpr (MODE == SM_BWD) sbx_load_values8(b, base, t1, b_vec, y);

  int64_t head_row, tail_row;
  int nruns;
  const SmRuns g = sm_find_runs(rp, base, t1, r0, r1, s_head, s_tail, s_cnt, head_row, tail_row, nruns);
  if (tid == 0) s_open[0] = t > 0 && (int64_t)rp[head_row] < t0;               // the first row began in an earlier tile
  if (tid == SM - 1) s_open[1] = t1 < nnz && (int64_t)rp[tail_row + 1] > t1;  // the last row goes on in the next one
  const SmScanLds<V> L{s_scan, s_wsum, s_whead, s_tab};

  // m: the maximum of the entry's run (SM_FWD); e: exp(val - m), 1 for a pattern; s: the sum of e, or of s g (SM_BWD)
  V m[SM_ITEMS], e[SM_ITEMS], s[SM_ITEMS];
  if constexpr (MODE == SM_FWD) {
#pragma unroll
    for (int k = 0; k < SM_ITEMS; k++)
      if (base + k >= t1) x[k] = sm_neg_inf<V>();
    sm_run_totals(g, [&](V acc, int k, bool fresh) { return fresh || !(acc > x[k]) ? x[k] : acc; }, SbxOpMax(), L, m);
#pragma unroll
    for (int k = 0; k < SM_ITEMS; k++) e[k] = base + k < t1 ? sm_exp((V)(x[k] - sm_shift(m[k]))) : (V)0;
  } else if constexpr (MODE == SM_PATTERN) {
#pragma unroll
    for (int k = 0; k < SM_ITEMS; k++) {
      m[k] = (V)0;
      e[k] = base + k < t1 ? (V)1 : (V)0;
    }
  } else {
#pragma unroll
    for (int k = 0; k < SM_ITEMS; k++) {
      m[k] = (V)0;
      if (base + k >= t1) x[k] = y[k] = (V)0;
    }
  }
  if constexpr (MODE == SM_BWD)
    sm_run_totals(g, [&](V acc, int k, bool fresh) { return sm_fma(x[k], y[k], fresh ? (V)0 : acc); }, SbxOpSum(), L, s);
  else
    sm_run_totals(g, [&](V acc, int k, bool fresh) { return fresh ? e[k] : (V)(acc + e[k]); }, SbxOpSum(), L, s);

  // (s_open was written before the barriers of sm_run_totals)
  const bool open_l = s_open[0] != 0, open_r = s_open[1] != 0;
  const int last = nruns - 1;
  V o[SM_ITEMS];
  unsigned open = 0;  // bit k: entry k lies in an open run, the fix-up's to write
#pragma unroll
  for (int k = 0; k < SM_ITEMS; k++) {
    const int rk = g.run(k);
    if ((rk == 0 && open_l) || (rk == last && open_r)) open |= 1u << k;
    if constexpr (MODE == SM_BWD) o[k] = x[k] * (V)(y[k] - s[k]);
    else o[k] = s[k] == (V)0 ? (V)0 : (V)(e[k] / s[k]);  // (a sum of 0: every entry of the row is -inf)
    if (g.head(k)) {  // where the first run ends and the last begins
      if (rk == 1) slots.ext[2 * t] = tid * SM_ITEMS + k;
      if (rk == last) slots.ext[2 * t + 1] = tid * SM_ITEMS + k;
    }
  }
  if (open == 0 && out_vec && base + SM_ITEMS <= t1) {
    sm_store_values8(out, base, o);
  } else {
#pragma unroll
    for (int k = 0; k < SM_ITEMS; k++)
      if (!((open >> k) & 1u) && base + k < t1) out[base + k] = o[k];
  }

  if (tid == 0) {
    const bool slot = nruns > 1 && open_l;
    slots.row[2 * t] = slot ? head_row : (nruns == 1 && (open_l || open_r) ? -2 - head_row : -1);
    if (nruns == 1) slots.ext[2 * t] = SM_TILE;
    if (slot) {
      if constexpr (MODE == SM_FWD) slots.m[2 * t] = m[0];
      slots.s[2 * t] = s[0];
    }
  }
  if (tid == SM - 1) {
    const bool slot = open_r || (nruns == 1 && open_l);
    slots.row[2 * t + 1] = slot ? tail_row : -1;
    if (slot) {
      if constexpr (MODE == SM_FWD) slots.m[2 * t + 1] = m[SM_ITEMS - 1];
      slots.s[2 * t + 1] = s[SM_ITEMS - 1];
    }
  }
}

// one thread per chain: the consecutive slots of one row, the first of them here.  Eight independent loads a round: a hub
// row's chain is not a chain of misses (as k_spmv_carry).
template <typename V, int MODE>
__global__ __launch_bounds__(SM) void k_sm_carry(SmSlots<V> slots, int64_t count) {
  const int64_t j = (int64_t)blockIdx.x * SM + threadIdx.x;
  if (j >= count) return;
  const int64_t key = sm_slot_key(slots.row[j]);
  if (key < 0) return;
  if (j > 0 && sm_slot_key(slots.row[j - 1]) == key) return;
  // where the chain ends, and the maximum of its parts (any order gives the same)
  int64_t end = j;
  V m = MODE == SM_FWD ? sm_neg_inf<V>() : (V)0;
  for (bool more = true; more;) {
    int64_t raw[8];
    V mu[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      raw[k] = end + k < count ? slots.row[end + k] : -1;
      mu[k] = sm_neg_inf<V>();
      if constexpr (MODE == SM_FWD)
        if (raw[k] >= 0) mu[k] = slots.m[end + k];
    }
    int taken = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      more = more && sm_slot_key(raw[k]) == key;
      if (more) {
        taken++;
        if constexpr (MODE == SM_FWD) m = m > mu[k] ? m : mu[k];
      }
    }
    end += taken;
  }
  // the sum, in slot order
  const V shift = sm_shift(m);
  V s = (V)0;
  for (int64_t u = j; u < end; u += 8) {
    V su[8], mu[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const bool in = u + k < end && slots.row[u + k] >= 0;
      su[k] = in ? slots.s[u + k] : (V)0;
      mu[k] = (V)0;
      if constexpr (MODE == SM_FWD)
        if (in) mu[k] = slots.m[u + k];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if constexpr (MODE == SM_FWD) {
        // (0: no slot here, or a part that is all -inf, whose m_t - m may be inf - inf)
        if (su[k] != (V)0) s = sm_fma(su[k], sm_exp((V)(mu[k] - shift)), s);
      } else {
        if (u + k < end) s = s + su[k];
      }
    }
  }
  for (int64_t u = j; u < end; u++) {
    if (slots.row[u] < 0) continue;
    if constexpr (MODE == SM_FWD) slots.m[u] = m;
    slots.s[u] = s;
  }
}

// the entries of a tile's open runs, from the row's (m, s) the carry left in the slots
template <typename V, int MODE>
__global__ __launch_bounds__(SM) void k_sm_fixup(const V *a, const V *b, int64_t nnz, bool a_vec, bool b_vec, V *out,
                                                 SmSlots<V> slots) {
  const int tid = (int)threadIdx.x;
  const int64_t t = blockIdx.x;
  const bool has_h = slots.row[2 * t] >= 0, has_l = slots.row[2 * t + 1] >= 0;
  if (!has_h && !has_l) return;
  const int hend = has_h ? slots.ext[2 * t] : 0, lbeg = has_l ? slots.ext[2 * t + 1] : SM_TILE;
  const int off = tid * SM_ITEMS;
  if (off >= hend && off + SM_ITEMS <= lbeg) return;
  const int64_t t0 = t * SM_TILE, t1 = t0 + SM_TILE < nnz ? t0 + SM_TILE : nnz;
  const int64_t base = t0 + off;
  if (base >= t1) return;
  V x[SM_ITEMS], y[SM_ITEMS];
  if constexpr (MODE != SM_PATTERN) sbx_load_values8(a, base, t1, a_vec, x);
  if constexpr (MODE == SM_BWD) sbx_load_values8(b, base, t1, b_vec, y);
  V hm = (V)0, hs = (V)0, lm = (V)0, ls = (V)0;
  if (has_h) {
    if constexpr (MODE == SM_FWD) hm = sm_shift(slots.m[2 * t]);
    hs = slots.s[2 * t];
  }
  if (has_l) {
    if constexpr (MODE == SM_FWD) lm = sm_shift(slots.m[2 * t + 1]);
    ls = slots.s[2 * t + 1];
  }
#pragma unroll
  for (int k = 0; k < SM_ITEMS; k++) {
    const bool in_h = off + k < hend, in_l = off + k >= lbeg;
    if (!(in_h || in_l) || base + k >= t1) continue;
    const V m = in_h ? hm : lm, s = in_h ? hs : ls;
    V o;
    if constexpr (MODE == SM_BWD) {
      o = x[k] * (V)(y[k] - s);
    } else {
      V e = (V)1;
      if constexpr (MODE == SM_FWD) e = sm_exp((V)(x[k] - m));
      o = s == (V)0 ? (V)0 : (V)(e / s);
    }
    out[base + k] = o;
  }
}

template <typename N, typename V, int MODE>
static int sm_run(sbx_handle_t h, int64_t n, int64_t nnz, const void *row_ptr, const void *a, const void *b, void *out) {
  SBX_HIP(h, hipSetDevice(h->device));
  SBX_TRY(sbx_arena_begin(h));
  const int64_t tiles = (nnz + SM_TILE - 1) / SM_TILE;
  int64_t *first = nullptr;
  SmSlots<V> slots{nullptr, nullptr, nullptr, nullptr};
  SBX_TRY(sbx_salloc(h, (size_t)tiles + 1, &first));
  SBX_TRY(sbx_salloc(h, (size_t)tiles * 2, &slots.row));
  SBX_TRY(sbx_salloc(h, (size_t)tiles * 2, &slots.ext));
  SBX_TRY(sbx_salloc(h, (size_t)tiles * 2, &slots.s));
  if (MODE == SM_FWD) SBX_TRY(sbx_salloc(h, (size_t)tiles * 2, &slots.m));
  const bool a_vec = ((uintptr_t)a & 15) == 0, b_vec = ((uintptr_t)b & 15) == 0, out_vec = ((uintptr_t)out & 15) == 0;
  SBX_KLAUNCH(h, SBX_K_SOFTMAX, (k_tile_first_rows<N, SM_TILE, SM>), dim3((unsigned)((tiles + 1 + SM - 1) / SM)), dim3(SM),
              (const N *)row_ptr, n, tiles, first);
  SBX_KLAUNCH(h, SBX_K_SOFTMAX, (k_sm_tile<N, V, MODE>), dim3((unsigned)tiles), dim3(SM), (const N *)row_ptr, (const V *)a,
              (const V *)b, nnz, (const int64_t *)first, a_vec, b_vec, out_vec, (V *)out, slots);
  SBX_KLAUNCH(h, SBX_K_SOFTMAX, (k_sm_carry<V, MODE>), dim3((unsigned)((2 * tiles + SM - 1) / SM)), dim3(SM), slots,
              2 * tiles);
  SBX_KLAUNCH(h, SBX_K_SOFTMAX, (k_sm_fixup<V, MODE>), dim3((unsigned)tiles), dim3(SM), (const V *)a, (const V *)b, nnz,
              a_vec, b_vec, (V *)out, slots);
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_SOFTMAX, nnz * (int64_t)sizeof(V) * (MODE == SM_BWD ? 3 : MODE == SM_FWD ? 2 : 1) +
                                       n * (int64_t)sizeof(N));
  return SBX_OK;
}

// the argument checks both entry points share; `out_name` is "out" or "dz"
static int sm_check_args(sbx_handle_t h, const char *who, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t nnz,
                         const void *row_ptr, const void *out, const char *out_name) {
  if (n < 0) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: n is negative", who);
  if (nnz < 0) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: nnz is negative", who);
  if (n == 0 && nnz > 0) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: nnz > 0 with n == 0", who);
  if (!row_ptr && n > 0) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: row_ptr is NULL", who);
  if (!out && nnz > 0) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: %s is NULL", who, out_name);
  if (!(it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: unknown index type", who);
  if (vt == SBX_V_NONE || sbx_value_bytes(vt) <= 0) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: the value type must be F32", who);
  if (vt == SBX_V_F64)  // (the kernels are templates over the value type; the double instances are not built: DESIGN §4.26)
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: the value type F64 is not built yet, F32 alone", who);
  if (vt != SBX_V_F32) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: the value type is an integer type, F32 alone", who);
  if (nnz >= ((int64_t)1 << 42)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: nnz = %lld >= 2^42", who, (long long)nnz);
  return SBX_OK;
}

template <int MODE>
static int sm_dispatch(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t nnz, const void *row_ptr, const void *a,
                       const void *b, void *out) {
  if (it == SBX_I32) return sm_run<int32_t, float, MODE>(h, n, nnz, row_ptr, a, b, out);
  return sm_run<int64_t, float, MODE>(h, n, nnz, row_ptr, a, b, out);  // SBX_I64, SBX_I32_N64
}

}  // namespace

extern "C" int sbsm_csr_row_softmax(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t nnz,
                                    const void *row_ptr, const void *val, void *out) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_TRY(sm_check_args(h, __func__, it, vt, n, nnz, row_ptr, out, "out"));
  if (n == 0 || nnz == 0) return SBX_OK;
  if (!val) return sm_dispatch<SM_PATTERN>(h, it, n, nnz, row_ptr, nullptr, nullptr, out);
  return sm_dispatch<SM_FWD>(h, it, n, nnz, row_ptr, val, nullptr, out);
}

extern "C" int sbsm_csr_row_softmax_backward(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t nnz,
                                             const void *row_ptr, const void *s, const void *g, void *dz) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_TRY(sm_check_args(h, __func__, it, vt, n, nnz, row_ptr, dz, "dz"));
  SBX_REQUIRE(h, s != nullptr || nnz == 0, "s is NULL");
  SBX_REQUIRE(h, g != nullptr || nnz == 0, "g is NULL");
  if (n == 0 || nnz == 0) return SBX_OK;
  return sm_dispatch<SM_BWD>(h, it, n, nnz, row_ptr, s, g, dz);
}
