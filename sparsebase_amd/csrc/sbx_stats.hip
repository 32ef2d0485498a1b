// sbx_stats.hip — the entry points of include/sbx_stats.h: the scalar statistics of an offset array and the count of
// nonzeros outside the diagonal blocks of a block partition.
//
//   feature/avg_degree.cc, min_degree.cc, max_degree.cc, min_max_avg_degree.cc,
//   feature/*_degree_column.cc (avg, min, max, median, standard deviation,
//   coefficient of variation, geometric average)                              sbxstat_degree_stats
//   feature/off_diag_block_nnz.cc:94-116                                      sbxstat_csr_off_diag_block_nnz
//
// sbxstat_degree_stats: one pass over the offsets for min, max, zeros, the exact 128-bit sum of squares and the sum of
// logarithms, then a radix select of both median ranks over 12-bit digits, most significant first.  The host cannot
// know how many digits the largest degree has without a read-back, so it enqueues a (histogram, pick) pair for every
// digit the word type can hold and the pairs above the largest degree's top digit return at once: the passes that do
// work are as many as the maximum has digits.  Every decision between two passes (which bin holds each rank, whether
// the two ranks have parted) is taken by k_ds_pick on the device; the one read-back is the result itself.
//
// sbxstat_csr_off_diag_block_nnz: the row blocks are contiguous rows, so block p is the position range
// [row_ptr[rs_p], row_ptr[re_p]) of `col`: a table of the h + 1 bounds, one search per tile of 2048 entries for the
// blocks it touches, and a stream over `col` with 16-byte loads.
#include "sbx_device.h"
#include "sbx_internal.h"
#include "sbx_stats.h"

#ifndef SBXSTAT_MAX_GRID
#define SBXSTAT_MAX_GRID 512  // workgroups of a pass over the offsets (each flushes its LDS histogram once)
#endif
#ifndef SBXSTAT_FOLD
#define SBXSTAT_FOLD 4  // rounds in which a wave folds its lanes' equal bins into one LDS add (0: one add per lane)
#endif
#ifndef SBXSTAT_OD_GRID
#define SBXSTAT_OD_GRID 4096  // workgroups of the stream over `col`
#endif

namespace {

constexpr int DS_THREADS = 256;
constexpr int DS_ITEMS = 4;  // consecutive degrees of a thread in one step: five words, four of them in 16-byte loads
constexpr int DS_STEPS = 4;
// the unit of the deterministic sum: a tile's logarithms are added in an order that depends on nothing but the tile
constexpr int DS_TILE = DS_THREADS * DS_ITEMS * DS_STEPS;
constexpr int DS_DIGIT = 12, DS_BINS = 1 << DS_DIGIT;
constexpr int DS_WAVES = DS_THREADS / 64;

struct DsBlock {
  long long mn, mx;
  unsigned long long zeros, sq_lo, sq_hi;
};

struct DsState {
  sbxstat_degrees out;  // median_lo / median_hi hold the two ranks' key prefixes while the select runs
  long long rank[2];    // rank of each order statistic among the degrees that share its prefix
  int digits;           // 12-bit digits of the largest degree
  int split;            // the two prefixes differ
};

// degrees i .. i + 3 (i a multiple of DS_ITEMS); the ones at and beyond n are 0 and the caller leaves them out
template <typename W>
__device__ __forceinline__ void load_degrees(const W *__restrict__ ptr, int64_t i, int64_t n, bool vec_ok, long long *d) {
  static_assert(DS_ITEMS == 4, "one 16-byte load of 32-bit words, two of 64-bit words");
  W w[DS_ITEMS + 1];
  if (vec_ok && i + DS_ITEMS <= n) {
    if (sizeof(W) == 4) {
      const int4 a = *(const int4 *)(ptr + i);
      w[0] = (W)a.x; w[1] = (W)a.y; w[2] = (W)a.z; w[3] = (W)a.w;
    } else {
      const longlong2 a = *(const longlong2 *)(ptr + i), b = *(const longlong2 *)(ptr + i + 2);
      w[0] = (W)a.x; w[1] = (W)a.y; w[2] = (W)b.x; w[3] = (W)b.y;
    }
    w[4] = ptr[i + 4];
  } else {
#pragma unroll
    for (int k = 0; k <= DS_ITEMS; k++) w[k] = ptr[i + k < n ? i + k : n];
  }
#pragma unroll
  for (int k = 0; k < DS_ITEMS; k++) d[k] = (long long)w[k + 1] - (long long)w[k];
}

__device__ __forceinline__ void add128(unsigned long long &lo, unsigned long long &hi, unsigned long long alo,
                                       unsigned long long ahi) {
  const unsigned long long s = lo + alo;
  hi += ahi + (s < lo ? 1ull : 0ull);
  lo = s;
}

// min, max, zeros and the sum of squares per workgroup (integers: any order gives the same result), the sum of
// logarithms per tile
template <typename W>
__global__ __launch_bounds__(DS_THREADS) void k_ds_stats(const W *__restrict__ ptr, int64_t n, int64_t tiles, bool vec_ok,
                                                         bool want_log, DsBlock *__restrict__ blk,
                                                         double *__restrict__ tile_log) {
  __shared__ double s_log[DS_WAVES];
  __shared__ DsBlock s_blk[DS_WAVES];
  const int tid = threadIdx.x;
  long long mn = std::numeric_limits<long long>::max(), mx = std::numeric_limits<long long>::lowest();
  unsigned long long zeros = 0, sq_lo = 0, sq_hi = 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    double lg = 0.0;
#pragma unroll
    for (int s = 0; s < DS_STEPS; s++) {
      const int64_t i = tile * DS_TILE + (int64_t)(s * DS_THREADS + tid) * DS_ITEMS;
      if (i < n) {
        long long d[DS_ITEMS];
        load_degrees(ptr, i, n, vec_ok, d);
#pragma unroll
        for (int k = 0; k < DS_ITEMS; k++) {
          if (i + k < n) {
            mn = d[k] < mn ? d[k] : mn;
            mx = d[k] > mx ? d[k] : mx;
            zeros += d[k] == 0;
            const unsigned long long u = (unsigned long long)d[k];
            add128(sq_lo, sq_hi, u * u, __umul64hi(u, u));
            if (want_log && d[k] > 0) lg += log((double)d[k]);
          }
        }
      }
    }
    if (want_log) {  // (uniform)
      lg = sbx_wave_sum(lg);
      if (sbx_lane() == 0) s_log[sbx_wave_in_block()] = lg;
      __syncthreads();
      if (tid == 0) tile_log[tile] = (s_log[0] + s_log[1]) + (s_log[2] + s_log[3]);
      __syncthreads();
    }
  }
  mn = sbx_wave_min(mn);
  mx = sbx_wave_max(mx);
  zeros = sbx_wave_sum(zeros);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) add128(sq_lo, sq_hi, __shfl_xor(sq_lo, d, 64), __shfl_xor(sq_hi, d, 64));
  if (sbx_lane() == 0) s_blk[sbx_wave_in_block()] = DsBlock{mn, mx, zeros, sq_lo, sq_hi};
  __syncthreads();
  if (tid == 0) {
    DsBlock b = s_blk[0];
    for (int w = 1; w < DS_WAVES; w++) {
      b.mn = s_blk[w].mn < b.mn ? s_blk[w].mn : b.mn;
      b.mx = s_blk[w].mx > b.mx ? s_blk[w].mx : b.mx;
      b.zeros += s_blk[w].zeros;
      add128(b.sq_lo, b.sq_hi, s_blk[w].sq_lo, s_blk[w].sq_hi);
    }
    blk[blockIdx.x] = b;
  }
}

// single workgroup: the workgroups' integers and the tiles' logarithm sums, both in a fixed order, into the result;
// the select's state
template <typename W>
__global__ __launch_bounds__(DS_THREADS) void k_ds_finish(const W *__restrict__ ptr, int64_t n,
                                                          const DsBlock *__restrict__ blk, int nblk,
                                                          const double *__restrict__ tile_log, int64_t tiles,
                                                          unsigned flags, DsState *__restrict__ st) {
  __shared__ double s_log[DS_WAVES];
  __shared__ DsBlock s_blk[DS_WAVES];
  const int tid = threadIdx.x;
  long long mn = std::numeric_limits<long long>::max(), mx = std::numeric_limits<long long>::lowest();
  unsigned long long zeros = 0, sq_lo = 0, sq_hi = 0;
  for (int i = tid; i < nblk; i += DS_THREADS) {
    const DsBlock b = blk[i];
    mn = b.mn < mn ? b.mn : mn;
    mx = b.mx > mx ? b.mx : mx;
    zeros += b.zeros;
    add128(sq_lo, sq_hi, b.sq_lo, b.sq_hi);
  }
  double lg = 0.0;
  if (flags & SBXSTAT_LOG)
    for (int64_t t = tid; t < tiles; t += DS_THREADS) lg += tile_log[t];
  mn = sbx_wave_min(mn);
  mx = sbx_wave_max(mx);
  zeros = sbx_wave_sum(zeros);
  lg = sbx_wave_sum(lg);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) add128(sq_lo, sq_hi, __shfl_xor(sq_lo, d, 64), __shfl_xor(sq_hi, d, 64));
  if (sbx_lane() == 0) {
    s_blk[sbx_wave_in_block()] = DsBlock{mn, mx, zeros, sq_lo, sq_hi};
    s_log[sbx_wave_in_block()] = lg;
  }
  __syncthreads();
  if (tid == 0) {
    DsBlock b = s_blk[0];
    for (int w = 1; w < DS_WAVES; w++) {
      b.mn = s_blk[w].mn < b.mn ? s_blk[w].mn : b.mn;
      b.mx = s_blk[w].mx > b.mx ? s_blk[w].mx : b.mx;
      b.zeros += s_blk[w].zeros;
      add128(b.sq_lo, b.sq_hi, s_blk[w].sq_lo, s_blk[w].sq_hi);
    }
    const bool median = (flags & SBXSTAT_MEDIAN) != 0;
    st->out.count = n;
    st->out.sum = (long long)ptr[n] - (long long)ptr[0];
    st->out.min = b.mn;
    st->out.max = b.mx;
    st->out.zeros = (int64_t)b.zeros;
    st->out.sumsq_lo = b.sq_lo;
    st->out.sumsq_hi = b.sq_hi;
    st->out.median_lo = median ? 0 : -1;
    st->out.median_hi = median ? 0 : -1;
    st->out.sum_log = (s_log[0] + s_log[1]) + (s_log[2] + s_log[3]);
    st->rank[0] = (n - 1) / 2;
    st->rank[1] = n / 2;
    int digits = 0;
    for (unsigned long long v = b.mx > 0 ? (unsigned long long)b.mx : 0; v; v >>= DS_DIGIT) digits++;
    st->digits = digits;
    st->split = 0;
  }
}

// one more in bin `bin` of an LDS histogram for every lane with `want`; all 64 lanes call it.  On a power-law matrix
// nearly every lane holds the bin of degree 1 or 2 and the LDS serialises adds to one word, so for SBXSTAT_FOLD
// rounds the wave takes the bin of its first waiting lane and adds the number of lanes that share it in one go.
__device__ __forceinline__ void hist_add(unsigned *hist, unsigned bin, bool want) {
#if SBXSTAT_FOLD > 0
  for (int r = 0; r < SBXSTAT_FOLD; r++) {
    const uint64_t m = __ballot(want);
    if (!m) return;
    const int leader = __builtin_ctzll(m);
    const unsigned lb = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
    const bool mine = want && bin == lb;
    const uint64_t same = __ballot(mine);
    if (sbx_lane() == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
    if (mine) want = false;
  }
#endif
  if (want) atomicAdd(&hist[bin], 1u);
}

// the part of a key above digit p (0 above the last digit a 64-bit key has)
__device__ __forceinline__ unsigned long long key_above(unsigned long long key, int p) {
  const int sh = DS_DIGIT * (p + 1);
  return sh >= 64 ? 0ull : key >> sh;
}

// digit p of every degree that shares a rank's prefix, counted per rank once the prefixes differ
template <typename W>
__global__ __launch_bounds__(DS_THREADS) void k_ds_hist(const W *__restrict__ ptr, int64_t n, int64_t tiles, bool vec_ok,
                                                        int p, const DsState *__restrict__ st,
                                                        unsigned *__restrict__ hist) {
  __shared__ unsigned s_h[2 * DS_BINS];
  if (p >= st->digits) return;  // (every thread of the grid alike)
  const int tid = threadIdx.x;
  const bool split = st->split != 0;
  const unsigned long long pre0 = (unsigned long long)st->out.median_lo, pre1 = (unsigned long long)st->out.median_hi;
  for (int b = tid; b < (split ? 2 : 1) * DS_BINS; b += DS_THREADS) s_h[b] = 0;
  __syncthreads();
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int s = 0; s < DS_STEPS; s++) {
      const int64_t i = tile * DS_TILE + (int64_t)(s * DS_THREADS + tid) * DS_ITEMS;
      long long d[DS_ITEMS] = {0, 0, 0, 0};
      if (i < n) load_degrees(ptr, i, n, vec_ok, d);
#pragma unroll
      for (int k = 0; k < DS_ITEMS; k++) {  // (no lane leaves before hist_add: it votes)
        const unsigned long long key = (unsigned long long)d[k], above = key_above(key, p);
        const unsigned bin = (unsigned)(key >> (DS_DIGIT * p)) & (DS_BINS - 1);
        const bool valid = i + k < n;
        hist_add(s_h, bin, valid && above == pre0);
        if (split) hist_add(s_h + DS_BINS, bin, valid && above == pre1);
      }
    }
  }
  __syncthreads();
  for (int b = tid; b < (split ? 2 : 1) * DS_BINS; b += DS_THREADS)
    if (s_h[b]) atomicAdd(&hist[b], s_h[b]);
}

// single workgroup: the bin that holds each rank becomes the next digit of its prefix; the histograms are zeroed for
// the next digit
__global__ __launch_bounds__(DS_THREADS) void k_ds_pick(int p, DsState *__restrict__ st, unsigned *__restrict__ hist) {
  constexpr int PER = DS_BINS / DS_THREADS;
  __shared__ unsigned s_scan[DS_WAVES + 1];
  __shared__ unsigned s_bin[2];
  __shared__ long long s_before[2];
  if (p >= st->digits) return;
  const int tid = threadIdx.x;
  const bool split = st->split != 0;
  const long long rank[2] = {st->rank[0], st->rank[1]};
  if (tid < 2) {
    s_bin[tid] = 0;
    s_before[tid] = 0;
  }
  __syncthreads();
  for (int k = 0; k < 2; k++) {
    const unsigned *src = hist + (split && k == 1 ? DS_BINS : 0);
    unsigned c[PER], local = 0, total;
#pragma unroll
    for (int j = 0; j < PER; j++) {
      c[j] = src[tid * PER + j];
      local += c[j];
    }
    unsigned before = sbx_block_exclusive_sum<unsigned, DS_THREADS>(local, s_scan, &total);
    if (rank[k] >= (long long)before && rank[k] < (long long)before + (long long)local) {  // one thread at most
#pragma unroll
      for (int j = 0; j < PER; j++) {
        if (rank[k] >= (long long)before && rank[k] < (long long)before + (long long)c[j]) {
          s_bin[k] = (unsigned)(tid * PER + j);
          s_before[k] = (long long)before;
        }
        before += c[j];
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    st->out.median_lo = (int64_t)(((unsigned long long)st->out.median_lo << DS_DIGIT) | s_bin[0]);
    st->out.median_hi = (int64_t)(((unsigned long long)st->out.median_hi << DS_DIGIT) | s_bin[1]);
    st->rank[0] = rank[0] - s_before[0];
    st->rank[1] = rank[1] - s_before[1];
    if (s_bin[0] != s_bin[1]) st->split = 1;
  }
  for (int b = tid; b < 2 * DS_BINS; b += DS_THREADS) hist[b] = 0;
}

template <typename W>
int degree_stats_typed(sbx_handle_t h, int64_t n, const void *ptr, unsigned flags, sbxstat_degrees *out_host) {
  SBX_TRY(sbx_arena_begin(h));
  const int64_t tiles = (n + DS_TILE - 1) / DS_TILE;
  const unsigned grid = sbx_grid_for(tiles, 1, SBXSTAT_MAX_GRID);  // (the sum of logarithms does not depend on it)
  const bool vec_ok = ((uintptr_t)ptr & 15) == 0;
  const bool median = (flags & SBXSTAT_MEDIAN) != 0;
  DsBlock *blk = nullptr;
  double *tile_log = nullptr;
  DsState *st = nullptr;
  unsigned *hist = nullptr;
  SBX_TRY(sbx_salloc(h, 1, &st));
  SBX_TRY(sbx_salloc(h, grid, &blk));
  SBX_TRY(sbx_salloc(h, (size_t)tiles, &tile_log));
  if (median) {
    SBX_TRY(sbx_salloc(h, 2 * DS_BINS, &hist));
    SBX_HIP(h, hipMemsetAsync(hist, 0, 2 * DS_BINS * sizeof(unsigned), h->stream));
  }
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_ds_stats<W>, dim3(grid), dim3(DS_THREADS), (const W *)ptr, n, tiles, vec_ok,
              (flags & SBXSTAT_LOG) != 0, blk, tile_log);
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_ds_finish<W>, dim3(1), dim3(DS_THREADS), (const W *)ptr, n, (const DsBlock *)blk, (int)grid,
              (const double *)tile_log, tiles, flags, st);
  if (median) {
    // every digit the word type holds, most significant first: the pairs above the largest degree's top digit return
    // at once (k_ds_finish left the number of digits in the state)
    const int digits = (8 * (int)sizeof(W) - 1 + DS_DIGIT - 1) / DS_DIGIT;
    for (int p = digits - 1; p >= 0; p--) {
      SBX_KLAUNCH(h, SBX_K_FEATURE, k_ds_hist<W>, dim3(grid), dim3(DS_THREADS), (const W *)ptr, n, tiles, vec_ok, p,
                  (const DsState *)st, hist);
      SBX_KLAUNCH(h, SBX_K_FEATURE, k_ds_pick, dim3(1), dim3(DS_THREADS), p, st, hist);
    }
  }
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_FEATURE, (int64_t)sizeof(W) * (n + 1));
  SBX_TRY(sbx_readback(h, out_host, &st->out, sizeof(sbxstat_degrees)));
  if (out_host->min < 0) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbxstat_degree_stats: the offsets decrease somewhere");
  return SBX_OK;
}

// ---- OffDiagBlockNNZ ------------------------------------------------------------------------------------------------
constexpr int OD_THREADS = 256;
constexpr int OD_ITEMS = 8;
constexpr int OD_TILE = OD_THREADS * OD_ITEMS;

// pos[p] = row_ptr[rs_p] for 0 <= p <= blocks, kept inside [0, nnz]: block p is the positions [pos[p], pos[p + 1]).
// `blocks` is min(h, n): with h > n the rule gives one row to each of the first n blocks and none to the others.
template <typename O>
__global__ __launch_bounds__(OD_THREADS) void k_od_bounds(const O *__restrict__ rp, int64_t n, int64_t h, int64_t blocks,
                                                          int64_t nnz, int64_t *__restrict__ pos) {
  const int64_t p = (int64_t)blockIdx.x * OD_THREADS + threadIdx.x;
  if (p > blocks) return;
  const int64_t q = n / h, r = n % h;
  int64_t rs = p * q + (p < r ? p : r);
  rs = rs < n ? rs : n;
  int64_t v = (int64_t)rp[rs];
  v = v < 0 ? 0 : v;
  pos[p] = v < nnz ? v : nnz;
}

static_assert(OD_ITEMS == 8, "sbx_load_items8 fills a thread's columns");

struct OdRange {
  int64_t cs, ce;
  bool counted;  // the position lies in one of the blocks
};

// off_diag_block_nnz.cc:107-108; for p >= w both bounds are m (p * (m / w) + min(p, m % w) >= m there)
__device__ __forceinline__ OdRange od_range(int64_t p, int64_t blocks, int64_t m, int64_t w, int64_t cq, int64_t cr) {
  OdRange r;
  r.counted = p >= 0 && p < blocks;
  if (p >= w || p < 0) {
    r.cs = r.ce = m;
  } else {
    r.cs = p * cq + (p < cr ? p : cr);
    r.ce = (p + 1) * cq + (p + 1 < cr ? p + 1 : cr);
    r.cs = r.cs < m ? r.cs : m;
    r.ce = r.ce < m ? r.ce : m;
  }
  return r;
}

template <typename C>
__global__ __launch_bounds__(OD_THREADS) void k_od_count(const C *__restrict__ col, int64_t nnz, int64_t tiles,
                                                         const int64_t *__restrict__ pos, const int2 *__restrict__ span,
                                                         int64_t blocks, int64_t m, int64_t w, bool vec_ok,
                                                         unsigned long long *__restrict__ partial) {
  __shared__ unsigned long long s_sum[OD_THREADS / 64];
  const int tid = threadIdx.x;
  const int64_t cq = m / w, cr = m % w;
  const int64_t never = std::numeric_limits<int64_t>::max();
  unsigned long long cnt = 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t t0 = tile * OD_TILE;
    const int64_t t1 = (t0 + OD_TILE < nnz) ? t0 + OD_TILE : nnz;
    const int64_t base = t0 + (int64_t)tid * OD_ITEMS;
    if (base >= t1) continue;
    C c[OD_ITEMS];
    sbx_load_items8(col, base, t1, vec_ok, c);
    const int2 sp = span[tile];
    // the block of this thread's first entry: searched among the tile's blocks only (none to search in most tiles)
    int64_t lo = sp.x, hi = sp.y;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;  // (> lo >= -1)
      if (pos[mid] <= base) lo = mid; else hi = mid - 1;
    }
    int64_t p = lo;
    int64_t next = p < sp.y ? pos[p + 1] : never;  // where block p ends
    OdRange r = od_range(p, blocks, m, w, cq, cr);
#pragma unroll
    for (int k = 0; k < OD_ITEMS; k++) {
      const int64_t x = base + k;
      if (x < t1) {
        while (x >= next) {  // (empty blocks are stepped over)
          p++;
          next = p < sp.y ? pos[p + 1] : never;
          r = od_range(p, blocks, m, w, cq, cr);
        }
        const int64_t cc = (int64_t)c[k];
        cnt += r.counted && (cc < r.cs || cc >= r.ce);
      }
    }
  }
  cnt = sbx_wave_sum(cnt);
  if (sbx_lane() == 0) s_sum[sbx_wave_in_block()] = cnt;
  __syncthreads();
  if (tid == 0) {
    for (int w2 = 1; w2 < OD_THREADS / 64; w2++) cnt += s_sum[w2];
    partial[blockIdx.x] = cnt;
  }
}

__global__ __launch_bounds__(OD_THREADS) void k_od_finish(const unsigned long long *__restrict__ partial, int count,
                                                          unsigned long long *__restrict__ out) {
  __shared__ unsigned long long s_sum[OD_THREADS / 64];
  unsigned long long sum = 0;
  for (int i = threadIdx.x; i < count; i += OD_THREADS) sum += partial[i];
  sum = sbx_wave_sum(sum);
  if (sbx_lane() == 0) s_sum[sbx_wave_in_block()] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < OD_THREADS / 64; w++) sum += s_sum[w];
    *out = sum;
  }
}

template <typename O, typename C>
int off_diag_typed(sbx_handle_t h, int64_t n, int64_t m, int64_t nnz, const void *row_ptr, const void *col, int64_t bh,
                   int64_t bw, int64_t *count_host) {
  SBX_TRY(sbx_arena_begin(h));
  if (bh <= 0 || n == 0 || nnz == 0) return SBX_OK;
  const int64_t blocks = bh < n ? bh : n;
  const int64_t tiles = (nnz + OD_TILE - 1) / OD_TILE;
  const unsigned grid = sbx_grid_for(tiles, 1, SBXSTAT_OD_GRID);
  int64_t *pos = nullptr;
  int2 *span = nullptr;
  unsigned long long *partial = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)blocks + 1, &pos));
  SBX_TRY(sbx_salloc(h, (size_t)tiles, &span));
  SBX_TRY(sbx_salloc(h, (size_t)grid + 1, &partial));
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_od_bounds<O>, dim3((unsigned)((blocks + 1 + OD_THREADS - 1) / OD_THREADS)), dim3(OD_THREADS),
              (const O *)row_ptr, n, bh, blocks, nnz, pos);
  // the block of every tile's first and last entry: -1 before pos[0], `blocks` from pos[blocks] on
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_tile_spans<int64_t, OD_TILE, OD_THREADS>),
              dim3((unsigned)((tiles + OD_THREADS - 1) / OD_THREADS)), dim3(OD_THREADS), (const int64_t *)pos, blocks, nnz, tiles,
              span);
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_od_count<C>, dim3(grid), dim3(OD_THREADS), (const C *)col, nnz, tiles, (const int64_t *)pos,
              (const int2 *)span, blocks, m, bw, ((uintptr_t)col & 15) == 0, partial);
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_od_finish, dim3(1), dim3(OD_THREADS), (const unsigned long long *)partial, (int)grid,
              partial + grid);
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_FEATURE, (int64_t)sizeof(C) * nnz + (int64_t)sizeof(O) * (blocks + 1));
  unsigned long long total = 0;
  SBX_TRY(sbx_readback(h, &total, partial + grid, sizeof(total)));
  *count_host = (int64_t)total;
  return SBX_OK;
}

}  // namespace

#define SBXSTAT_REQUIRE(h, cond, msg)                                   \
  do {                                                                  \
    if (!(cond)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: %s", __func__, msg); \
  } while (0)

extern "C" int sbxstat_degree_stats(sbx_handle_t h, sbx_index_type it, int64_t n, const void *ptr, unsigned flags,
                                    sbxstat_degrees *out_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBXSTAT_REQUIRE(h, ptr && out_host, "bad argument");
  SBXSTAT_REQUIRE(h, n >= 1, "an offset array of no degrees has no statistics");
  SBXSTAT_REQUIRE(h, n < ((int64_t)1 << 31), "dimension exceeds what the call takes");
  SBXSTAT_REQUIRE(h, (flags & ~(SBXSTAT_MEDIAN | SBXSTAT_LOG)) == 0, "unknown flag");
  SBXSTAT_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  return it == SBX_I32 ? degree_stats_typed<int32_t>(h, n, ptr, flags, out_host)  // (SBX_I32_N64: 64-bit offsets, no id array)
                       : degree_stats_typed<int64_t>(h, n, ptr, flags, out_host);
}

extern "C" int sbxstat_csr_off_diag_block_nnz(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t m, int64_t nnz,
                                              const void *row_ptr, const void *col, int64_t block_rows,
                                              int64_t block_cols, int64_t *count_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBXSTAT_REQUIRE(h, n >= 0 && m >= 0 && nnz >= 0 && row_ptr && count_host && (nnz == 0 || col), "bad argument");
  SBXSTAT_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  SBXSTAT_REQUIRE(h, n < ((int64_t)1 << 31) - 1 && nnz / OD_TILE < ((int64_t)1 << 31), "dimension exceeds what the call takes");
  *count_host = 0;
  if (block_rows <= 0) return SBX_OK;  // off_diag_block_nnz.cc:104: no block, nothing counted
  SBXSTAT_REQUIRE(h, block_cols > 0, "block_cols must be positive (the reference divides by it)");
  if (it == SBX_I32) return off_diag_typed<int32_t, int32_t>(h, n, m, nnz, row_ptr, col, block_rows, block_cols, count_host);
  if (it == SBX_I64) return off_diag_typed<int64_t, int64_t>(h, n, m, nnz, row_ptr, col, block_rows, block_cols, count_host);
  return off_diag_typed<int64_t, int32_t>(h, n, m, nnz, row_ptr, col, block_rows, block_cols, count_host);
}
