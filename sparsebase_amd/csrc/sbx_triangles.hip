// sbx_triangles.hip — feature::TriangleCount on the device (reference: feature/triangle_count.cc:142-223), in two modes:
// the reference's value (the default) and the exact triangle / directed 3-cycle count (SBX_TC_EXACT).  The rules are in
// include/sbx.h; every id inside is 32-bit (n < 2^31) and every list a run of one sorted array of 64-bit keys
// (row << 32 | value), sorted by the library's radix sort.
//
// Reference mode (the closed form of the reference's marker loops):
//   1. first    first[w] by an atomicMin per nonzero (undirected: rows >= 1 holding w; directed: columns >= 1 of row w)
//   2. keys     one key per nonzero (v, w) of row v: v << 32 | first[w] (undirected: w > v only); directed, a second
//               array of v << 32 | max(first[w], w).  Entries without a key take the sentinel n << 32.
//   3. sort     radix sort of each array, then off[v] = the first key of row v (a search per row)
//   4. count    per nonzero (node, v) with node < v: the keys of row v with value <= node (one search in the row),
//               directed minus the same count in the second array; 64-bit sum by wave reductions
// Exact mode:
//   1. emit     undirected: both directions of every entry off the diagonal; directed: the arc and its reverse into
//               a second array (the in-lists)
//   2. simple   sort, drop duplicates (scan + scatter), off[] per row: sorted adjacency lists of the simple graph
//   3. orient   undirected: keep u -> v when (deg u, u) < (deg v, v) (scan + scatter, sorted out-lists N+)
//   4. items    undirected: every oriented edge (u, v), lists N+(u), N+(v); directed: every arc a -> b with a < b,
//               lists out(b), in(a), both cut to values > a.  The shorter list is probed in the longer.
//   5. bins     by the probe length: TB_G8 / TB_G16 / TB_WAVE: 8 / 16 / 64 lanes per item, each lane searching
//               entries l, l + G, ... of the probe list; TB_BLOCK: a workgroup per item, the searched list staged in
//               LDS when it fits.  Every lane sums its hits; one 64-bit atomic per wave at the end.
// Scratch comes from the handle's arena; the only read-back is the count itself.
#include "sbx_device.h"
#include "sbx_internal.h"

namespace {

constexpr int TT = 256;    // threads per workgroup, every kernel
constexpr int TITEMS = 4;  // consecutive nonzeros per thread in the nonzero-parallel kernels
constexpr uint32_t TC_INF = 0xFFFFFFFFu;
constexpr int TB_G8 = 0, TB_G16 = 1, TB_WAVE = 2, TB_BLOCK = 3, TB_COUNT = 4;
constexpr uint32_t TB_MAX_G8 = 8, TB_MAX_G16 = 16, TB_MAX_WAVE = 128;  // probe-length upper bounds of the first three bins
constexpr int TB_LDS_BYTES = 64 * 1024;                               // searched list staged when it fits: two workgroups per CU
constexpr unsigned char TB_SKIP = 0xFF;

// counters (u64): [0] the count, [1, 5) items per bin, [5, 9) scatter cursors
constexpr int TC_SUM = 0, TC_CNT = 1, TC_CUR = 5, TC_WORDS = 9;

__device__ __forceinline__ uint32_t tc_hi(uint64_t k) { return (uint32_t)(k >> 32); }
__device__ __forceinline__ uint32_t tc_lo(uint64_t k) { return (uint32_t)k; }

// f(p, row of p) for every nonzero p, TITEMS consecutive ones per thread: two searches over all rows, then narrow
// ones.  No cross-lane operation may sit in f: the trip count differs between lanes.
template <typename N, typename F>
__device__ __forceinline__ void tc_nonzeros(const N *__restrict__ rp, int64_t n, int64_t nnz, F f) {
  const int64_t stride = (int64_t)gridDim.x * TT * TITEMS;
  for (int64_t p0 = ((int64_t)blockIdx.x * TT + threadIdx.x) * TITEMS; p0 < nnz; p0 += stride) {
    const int k = nnz - p0 < TITEMS ? (int)(nnz - p0) : TITEMS;
    int64_t r = sbx_row_of(rp, p0, 0, n - 1);
    const int64_t r_last = sbx_row_of(rp, p0 + k - 1, r, n - 1);
    f(p0, r);
#pragma unroll
    for (int j = 1; j < TITEMS; j++)
      if (j < k) {
        r = sbx_row_of(rp, p0 + j, r, r_last);
        f(p0 + j, r);
      }
  }
}

// first index in [lo, hi) of a sorted u32 list whose value is >= x
__device__ __forceinline__ uint32_t tc_lower(const uint32_t *__restrict__ a, uint32_t lo, uint32_t hi, uint32_t x) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// does the sorted list a[0 .. len) hold x
__device__ __forceinline__ bool tc_find(const uint32_t *a, uint32_t len, uint32_t x) {
  uint32_t lo = 0, hi = len;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo < len && a[lo] == x;
}

// keys in [lo, hi) (one row of a sorted key array) whose value is <= x
__device__ __forceinline__ uint32_t tc_count_le(const uint64_t *__restrict__ k, uint32_t lo, uint32_t hi, uint32_t x) {
  const uint32_t start = lo;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (tc_lo(k[mid]) <= x) lo = mid + 1; else hi = mid;
  }
  return lo - start;
}

__device__ __forceinline__ void tc_add_sum(unsigned long long *sum, unsigned long long acc) {
  acc = sbx_wave_sum(acc);
  if (sbx_lane() == 0 && acc) atomicAdd(sum, acc);
}

// ---- reference mode -------------------------------------------------------------------------------------------------

// first[] (pre-filled with TC_INF).  A column outside [0, n) neither marks nor is marked.
template <typename I, typename N, bool DIRECTED>
__global__ __launch_bounds__(TT) void k_tc_first(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                 int64_t nnz, uint32_t *__restrict__ first) {
  tc_nonzeros(rp, n, nnz, [&](int64_t p, int64_t u) {
    const int64_t w = (int64_t)col[p];
    if (w < 0 || w >= n) return;
    const int64_t at = DIRECTED ? u : w, val = DIRECTED ? w : u;
    // (a plain look first: once a small value is in, the atomics of the rows after it are skipped)
    if (val >= 1 && (uint32_t)val < __atomic_load_n(&first[at], __ATOMIC_RELAXED)) atomicMin(&first[at], (uint32_t)val);
  });
}

template <typename I, typename N, bool DIRECTED>
__global__ __launch_bounds__(TT) void k_tc_ref_keys(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                    int64_t nnz, const uint32_t *__restrict__ first,
                                                    uint64_t *__restrict__ ka, uint64_t *__restrict__ kb) {
  const uint64_t sentinel = (uint64_t)n << 32;
  tc_nonzeros(rp, n, nnz, [&](int64_t p, int64_t v) {
    const int64_t w = (int64_t)col[p];
    uint64_t a = sentinel, b = sentinel;
    const uint32_t f = (w >= 0 && w < n) ? first[w] : TC_INF;
    if (f != TC_INF) {
      const uint64_t row = (uint64_t)v << 32;
      if (DIRECTED) {
        a = row | f;
        b = row | (f > (uint32_t)w ? f : (uint32_t)w);
      } else if (w > v) {
        a = row | f;
      }
    }
    ka[p] = a;
    if (DIRECTED) kb[p] = b;
  });
}

// off[r] = first index of a sorted key array (cnt keys, cnt from the device when cnt_dev is set) with key >= r << 32,
// r in [0, n]
__global__ __launch_bounds__(TT) void k_tc_offsets(const uint64_t *__restrict__ keys, int64_t cnt_host,
                                                   const uint32_t *__restrict__ cnt_dev, int64_t n,
                                                   uint32_t *__restrict__ off) {
  const uint32_t cnt = cnt_dev ? *cnt_dev : (uint32_t)cnt_host;
  for (int64_t r = (int64_t)blockIdx.x * TT + threadIdx.x; r <= n; r += (int64_t)gridDim.x * TT) {
    const uint64_t x = (uint64_t)r << 32;
    uint32_t lo = 0, hi = cnt;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < x) lo = mid + 1; else hi = mid;
    }
    off[r] = lo;
  }
}

template <typename I, typename N, bool DIRECTED>
__global__ __launch_bounds__(TT) void k_tc_ref_count(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                     int64_t nnz, const uint64_t *__restrict__ ka,
                                                     const uint32_t *__restrict__ offa, const uint64_t *__restrict__ kb,
                                                     const uint32_t *__restrict__ offb,
                                                     unsigned long long *__restrict__ sum) {
  unsigned long long acc = 0;
  tc_nonzeros(rp, n, nnz, [&](int64_t p, int64_t node) {
    const int64_t v = (int64_t)col[p];
    if (v <= node || v >= n) return;
    acc += tc_count_le(ka, offa[v], offa[v + 1], (uint32_t)node);
    if (DIRECTED) acc -= tc_count_le(kb, offb[v], offb[v + 1], (uint32_t)node);  // (never more than the first count)
  });
  tc_add_sum(sum, acc);
}

// ---- exact mode: the simple graph -----------------------------------------------------------------------------------

template <typename I, typename N, bool DIRECTED>
__global__ __launch_bounds__(TT) void k_tc_emit(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                int64_t nnz, uint64_t *__restrict__ ka, uint64_t *__restrict__ kb) {
  const uint64_t sentinel = (uint64_t)n << 32;
  tc_nonzeros(rp, n, nnz, [&](int64_t p, int64_t a) {
    const int64_t b = (int64_t)col[p];
    const bool ok = b >= 0 && b < n && b != a;
    const uint64_t fwd = ok ? (uint64_t)a << 32 | (uint64_t)b : sentinel;
    const uint64_t rev = ok ? (uint64_t)b << 32 | (uint64_t)a : sentinel;
    if (DIRECTED) {
      ka[p] = fwd;
      kb[p] = rev;
    } else {
      ka[2 * p] = fwd;
      ka[2 * p + 1] = rev;
    }
  });
}

// flag[i] = keys[i] is the first of its run and not the sentinel (sorted keys, cnt of them)
__global__ __launch_bounds__(TT) void k_tc_unique_flag(const uint64_t *__restrict__ keys, int64_t cnt,
                                                       uint64_t sentinel, uint32_t *__restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * TT) {
    const uint64_t k = keys[i];
    flag[i] = k < sentinel && (i == 0 || keys[i - 1] != k);
  }
}

__global__ __launch_bounds__(TT) void k_tc_unique_scatter(const uint64_t *__restrict__ keys, int64_t cnt,
                                                          uint64_t sentinel, const uint32_t *__restrict__ pos,
                                                          uint64_t *__restrict__ out, uint32_t *__restrict__ adj) {
  for (int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * TT) {
    const uint64_t k = keys[i];
    if (k < sentinel && (i == 0 || keys[i - 1] != k)) {
      out[pos[i]] = k;
      adj[pos[i]] = tc_lo(k);
    }
  }
}

// u -> v kept when (deg u, u) < (deg v, v); entries [m, cap) flagged 0 (m from the device)
__device__ __forceinline__ bool tc_keep(uint64_t k, const uint32_t *__restrict__ off) {
  const uint32_t u = tc_hi(k), v = tc_lo(k);
  const uint32_t du = off[u + 1] - off[u], dv = off[v + 1] - off[v];
  return du < dv || (du == dv && u < v);
}

__global__ __launch_bounds__(TT) void k_tc_orient_flag(const uint64_t *__restrict__ keys, int64_t cap,
                                                       const uint32_t *__restrict__ m_dev,
                                                       const uint32_t *__restrict__ off, uint32_t *__restrict__ flag) {
  const uint32_t m = *m_dev;
  for (int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x; i < cap; i += (int64_t)gridDim.x * TT)
    flag[i] = i < m && tc_keep(keys[i], off);
}

__global__ __launch_bounds__(TT) void k_tc_orient_scatter(const uint64_t *__restrict__ keys,
                                                          const uint32_t *__restrict__ m_dev,
                                                          const uint32_t *__restrict__ off,
                                                          const uint32_t *__restrict__ pos, uint64_t *__restrict__ out,
                                                          uint32_t *__restrict__ adj) {
  const uint32_t m = *m_dev;
  for (int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x; i < m; i += (int64_t)gridDim.x * TT) {
    const uint64_t k = keys[i];
    if (tc_keep(k, off)) {
      out[pos[i]] = k;
      adj[pos[i]] = tc_lo(k);
    }
  }
}

// ---- exact mode: intersections --------------------------------------------------------------------------------------

// the adjacency lists of an item: undirected, X = N+(u), Y = N+(v) (both from x_off / x_adj); directed (a -> b,
// a < b), X = out(b), Y = in(a) (from y_off / y_adj), both cut to the values > a.  X is the shorter one.
struct tc_lists {
  const uint32_t *x;
  uint32_t xl;
  const uint32_t *y;
  uint32_t yl;
};

template <bool DIRECTED>
__device__ __forceinline__ tc_lists tc_item(uint64_t k, const uint32_t *__restrict__ x_off,
                                            const uint32_t *__restrict__ x_adj, const uint32_t *__restrict__ y_off,
                                            const uint32_t *__restrict__ y_adj) {
  const uint32_t a = tc_hi(k), b = tc_lo(k);
  tc_lists L;
  if (DIRECTED) {
    if (a > b) return tc_lists{x_adj, 0, y_adj, 0};
    const uint32_t xe = x_off[b + 1], ye = y_off[a + 1];
    const uint32_t xs = tc_lower(x_adj, x_off[b], xe, a + 1), ys = tc_lower(y_adj, y_off[a], ye, a + 1);
    L = tc_lists{x_adj + xs, xe - xs, y_adj + ys, ye - ys};
  } else {
    const uint32_t xs = x_off[a], ys = x_off[b];
    L = tc_lists{x_adj + xs, x_off[a + 1] - xs, x_adj + ys, x_off[b + 1] - ys};
  }
  if (L.xl > L.yl) L = tc_lists{L.y, L.yl, L.x, L.xl};
  return L;
}

__device__ __forceinline__ int tc_bin(uint32_t len) {
  return len == 0 ? -1 : len <= TB_MAX_G8 ? TB_G8 : len <= TB_MAX_G16 ? TB_G16 : len <= TB_MAX_WAVE ? TB_WAVE : TB_BLOCK;
}

// the bin of every item [0, m) (m from the device; items past it and items with nothing to probe: TB_SKIP), counts per
// bin.  Whole workgroups walk the range together: the per-bin wave sums sit in the loop.
template <bool DIRECTED>
__global__ __launch_bounds__(TT) void k_tc_mark(const uint64_t *__restrict__ items, const uint32_t *__restrict__ m_dev, const uint32_t *__restrict__ x_off,
                                                const uint32_t *__restrict__ x_adj, const uint32_t *__restrict__ y_off,
                                                const uint32_t *__restrict__ y_adj, unsigned char *__restrict__ code,
                                                unsigned long long *__restrict__ ctr) {
  const uint32_t m = *m_dev;
  for (int64_t base = (int64_t)blockIdx.x * TT; base < m; base += (int64_t)gridDim.x * TT) {
    const int64_t i = base + threadIdx.x;
    int bin = -1;
    if (i < m) {
      bin = tc_bin(tc_item<DIRECTED>(items[i], x_off, x_adj, y_off, y_adj).xl);
      code[i] = bin < 0 ? TB_SKIP : (unsigned char)bin;
    }
#pragma unroll
    for (int b = 0; b < TB_COUNT; b++) {
      const unsigned long long c = (unsigned long long)sbx_wave_sum((int)(bin == b));
      if (c && sbx_lane() == 0) atomicAdd(&ctr[TC_CNT + b], c);
    }
  }
}

// every binned item's index into its bin's segment [sum of the counts before it, ...)
__global__ __launch_bounds__(TT) void k_tc_scatter(const unsigned char *__restrict__ code,
                                                   const uint32_t *__restrict__ m_dev,
                                                   unsigned long long *__restrict__ ctr, uint32_t *__restrict__ idx) {
  unsigned long long base[TB_COUNT];
  base[0] = 0;
#pragma unroll
  for (int b = 1; b < TB_COUNT; b++) base[b] = base[b - 1] + ctr[TC_CNT + b - 1];
  const uint32_t m = *m_dev;
  for (int64_t blk = (int64_t)blockIdx.x * TT; blk < m; blk += (int64_t)gridDim.x * TT) {
    const int64_t i = blk + threadIdx.x;
    const unsigned char c = i < m ? code[i] : TB_SKIP;
#pragma unroll
    for (int b = 0; b < TB_COUNT; b++) {
      const bool want = c == b;
      const unsigned long long slot = sbx_wave_append64(&ctr[TC_CUR + b], want);
      if (want) idx[base[b] + slot] = (uint32_t)i;
    }
  }
}

// bins TB_G8 / TB_G16 / TB_WAVE: G lanes per item, lane l probes entries l, l + G, ... of X in Y
template <bool DIRECTED, int G>
__global__ __launch_bounds__(TT) void k_tc_group(const uint64_t *__restrict__ items, const uint32_t *__restrict__ idx,
                                                 const uint32_t *__restrict__ x_off, const uint32_t *__restrict__ x_adj,
                                                 const uint32_t *__restrict__ y_off, const uint32_t *__restrict__ y_adj,
                                                 unsigned long long *__restrict__ ctr, int bin) {
  unsigned long long lo = 0;
  for (int b = 0; b < bin; b++) lo += ctr[TC_CNT + b];
  const unsigned long long hi = lo + ctr[TC_CNT + bin];
  const int g = threadIdx.x % G;
  const unsigned long long groups = (unsigned long long)gridDim.x * (TT / G);
  unsigned long long acc = 0;
  for (unsigned long long e = lo + ((unsigned long long)blockIdx.x * TT + threadIdx.x) / G; e < hi; e += groups) {
    const tc_lists L = tc_item<DIRECTED>(items[idx[e]], x_off, x_adj, y_off, y_adj);
    for (uint32_t t = g; t < L.xl; t += G) acc += tc_find(L.y, L.yl, L.x[t]);
  }
  tc_add_sum(&ctr[TC_SUM], acc);
}

// bin TB_BLOCK: a workgroup per item, items by a static stride; Y in LDS when it fits, else searched where it lies.
// Every thread derives the same lists, so the branch and the barriers are uniform.
template <bool DIRECTED>
__global__ __launch_bounds__(TT) void k_tc_block(const uint64_t *__restrict__ items, const uint32_t *__restrict__ idx,
                                                 const uint32_t *__restrict__ x_off, const uint32_t *__restrict__ x_adj,
                                                 const uint32_t *__restrict__ y_off, const uint32_t *__restrict__ y_adj,
                                                 unsigned long long *__restrict__ ctr) {
  constexpr uint32_t CAP = TB_LDS_BYTES / sizeof(uint32_t);
  __shared__ uint32_t s_y[CAP];
  const unsigned long long lo = ctr[TC_CNT + 0] + ctr[TC_CNT + 1] + ctr[TC_CNT + 2];
  const unsigned long long hi = lo + ctr[TC_CNT + TB_BLOCK];
  unsigned long long acc = 0;
  for (unsigned long long e = lo + blockIdx.x; e < hi; e += gridDim.x) {
    const tc_lists L = tc_item<DIRECTED>(items[idx[e]], x_off, x_adj, y_off, y_adj);
    if (L.yl <= CAP) {
      for (uint32_t t = threadIdx.x; t < L.yl; t += TT) s_y[t] = L.y[t];
      __syncthreads();
      for (uint32_t t = threadIdx.x; t < L.xl; t += TT) acc += tc_find(s_y, L.yl, L.x[t]);
      __syncthreads();  // (s_y free for the next item)
    } else {
      for (uint32_t t = threadIdx.x; t < L.xl; t += TT) acc += tc_find(L.y, L.yl, L.x[t]);
    }
  }
  tc_add_sum(&ctr[TC_SUM], acc);
}

}  // namespace

static int tc_offsets(sbx_handle_t h, const uint64_t *keys, int64_t cnt_host, const uint32_t *cnt_dev, int64_t n,
                      uint32_t *off) {
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_tc_offsets, dim3(sbx_grid_for(n + 1, TT, (int64_t)h->num_cus * 32)), dim3(TT), keys,
              cnt_host, cnt_dev, n, off);
  SBX_LAUNCH_CHECK(h);
  return SBX_OK;
}

// sorted, duplicate-free keys of cnt sorted keys (sentinels at the end): out / adj / off of the simple graph, the
// count in *m_dev
static int tc_unique(sbx_handle_t h, int64_t n, const uint64_t *keys, int64_t cnt, uint32_t *flag, uint64_t *out,
                     uint32_t *adj, uint32_t *off, uint32_t *m_dev) {
  const uint64_t sentinel = (uint64_t)n << 32;
  const unsigned g = sbx_grid_for(cnt, TT, (int64_t)h->num_cus * 32);
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_tc_unique_flag, dim3(g), dim3(TT), keys, cnt, sentinel, flag);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_exclusive_scan_u32(h, flag, flag, cnt, m_dev));
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_tc_unique_scatter, dim3(g), dim3(TT), keys, cnt, sentinel, (const uint32_t *)flag, out,
              adj);
  SBX_LAUNCH_CHECK(h);
  return tc_offsets(h, out, 0, m_dev, n, off);
}

// steps 4-5 of exact mode over the items [0, *m_dev) (cap bounds *m_dev); adds into ctr[TC_SUM]
template <bool DIRECTED>
static int tc_intersect(sbx_handle_t h, const uint64_t *items, int64_t cap, const uint32_t *m_dev, const uint32_t *x_off,
                        const uint32_t *x_adj, const uint32_t *y_off, const uint32_t *y_adj, unsigned long long *ctr) {
  unsigned char *code = nullptr;
  uint32_t *idx = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)cap, &code));
  SBX_TRY(sbx_salloc(h, (size_t)cap, &idx));
  const unsigned g_items = sbx_grid_for(cap, TT, (int64_t)h->num_cus * 32);
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_tc_mark<DIRECTED>, dim3(g_items), dim3(TT), items, m_dev, x_off, x_adj, y_off,
              y_adj, code, ctr);
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_tc_scatter, dim3(g_items), dim3(TT), (const unsigned char *)code, m_dev, ctr, idx);
  // fixed grids over the bins (their sizes stay on the device): enough groups to fill every CU
  const unsigned g_bins = (unsigned)h->num_cus * 16;
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_tc_group<DIRECTED, 8>), dim3(g_bins), dim3(TT), items, (const uint32_t *)idx, x_off,
              x_adj, y_off, y_adj, ctr, TB_G8);
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_tc_group<DIRECTED, 16>), dim3(g_bins), dim3(TT), items, (const uint32_t *)idx, x_off,
              x_adj, y_off, y_adj, ctr, TB_G16);
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_tc_group<DIRECTED, 64>), dim3(g_bins), dim3(TT), items, (const uint32_t *)idx, x_off,
              x_adj, y_off, y_adj, ctr, TB_WAVE);
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_tc_block<DIRECTED>, dim3((unsigned)h->num_cus * 2), dim3(TT), items,
              (const uint32_t *)idx, x_off, x_adj, y_off, y_adj, ctr);
  SBX_LAUNCH_CHECK(h);
  return SBX_OK;
}

template <typename I, typename N, bool DIRECTED>
static int tc_reference(sbx_handle_t h, int64_t n, int64_t nnz, const N *rp, const I *col, unsigned long long *ctr) {
  const unsigned g_nz = sbx_grid_for((nnz + TITEMS - 1) / TITEMS, TT, (int64_t)h->num_cus * 64);
  // (the sorts' bit ranges: a key's low field holds a value < n, its high field a row <= n)
  const int lo_bits = sbx_bits_for((uint64_t)(n - 1)), hi_end = 32 + sbx_bits_for((uint64_t)n);
  uint32_t *first = nullptr, *offa = nullptr, *offb = nullptr;
  uint64_t *ka = nullptr, *kb = nullptr, *tmp = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)n, &first));
  SBX_TRY(sbx_salloc(h, (size_t)n + 1, &offa));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &ka));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &tmp));
  if (DIRECTED) {
    SBX_TRY(sbx_salloc(h, (size_t)n + 1, &offb));
    SBX_TRY(sbx_salloc(h, (size_t)nnz, &kb));
  }
  SBX_HIP(h, hipMemsetAsync(first, 0xFF, (size_t)n * sizeof(uint32_t), h->stream));
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_tc_first<I, N, DIRECTED>), dim3(g_nz), dim3(TT), rp, col, n, nnz, first);
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_tc_ref_keys<I, N, DIRECTED>), dim3(g_nz), dim3(TT), rp, col, n, nnz,
              (const uint32_t *)first, ka, kb);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_sort_keys(h, &ka, &tmp, nnz, 0, lo_bits, 32, hi_end));
  SBX_TRY(tc_offsets(h, ka, nnz, nullptr, n, offa));
  if (DIRECTED) {
    SBX_TRY(sbx_sort_keys(h, &kb, &tmp, nnz, 0, lo_bits, 32, hi_end));
    SBX_TRY(tc_offsets(h, kb, nnz, nullptr, n, offb));
  }
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_tc_ref_count<I, N, DIRECTED>), dim3(g_nz), dim3(TT), rp, col, n, nnz,
              (const uint64_t *)ka, (const uint32_t *)offa, (const uint64_t *)kb, (const uint32_t *)offb, ctr + TC_SUM);
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_FEATURE, (int64_t)(2 * sizeof(I) + (DIRECTED ? 32 : 16)) * nnz + (int64_t)sizeof(N) * (n + 1));
  return SBX_OK;
}

template <typename I, typename N>
static int tc_exact_undirected(sbx_handle_t h, int64_t n, int64_t nnz, const N *rp, const I *col,
                               unsigned long long *ctr) {
  const int64_t cap = 2 * nnz;  // < 2^32: nnz < 2^31
  const unsigned g_nz = sbx_grid_for((nnz + TITEMS - 1) / TITEMS, TT, (int64_t)h->num_cus * 64);
  // (the sorts' bit ranges: a key's low field holds a value < n, its high field a row <= n)
  const int lo_bits = sbx_bits_for((uint64_t)(n - 1)), hi_end = 32 + sbx_bits_for((uint64_t)n);
  uint64_t *ka = nullptr, *tmp = nullptr, *sym = nullptr;
  uint32_t *flag = nullptr, *adj = nullptr, *off = nullptr, *oadj = nullptr, *ooff = nullptr, *m_dev = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)cap, &ka));
  SBX_TRY(sbx_salloc(h, (size_t)cap, &tmp));
  SBX_TRY(sbx_salloc(h, (size_t)cap, &sym));
  SBX_TRY(sbx_salloc(h, (size_t)cap, &flag));
  SBX_TRY(sbx_salloc(h, (size_t)cap, &adj));
  SBX_TRY(sbx_salloc(h, (size_t)cap, &oadj));
  SBX_TRY(sbx_salloc(h, (size_t)n + 1, &off));
  SBX_TRY(sbx_salloc(h, (size_t)n + 1, &ooff));
  SBX_TRY(sbx_salloc(h, 2, &m_dev));
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_tc_emit<I, N, false>), dim3(g_nz), dim3(TT), rp, col, n, nnz, ka, (uint64_t *)nullptr);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_sort_keys(h, &ka, &tmp, cap, 0, lo_bits, 32, hi_end));
  SBX_TRY(tc_unique(h, n, ka, cap, flag, sym, adj, off, m_dev));
  // orientation: the oriented keys go to the sort's input buffer, free again
  const unsigned g = sbx_grid_for(cap, TT, (int64_t)h->num_cus * 32);
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_tc_orient_flag, dim3(g), dim3(TT), (const uint64_t *)sym, cap, (const uint32_t *)m_dev,
              (const uint32_t *)off, flag);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_exclusive_scan_u32(h, flag, flag, cap, m_dev + 1));
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_tc_orient_scatter, dim3(g), dim3(TT), (const uint64_t *)sym, (const uint32_t *)m_dev,
              (const uint32_t *)off, (const uint32_t *)flag, ka, oadj);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(tc_offsets(h, ka, 0, m_dev + 1, n, ooff));
  return tc_intersect<false>(h, ka, cap, m_dev + 1, ooff, oadj, ooff, oadj, ctr);
}

template <typename I, typename N>
static int tc_exact_directed(sbx_handle_t h, int64_t n, int64_t nnz, const N *rp, const I *col,
                             unsigned long long *ctr) {
  const unsigned g_nz = sbx_grid_for((nnz + TITEMS - 1) / TITEMS, TT, (int64_t)h->num_cus * 64);
  // (the sorts' bit ranges: a key's low field holds a value < n, its high field a row <= n)
  const int lo_bits = sbx_bits_for((uint64_t)(n - 1)), hi_end = 32 + sbx_bits_for((uint64_t)n);
  uint64_t *kout = nullptr, *kin = nullptr, *tmp = nullptr, *uout = nullptr, *uin = nullptr;
  uint32_t *flag = nullptr, *out_adj = nullptr, *in_adj = nullptr, *out_off = nullptr, *in_off = nullptr, *m_dev = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &kout));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &kin));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &tmp));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &uout));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &uin));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &flag));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &out_adj));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &in_adj));
  SBX_TRY(sbx_salloc(h, (size_t)n + 1, &out_off));
  SBX_TRY(sbx_salloc(h, (size_t)n + 1, &in_off));
  SBX_TRY(sbx_salloc(h, 2, &m_dev));
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_tc_emit<I, N, true>), dim3(g_nz), dim3(TT), rp, col, n, nnz, kout, kin);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_sort_keys(h, &kout, &tmp, nnz, 0, lo_bits, 32, hi_end));
  SBX_TRY(tc_unique(h, n, kout, nnz, flag, uout, out_adj, out_off, m_dev));
  SBX_TRY(sbx_sort_keys(h, &kin, &tmp, nnz, 0, lo_bits, 32, hi_end));
  SBX_TRY(tc_unique(h, n, kin, nnz, flag, uin, in_adj, in_off, m_dev + 1));
  return tc_intersect<true>(h, uout, nnz, m_dev, out_off, out_adj, in_off, in_adj, ctr);
}

template <typename I, typename N>
static int tc_typed(sbx_handle_t h, int64_t n, int64_t nnz, const void *row_ptr, const void *col_v, unsigned flags,
                    int64_t *count_host) {
  SBX_TRY(sbx_arena_begin(h));
  if (nnz == 0 || n < 3) return SBX_OK;  // three distinct vertices are needed in every mode
  const N *rp = (const N *)row_ptr;
  const I *col = (const I *)col_v;
  unsigned long long *ctr = nullptr;
  SBX_TRY(sbx_salloc(h, TC_WORDS, &ctr));
  SBX_HIP(h, hipMemsetAsync(ctr, 0, TC_WORDS * sizeof(unsigned long long), h->stream));
  const bool directed = flags & SBX_TC_DIRECTED;
  if (flags & SBX_TC_EXACT) {
    SBX_TRY(directed ? (tc_exact_directed<I, N>(h, n, nnz, rp, col, ctr))
                     : (tc_exact_undirected<I, N>(h, n, nnz, rp, col, ctr)));
  } else {
    SBX_TRY(directed ? (tc_reference<I, N, true>(h, n, nnz, rp, col, ctr))
                     : (tc_reference<I, N, false>(h, n, nnz, rp, col, ctr)));
  }
  unsigned long long total = 0;
  SBX_TRY(sbx_readback(h, &total, ctr + TC_SUM, sizeof(total)));
  *count_host = (int64_t)total;
  return SBX_OK;
}

extern "C" int sbx_csr_triangle_count(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t nnz, const void *row_ptr,
                                      const void *col, unsigned flags, int64_t *count_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, n >= 0 && nnz >= 0 && (n > 0 || nnz == 0) && count_host && (nnz == 0 || (row_ptr && col)),
              "bad argument");
  SBX_REQUIRE(h, (flags & ~(SBX_TC_DIRECTED | SBX_TC_EXACT)) == 0, "unknown flag");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  if (it != SBX_I64 && n >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: row count exceeds int32", __func__);
  if (it == SBX_I32 && nnz >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: nnz exceeds int32", __func__);
  *count_host = 0;
  if (n >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: n >= 2^31", __func__);
  if (nnz >= ((int64_t)1 << ((flags & SBX_TC_EXACT) ? 31 : 32)))
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: nnz >= 2^%d in this mode", __func__, (flags & SBX_TC_EXACT) ? 31 : 32);
  if (it == SBX_I32) return tc_typed<int32_t, int32_t>(h, n, nnz, row_ptr, col, flags, count_host);
  if (it == SBX_I32_N64) return tc_typed<int32_t, int64_t>(h, n, nnz, row_ptr, col, flags, count_host);
  return tc_typed<int64_t, int64_t>(h, n, nnz, row_ptr, col, flags, count_host);
}
