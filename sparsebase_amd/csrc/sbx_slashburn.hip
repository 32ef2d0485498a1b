// sbx_slashburn.hip — reorder::SlashburnReorder on the device (reference: reorder/slashburn_reorder.cc).  The rules the
// device reproduces are in include/sbx.h and DESIGN §4.13; every id, offset and position inside is 32-bit (n < 2^31,
// 2 nnz < 2^31).  The host drives one loop iteration per round; the device keeps the round's state.
//
//   S        the symmetrized adjacency of :333-376: the entries are transposed by the library's radix sort (keys
//            col << 32 | row); a kept transposed entry is one whose mirror is not stored (a binary search in the sorted
//            column segment of its row); count, scan, emit.  Kept entries are read from the back of their segment.
//   phase 0  components of S (union-find, roots = smallest ids), sorted by (size, root); all but the last placed
//   round    deg over E (a wave per row), hubs (default: radix select of the k-th largest degree tau, then the closed
//            form of the reference's size-k heap through one scan; greedy: ONE workgroup runs the k picks over the
//            vertices sorted by (degree desc, id asc), rescanning lazily), components of E minus the hubs, each
//            component's root entry by an atomicMin over the hub rows' scan positions, the GCC by one packed 64-bit
//            atomicMax, the other components sorted by (hub index?, size, root) with two stable radix sorts
//   place    one ordered BFS from all of the round's roots at once, level by level.  A child's key is (rank of its
//            parent in the level, adjacency index), taken with a 64-bit atomicMin; every level is sorted by key.
//            Narrow levels (<= SB_CAP vertices) run inside one workgroup, level after level, until a level grows wider;
//            wide ones take a grid kernel, a read-back and the radix sort.  The levels concatenated and sorted stably
//            by component index give each component's BFS order; the i-th vertex of that sequence goes to P - i.
// Scratch comes from the handle's arena.  Read-backs per call: the column check, the phase-0 component count, and per
// round the component count plus one per wide BFS level and one per run of narrow levels.
#include <cstddef>

#include "sbx_device.h"
#include "sbx_internal.h"

namespace {

constexpr int ST = 256;          // threads per workgroup of the grid kernels
constexpr int SB_WG = 1024;      // threads of the one-workgroup kernels (greedy picks, narrow BFS levels)
constexpr unsigned SB_CAP = 1024;  // widest level the one-workgroup BFS sorts in LDS
constexpr uint64_t SB_UNSEEN = ~0ull;
constexpr unsigned SB_NONE = 0xFFFFFFFFu;

// device state of a call (one struct in the arena, zeroed once)
struct SbDev {
  unsigned bad;        // a column outside [0, n)
  unsigned ncomp;      // components found by the last component pass
  unsigned long long gcc;  // packed GCC: phase 0 (size << 32 | root), rounds (size << 32 | ~root scan position)
  unsigned maxdeg;     // largest row of S
  unsigned noroot;     // a component of a round without a root entry (a broken invariant)
  // hub selection (default mode)
  unsigned prefix, pmask, krem, T, D, hub_cnt;
  unsigned hist[256];
  // BFS: the four words the host reads back after a BFS step
  unsigned f, seq_off, nxt_cnt, status;
};
constexpr unsigned SB_BFS_DONE = 1, SB_BFS_WIDE = 2;

__device__ __forceinline__ unsigned sb_ld8(const unsigned char *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sb_st8(unsigned char *p, unsigned char v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned sb_ld32(const unsigned *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long sb_ld64(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#define SB_GRID_LOOP(i, count) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)(count); i += (int64_t)gridDim.x * blockDim.x)

// ---- S ---------------------------------------------------------------------------------------------------------------

// transposed keys col << 32 | row; a column outside [0, n) raises dv->bad (its key is a harmless 0)
template <typename I, typename N>
__global__ __launch_bounds__(ST) void k_sb_tkeys(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                 int64_t nnz, uint64_t *__restrict__ tkey, SbDev *__restrict__ dv) {
  SB_GRID_LOOP(p, nnz) {
    const int64_t c = (int64_t)col[p];
    if (c < 0 || c >= n) {
      dv->bad = 1;
      tkey[p] = 0;
    } else {
      tkey[p] = (uint64_t)c << 32 | (uint64_t)sbx_row_of(rp, n, p);
    }
  }
}

// off[r] = the first position of the sorted keys with key >= r << 32, r in [0, n]
__global__ __launch_bounds__(ST) void k_sb_offsets(const uint64_t *__restrict__ keys, int64_t cnt, int64_t n,
                                                   uint32_t *__restrict__ off) {
  SB_GRID_LOOP(r, n + 1) {
    const uint64_t x = (uint64_t)r << 32;
    uint32_t lo = 0, hi = (uint32_t)cnt;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < x) lo = mid + 1; else hi = mid;
    }
    off[r] = lo;
  }
}

// keep[q] = 1 when the transposed entry (row c gets r) has no mirror: row c stores no column r, i.e. the sorted segment
// of column r holds no row c
__global__ __launch_bounds__(ST) void k_sb_keep(const uint64_t *__restrict__ tkey, int64_t nnz,
                                                const uint32_t *__restrict__ tptr, uint32_t *__restrict__ keep) {
  SB_GRID_LOOP(q, nnz) {
    const uint64_t k = tkey[q];
    const uint32_t c = (uint32_t)(k >> 32), r = (uint32_t)k;
    const uint64_t want = (uint64_t)r << 32 | c;
    uint32_t lo = tptr[r], hi = tptr[r + 1];
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (tkey[mid] < want) lo = mid + 1; else hi = mid;
    }
    keep[q] = (lo < tptr[r + 1] && tkey[lo] == want) ? 0u : 1u;
  }
}

template <typename N>
__global__ __launch_bounds__(ST) void k_sb_rowlen(const N *__restrict__ rp, int64_t n, const uint32_t *__restrict__ tptr,
                                                  const uint32_t *__restrict__ kscan, uint32_t *__restrict__ len) {
  SB_GRID_LOOP(i, n) {
    len[i] = (uint32_t)((int64_t)rp[i + 1] - (int64_t)rp[i]) + kscan[tptr[i + 1]] - kscan[tptr[i]];
  }
}

template <typename I, typename N>
__global__ __launch_bounds__(ST) void k_sb_emit_stored(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                       int64_t nnz, const uint32_t *__restrict__ srp,
                                                       uint32_t *__restrict__ scol) {
  SB_GRID_LOOP(p, nnz) {
    const int64_t r = sbx_row_of(rp, n, p);
    scol[srp[r] + (uint32_t)(p - (int64_t)rp[r])] = (uint32_t)col[p];
  }
}

// kept transposed entries of segment c follow row c's stored entries in descending row order: the segment read backwards
__global__ __launch_bounds__(ST) void k_sb_emit_kept(const uint64_t *__restrict__ tkey, int64_t nnz,
                                                     const uint32_t *__restrict__ tptr, const uint32_t *__restrict__ kscan,
                                                     const uint32_t *__restrict__ srp, uint32_t *__restrict__ scol) {
  SB_GRID_LOOP(q, nnz) {
    if (kscan[q + 1] == kscan[q]) continue;  // not kept
    const uint64_t k = tkey[q];
    const uint32_t c = (uint32_t)(k >> 32);
    const uint32_t front = kscan[q] - kscan[tptr[c]];
    scol[srp[c + 1] - 1 - front] = (uint32_t)k;
  }
}

__global__ __launch_bounds__(ST) void k_sb_maxdeg(const uint32_t *__restrict__ srp, int64_t n, SbDev *__restrict__ dv) {
  unsigned m = 0;
  SB_GRID_LOOP(i, n) {
    const unsigned d = srp[i + 1] - srp[i];
    m = d > m ? d : m;
  }
  m = sbx_wave_max(m);
  if (sbx_lane() == 0 && m) atomicMax(&dv->maxdeg, m);
}

// ---- components of S over the vertices with inE set ----------------------------------------------------------------

__device__ __forceinline__ uint32_t cc_find(uint32_t *parent, uint32_t v) {
  uint32_t curr = parent[v];
  if (curr != v) {
    uint32_t prev = v, next;
    while (curr > (next = parent[curr])) {  // parent[x] <= x always: the chain descends
      parent[prev] = next;                  // path halving
      prev = curr;
      curr = next;
    }
  }
  return curr;
}

__device__ __forceinline__ void cc_hook(uint32_t *parent, uint32_t a, uint32_t b) {
  uint32_t ra = cc_find(parent, a), rb = cc_find(parent, b);
  bool again;
  do {
    again = false;
    if (ra != rb) {
      if (ra < rb) {
        const uint32_t got = atomicCAS(&parent[rb], rb, ra);
        if (got != rb) { rb = got; again = true; }
      } else {
        const uint32_t got = atomicCAS(&parent[ra], ra, rb);
        if (got != ra) { ra = got; again = true; }
      }
    }
  } while (again);
}

__global__ __launch_bounds__(ST) void k_sb_cc_init(const unsigned char *__restrict__ inE, int64_t n,
                                                   uint32_t *__restrict__ parent, uint32_t *__restrict__ csize,
                                                   unsigned long long *__restrict__ rkey) {
  SB_GRID_LOOP(v, n) {
    if (!inE[v]) continue;
    parent[v] = (uint32_t)v;
    csize[v] = 0;
    rkey[v] = SB_UNSEEN;
  }
}

// a wave per vertex of E: hooks every entry towards a smaller eligible id (S is symmetric: each edge is seen twice)
__global__ __launch_bounds__(ST) void k_sb_cc_hook(const uint32_t *__restrict__ srp, const uint32_t *__restrict__ scol,
                                                   const unsigned char *__restrict__ inE, int64_t n, uint32_t *parent) {
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t v = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; v < n; v += nwaves) {
    if (!inE[v]) continue;
    for (uint32_t e = srp[v] + sbx_lane(); e < srp[v + 1]; e += 64) {
      const uint32_t w = scol[e];
      if (w < (uint32_t)v && inE[w]) cc_hook(parent, (uint32_t)v, w);
    }
  }
}

// parent[v] = the component's root (its smallest id); sizes by atomics, equal roots combined inside the wave
__global__ __launch_bounds__(ST) void k_sb_cc_final(const unsigned char *__restrict__ inE, int64_t n, uint32_t *parent,
                                                    uint32_t *__restrict__ csize) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t vb = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - sbx_lane(); vb < n; vb += stride) {
    const int64_t v = vb + sbx_lane();
    uint32_t root = SB_NONE;
    if (v < n && inE[v]) {
      root = parent[v];
      while (root != parent[root]) root = parent[root];
    }
    uint64_t todo = __ballot(root != SB_NONE);
    while (todo) {
      const int leader = __builtin_ctzll(todo);
      const uint32_t lr = (uint32_t)__builtin_amdgcn_readlane((int)root, leader);
      const uint64_t same = __ballot(root == lr) & todo;
      if (sbx_lane() == leader) atomicAdd(&csize[lr], (uint32_t)__popcll(same));
      todo &= ~same;
    }
    if (root != SB_NONE) parent[v] = root;  // (path compression: a chain through v still ends at the root)
  }
}

// ---- hub selection -----------------------------------------------------------------------------------------------------

// deg[v] = entries of row v whose column is in E (self loops and duplicates count); a wave per row.  cur = deg (greedy).
__global__ __launch_bounds__(ST) void k_sb_degree(const uint32_t *__restrict__ srp, const uint32_t *__restrict__ scol,
                                                  const unsigned char *__restrict__ inE, int64_t n,
                                                  uint32_t *__restrict__ deg, int32_t *__restrict__ cur) {
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t v = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; v < n; v += nwaves) {
    if (!inE[v]) continue;
    unsigned d = 0;
    for (uint32_t e = srp[v] + sbx_lane(); e < srp[v + 1]; e += 64) d += inE[scol[e]] ? 1u : 0u;
    d = sbx_wave_sum(d);
    if (sbx_lane() == 0) {
      deg[v] = d;
      if (cur) cur[v] = (int32_t)d;
    }
  }
}

__global__ void k_sb_sel_init(int64_t k, SbDev *__restrict__ dv) {
  for (int i = threadIdx.x; i < 256; i += blockDim.x) dv->hist[i] = 0;
  if (threadIdx.x == 0) {
    dv->prefix = 0;
    dv->pmask = 0;
    dv->krem = (unsigned)k;
    dv->hub_cnt = 0;
  }
}

// one 8-bit digit of the k-th largest degree of E: histogram of the vertices that match the digits found so far
__global__ __launch_bounds__(ST) void k_sb_sel_hist(const unsigned char *__restrict__ inE, const uint32_t *__restrict__ deg,
                                                    int64_t n, int shift, SbDev *__restrict__ dv) {
  __shared__ unsigned s_hist[256];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned prefix = dv->prefix, pmask = dv->pmask;
  SB_GRID_LOOP(v, n) {
    if (!inE[v]) continue;
    const unsigned d = deg[v];
    if ((d & pmask) == prefix) atomicAdd(&s_hist[(d >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (s_hist[threadIdx.x]) atomicAdd(&dv->hist[threadIdx.x], s_hist[threadIdx.x]);
}

__global__ void k_sb_sel_pick(int shift, SbDev *__restrict__ dv) {
  if (threadIdx.x != 0) return;
  unsigned above = 0, b = 255;
  for (;; b--) {
    if (above + dv->hist[b] >= dv->krem || b == 0) break;
    above += dv->hist[b];
  }
  dv->prefix |= b << shift;
  dv->pmask |= 255u << shift;
  dv->krem -= above;
  for (int i = 0; i < 256; i++) dv->hist[i] = 0;
}

// flags of the closed form: hi word (deg >= tau), lo word (deg == tau), for the exclusive scan
__global__ __launch_bounds__(ST) void k_sb_sel_flags(const unsigned char *__restrict__ inE, const uint32_t *__restrict__ deg,
                                                     int64_t n, const SbDev *__restrict__ dv, int64_t *__restrict__ x) {
  const unsigned tau = dv->prefix;
  SB_GRID_LOOP(v, n) {
    const bool e = inE[v];
    const unsigned d = e ? deg[v] : 0;
    x[v] = (int64_t)((uint64_t)(e && d >= tau) << 32 | (uint64_t)(e && d == tau));
  }
}

// T = the k-th vertex (id order) with deg >= tau; D = the degree-tau vertices with id <= T
__global__ __launch_bounds__(ST) void k_sb_sel_T(const unsigned char *__restrict__ inE, const uint32_t *__restrict__ deg,
                                                 int64_t n, int64_t k, const int64_t *__restrict__ x,
                                                 SbDev *__restrict__ dv) {
  const unsigned tau = dv->prefix;
  SB_GRID_LOOP(v, n) {
    if (!inE[v] || deg[v] < tau) continue;
    const uint64_t xv = (uint64_t)x[v];
    if ((xv >> 32) == (uint64_t)(k - 1)) {
      dv->T = (unsigned)v;
      dv->D = (uint32_t)xv + (deg[v] == tau ? 1u : 0u);
    }
  }
}

// the hubs of the closed form: deg > tau, and the last c = krem degree-tau vertices with id <= T; keys deg << 32 | id
__global__ __launch_bounds__(ST) void k_sb_sel_mark(const unsigned char *__restrict__ inE, const uint32_t *__restrict__ deg,
                                                    int64_t n, int64_t k, const int64_t *__restrict__ x,
                                                    SbDev *__restrict__ dv, uint64_t *__restrict__ hkey) {
  const unsigned tau = dv->prefix, T = dv->T, lo_rank = dv->D - dv->krem;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t vb = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - sbx_lane(); vb < n; vb += stride) {
    const int64_t v = vb + sbx_lane();
    bool hub = false;
    unsigned d = 0;
    if (v < n && inE[v]) {
      d = deg[v];
      hub = d > tau || (d == tau && (unsigned)v <= T && (uint32_t)(uint64_t)x[v] >= lo_rank);
    }
    const unsigned slot = sbx_wave_append(&dv->hub_cnt, hub);
    if (hub && slot < (unsigned)k) hkey[slot] = (uint64_t)d << 32 | (uint64_t)v;  // (exactly k by the closed form)
  }
}

// greedy: sort keys (maxdeg - deg) << 32 | id for E, (maxdeg + 1) << 32 | id for the rest
__global__ __launch_bounds__(ST) void k_sb_greedy_keys(const unsigned char *__restrict__ inE,
                                                       const uint32_t *__restrict__ deg, int64_t n, unsigned maxdeg,
                                                       uint64_t *__restrict__ key) {
  SB_GRID_LOOP(v, n) {
    const uint64_t hi = inE[v] ? (uint64_t)(maxdeg - deg[v]) : (uint64_t)maxdeg + 1;
    key[v] = hi << 32 | (uint64_t)v;
  }
}

// greedy: ONE workgroup runs the k picks.  Pick j is the smallest id of maximal current degree among E minus the hubs
// picked so far; the list is sorted by (initial degree desc, id asc) and current <= initial, so a scan stops at the
// first chunk whose last initial degree is below the best current one.  After a pick, every entry (h, w) of the hub's
// row with w still eligible lowers cur[w] by one.  Current degrees are signed: a row that holds w more often than w's
// row holds h takes w below zero, as the reference's signed counters do.
__global__ __launch_bounds__(SB_WG) void k_sb_greedy(const uint32_t *__restrict__ srp, const uint32_t *__restrict__ scol,
                                                     unsigned char *inE, const uint64_t *__restrict__ list, int64_t nE,
                                                     unsigned maxdeg, int64_t k, int32_t *cur,
                                                     uint32_t *__restrict__ hub) {
  __shared__ unsigned long long s_best[SB_WG / 64];
  __shared__ unsigned long long s_pick;
  __shared__ int64_t s_start;
  if (threadIdx.x == 0) s_start = 0;
  __syncthreads();
  for (int64_t j = 0; j < k; j++) {
    unsigned long long best = 0;  // (cur ^ 2^31) << 32 | ~id (order-preserving for signed cur); 0 = none
    for (int64_t c0 = s_start; c0 < nE; c0 += SB_WG) {
      const int64_t i = c0 + threadIdx.x;
      if (i < nE) {
        const uint32_t v = (uint32_t)list[i];
        if (sb_ld8(&inE[v])) {
          const unsigned long long cand = (unsigned long long)(sb_ld32((const unsigned *)&cur[v]) ^ 0x80000000u) << 32 |
                                          (uint32_t)~v;
          best = cand > best ? cand : best;
        }
      }
      best = sbx_wave_max(best);
      if (sbx_lane() == 0) s_best[sbx_wave_in_block()] = best;
      __syncthreads();
      for (int w = 0; w < SB_WG / 64; w++) best = s_best[w] > best ? s_best[w] : best;
      __syncthreads();
      const int64_t last = (c0 + SB_WG < nE ? c0 + SB_WG : nE) - 1;
      const int64_t last_init = (int64_t)maxdeg - (int64_t)(list[last] >> 32);
      const int64_t best_cur = (int32_t)((uint32_t)(best >> 32) ^ 0x80000000u);
      if (best && last_init < best_cur) break;  // every later vertex has cur <= init < best's cur
    }
    if (!best) break;  // (no eligible vertex: |E| >= k rules it out; the host finds the missing positions)
    const uint32_t h = ~(uint32_t)best;
    if (threadIdx.x == 0) {
      hub[j] = h;
      sb_st8(&inE[h], 0);
      int64_t s = s_start;  // skip the picked prefix of the list
      while (s < nE && !sb_ld8(&inE[(uint32_t)list[s]])) s++;
      s_start = s;
    }
    __syncthreads();
    for (uint32_t e = srp[h] + threadIdx.x; e < srp[h + 1]; e += SB_WG) {
      const uint32_t w = scol[e];
      if (sb_ld8(&inE[w])) atomicSub(&cur[w], 1);
    }
    __syncthreads();
  }
}

// hubs in place order: pos[h_j] = base + j, out of E; hlen[k - 1 - j] = |row h_j| (the scan runs h_{k-1} ... h_0).
// Default mode: h_j = the (j+1)-th largest (deg, id) of the sorted keys.
__global__ __launch_bounds__(ST) void k_sb_hub_commit(const uint64_t *__restrict__ hkey_sorted, uint32_t *__restrict__ hub,
                                                      int64_t k, int64_t n, uint32_t base,
                                                      const uint32_t *__restrict__ srp, unsigned char *__restrict__ inE,
                                                      uint32_t *__restrict__ pos, uint32_t *__restrict__ hlen) {
  SB_GRID_LOOP(j, k) {
    uint32_t v = hkey_sorted ? (uint32_t)hkey_sorted[k - 1 - j] : hub[j];
    if (v >= (uint64_t)n) v = 0;  // (a broken invariant, harmless here: the host's position count fails the call)
    if (hkey_sorted) hub[j] = v;
    pos[v] = base + (uint32_t)j;
    inE[v] = 0;
    hlen[k - 1 - j] = srp[v + 1] - srp[v];
  }
}

// the root entry of every component of E': a workgroup per hub row, in scan order q = k - 1 - j
__global__ __launch_bounds__(ST) void k_sb_roots(const uint32_t *__restrict__ srp, const uint32_t *__restrict__ scol,
                                                 const unsigned char *__restrict__ inE, const uint32_t *__restrict__ hub,
                                                 const uint32_t *__restrict__ hoff, int64_t k,
                                                 const uint32_t *__restrict__ label, unsigned long long *rkey) {
  for (int64_t q = blockIdx.x; q < k; q += gridDim.x) {
    const uint32_t v = hub[k - 1 - q], s = srp[v], len = srp[v + 1] - s;
    for (uint32_t e = threadIdx.x; e < len; e += ST) {
      const uint32_t w = scol[s + e];
      if (inE[w]) atomicMin(&rkey[label[w]], (unsigned long long)(hoff[q] + e) << 32 | w);
    }
  }
}

// the components (their smallest-id labels) in any order, and the GCC by one packed atomicMax
__global__ __launch_bounds__(ST) void k_sb_comps(const unsigned char *__restrict__ inE, int64_t n,
                                                 const uint32_t *__restrict__ label, const uint32_t *__restrict__ csize,
                                                 const unsigned long long *__restrict__ rkey, int phase0,
                                                 uint32_t *__restrict__ list, SbDev *__restrict__ dv) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long g = 0;
  for (int64_t vb = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - sbx_lane(); vb < n; vb += stride) {
    const int64_t v = vb + sbx_lane();
    const bool is_root = v < n && inE[v] && label[v] == (uint32_t)v;
    const unsigned slot = sbx_wave_append(&dv->ncomp, is_root);
    if (!is_root) continue;
    list[slot] = (uint32_t)v;
    unsigned long long key;
    if (phase0) {
      key = (unsigned long long)csize[v] << 32 | (uint32_t)v;
    } else {
      const unsigned long long r = rkey[v];
      if (r == SB_UNSEEN) dv->noroot = 1;
      key = (unsigned long long)csize[v] << 32 | (uint32_t)~(uint32_t)(r >> 32);
    }
    g = key > g ? key : g;
  }
  g = sbx_wave_max(g);
  if (sbx_lane() == 0 && g) atomicMax(&dv->gcc, g);
}

// component order keys: pass 1 the root (phase 0: the label, else the root entry's column)
__global__ __launch_bounds__(ST) void k_sb_comp_keys1(const uint32_t *__restrict__ list, int64_t cnt, int phase0,
                                                      const unsigned long long *__restrict__ rkey,
                                                      uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
  SB_GRID_LOOP(i, cnt) {
    const uint32_t c = list[i];
    key[i] = phase0 ? c : (uint32_t)rkey[c];
    val[i] = c;
  }
}

// pass 2: (hub index if hub_order) << 32 | size; the GCC of a round sorts last (every planned bit set)
__global__ __launch_bounds__(ST) void k_sb_comp_keys2(const uint32_t *__restrict__ comp, int64_t cnt, int phase0,
                                                      int hub_order, const unsigned long long *__restrict__ rkey,
                                                      const uint32_t *__restrict__ csize,
                                                      const uint32_t *__restrict__ hoff, int64_t k,
                                                      unsigned long long gcc, uint64_t gcc_key,
                                                      uint64_t *__restrict__ key) {
  SB_GRID_LOOP(i, cnt) {
    const uint32_t c = comp[i];
    uint64_t hi = 0;
    if (!phase0 && hub_order) {
      const uint32_t spos = (uint32_t)(rkey[c] >> 32);
      int64_t lo = 0, up = k - 1;  // the last q with hoff[q] <= spos
      while (lo < up) {
        const int64_t mid = (lo + up + 1) >> 1;
        if (hoff[mid] <= spos) lo = mid; else up = mid - 1;
      }
      hi = (uint64_t)(k - 1 - lo);
    }
    const bool is_gcc =
        !phase0 && ((unsigned long long)csize[c] << 32 | (uint32_t)~(uint32_t)(rkey[c] >> 32)) == gcc;  // (as k_sb_comps)
    key[i] = is_gcc ? gcc_key : (hi << 32 | csize[c]);
  }
}

// level 0 of the placement BFS: the roots in component order, committed; cidx[label] = component index
__global__ __launch_bounds__(ST) void k_sb_level0(const uint32_t *__restrict__ comp, int64_t cnt, int phase0,
                                                  const unsigned long long *__restrict__ rkey,
                                                  uint32_t *__restrict__ cidx, unsigned char *__restrict__ inE,
                                                  uint32_t *__restrict__ fr, uint32_t *__restrict__ seq,
                                                  SbDev *__restrict__ dv) {
  SB_GRID_LOOP(i, cnt) {
    const uint32_t c = comp[i];
    const uint32_t root = phase0 ? c : (uint32_t)rkey[c];
    cidx[c] = (uint32_t)i;
    inE[root] = 0;
    fr[i] = root;
    seq[i] = root;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dv->f = (unsigned)cnt;
    dv->seq_off = (unsigned)cnt;
    dv->nxt_cnt = 0;
    dv->status = 0;
  }
}

// ---- placement BFS ----------------------------------------------------------------------------------------------------

// one wide level: a wave per frontier vertex; a child's key is (parent rank << 32 | adjacency index), the first to
// lower it from SB_UNSEEN appends it
__global__ __launch_bounds__(ST) void k_sb_bfs_expand(const uint32_t *__restrict__ srp, const uint32_t *__restrict__ scol,
                                                      const unsigned char *__restrict__ inE,
                                                      const uint32_t *__restrict__ fr, int64_t f,
                                                      unsigned long long *key, uint32_t *__restrict__ nxt,
                                                      SbDev *__restrict__ dv) {
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < f; i += nwaves) {
    const uint32_t v = fr[i], s = srp[v], len = srp[v + 1] - s;
    for (uint32_t e0 = 0; e0 < len; e0 += 64) {  // (wave-uniform trip count: the append is a wave operation)
      const uint32_t e = e0 + sbx_lane();
      bool fresh = false;
      uint32_t w = 0;
      if (e < len) {
        w = scol[s + e];
        if (inE[w]) fresh = atomicMin(&key[w], (unsigned long long)i << 32 | e) == SB_UNSEEN;
      }
      const unsigned slot = sbx_wave_append(&dv->nxt_cnt, fresh);
      if (fresh) nxt[slot] = w;
    }
  }
}

__global__ __launch_bounds__(ST) void k_sb_bfs_gather(const uint32_t *__restrict__ nxt, int64_t c,
                                                      const unsigned long long *__restrict__ key,
                                                      uint64_t *__restrict__ k_out, uint32_t *__restrict__ v_out) {
  SB_GRID_LOOP(i, c) {
    const uint32_t w = nxt[i];
    k_out[i] = key[w];
    v_out[i] = w;
  }
}

__global__ __launch_bounds__(ST) void k_sb_bfs_commit(const uint32_t *__restrict__ sorted, int64_t c, uint32_t off,
                                                      unsigned char *__restrict__ inE, uint32_t *__restrict__ fr,
                                                      uint32_t *__restrict__ seq, SbDev *__restrict__ dv) {
  SB_GRID_LOOP(i, c) {
    const uint32_t v = sorted[i];
    inE[v] = 0;
    fr[i] = v;
    seq[off + i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    dv->f = (unsigned)c;
    dv->seq_off = off + (unsigned)c;
    dv->nxt_cnt = 0;
    dv->status = 0;
  }
}

// narrow levels, one workgroup: expand, sort the level by rank in LDS (keys are distinct), commit, repeat until the
// BFS ends (status DONE) or a level holds more than SB_CAP vertices (status WIDE: the level stands unsorted in nxt,
// nxt_cnt long, for the grid path)
__global__ __launch_bounds__(SB_WG) void k_sb_bfs_narrow(const uint32_t *__restrict__ srp, const uint32_t *__restrict__ scol,
                                                         unsigned char *inE, const uint32_t *__restrict__ fr_in,
                                                         unsigned long long *key, uint32_t *__restrict__ nxt,
                                                         uint32_t *__restrict__ seq, SbDev *__restrict__ dv) {
  __shared__ uint32_t s_fr[SB_CAP];
  __shared__ uint32_t s_nv[SB_CAP];
  __shared__ unsigned long long s_nk[SB_CAP];
  __shared__ unsigned s_cnt;
  unsigned f = dv->f, off = dv->seq_off;
  for (unsigned i = threadIdx.x; i < f; i += SB_WG) s_fr[i] = fr_in[i];
  unsigned status = 0, c = 0;
  for (;;) {
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    for (unsigned i = threadIdx.x >> 6; i < f; i += SB_WG / 64) {
      const uint32_t v = s_fr[i], s = srp[v], len = srp[v + 1] - s;
      for (uint32_t e = sbx_lane(); e < len; e += 64) {
        const uint32_t w = scol[s + e];
        if (sb_ld8(&inE[w]) && atomicMin(&key[w], (unsigned long long)i << 32 | e) == SB_UNSEEN) {
          const unsigned slot = atomicAdd(&s_cnt, 1u);
          nxt[slot] = w;
          if (slot < SB_CAP) s_nv[slot] = w;
        }
      }
    }
    __syncthreads();
    c = s_cnt;
    if (c == 0) { status = SB_BFS_DONE; break; }
    if (c > SB_CAP) { status = SB_BFS_WIDE; break; }
    for (unsigned t = threadIdx.x; t < c; t += SB_WG) s_nk[t] = sb_ld64(&key[s_nv[t]]);
    __syncthreads();
    for (unsigned t = threadIdx.x; t < c; t += SB_WG) {
      const unsigned long long mine = s_nk[t];
      unsigned rank = 0;
      for (unsigned u = 0; u < c; u++) rank += s_nk[u] < mine ? 1u : 0u;
      const uint32_t v = s_nv[t];
      s_fr[rank] = v;
      seq[off + rank] = v;
      sb_st8(&inE[v], 0);
    }
    __syncthreads();
    f = c;
    off += c;
  }
  if (threadIdx.x == 0) {
    dv->f = status == SB_BFS_WIDE ? f : 0;
    dv->seq_off = off;
    dv->nxt_cnt = status == SB_BFS_WIDE ? c : 0;
    dv->status = status;
  }
}

// final order of a round: the placed sequence sorted stably by component index; keys and payloads
__global__ __launch_bounds__(ST) void k_sb_seq_keys(const uint32_t *__restrict__ seq, int64_t cnt,
                                                    const uint32_t *__restrict__ label, const uint32_t *__restrict__ cidx,
                                                    uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
  SB_GRID_LOOP(i, cnt) {
    const uint32_t v = seq[i];
    key[i] = cidx[label[v]];
    val[i] = v;
  }
}

__global__ __launch_bounds__(ST) void k_sb_place(const uint32_t *__restrict__ order, int64_t cnt, uint32_t top,
                                                 uint32_t *__restrict__ pos) {
  SB_GRID_LOOP(i, cnt) pos[order[i]] = top - (uint32_t)i;
}

template <typename I>
__global__ __launch_bounds__(ST) void k_sb_out(const uint32_t *__restrict__ pos, int64_t n, I *__restrict__ out) {
  SB_GRID_LOOP(i, n) out[i] = (I)pos[i];
}

struct SbCall {
  sbx_handle_t h;
  int64_t n, k;
  bool greedy, hub_order;
  SbDev *dv;
  uint32_t *srp, *scol;
  unsigned maxdeg;
  unsigned char *inE;
  uint32_t *deg, *parent, *csize, *cidx, *pos;
  int32_t *cur;
  unsigned long long *rkey, *key;
  uint32_t *fr, *nxt, *seq;
  uint32_t *k32a, *k32b, *v32a, *v32b;  // sort buffers, n each
  uint64_t *k64a, *k64b;
  int64_t *x;
  uint32_t *hub, *hlen, *hoff;
  uint64_t *hkey, *hkey_b;
  int64_t placed_back;
  sbx_slashburn_stats st;
};

static unsigned sb_grid(const SbCall &c, int64_t items, int per_block = ST) {
  return sbx_grid_for(items, per_block, (int64_t)c.h->num_cus * 32);
}

// components of S over inE: parent[] becomes the label; returns (count, packed GCC) through one read-back
static int sb_components(SbCall &c, int phase0, unsigned *ncomp, unsigned long long *gcc, unsigned *noroot) {
  sbx_handle_t h = c.h;
  const unsigned gn = sb_grid(c, c.n), gw = sb_grid(c, c.n * 64);
  SBX_KLAUNCH(h, SBX_K_CC, k_sb_cc_init, dim3(gn), dim3(ST), (const unsigned char *)c.inE, c.n, c.parent, c.csize, c.rkey);
  SBX_KLAUNCH(h, SBX_K_CC, k_sb_cc_hook, dim3(gw), dim3(ST), (const uint32_t *)c.srp, (const uint32_t *)c.scol,
              (const unsigned char *)c.inE, c.n, c.parent);
  SBX_KLAUNCH(h, SBX_K_CC, k_sb_cc_final, dim3(gn), dim3(ST), (const unsigned char *)c.inE, c.n, c.parent, c.csize);
  SBX_LAUNCH_CHECK(h);
  if (!phase0)
    SBX_KLAUNCH(h, SBX_K_CC, k_sb_roots, dim3(sbx_grid_for(c.k, 1, (int64_t)h->num_cus * 64)), dim3(ST),
                (const uint32_t *)c.srp, (const uint32_t *)c.scol, (const unsigned char *)c.inE, (const uint32_t *)c.hub,
                (const uint32_t *)c.hoff, c.k, (const uint32_t *)c.parent, c.rkey);
  SBX_HIP(h, hipMemsetAsync(&c.dv->ncomp, 0, offsetof(SbDev, maxdeg) - offsetof(SbDev, ncomp), h->stream));
  SBX_KLAUNCH(h, SBX_K_CC, k_sb_comps, dim3(gn), dim3(ST), (const unsigned char *)c.inE, c.n, (const uint32_t *)c.parent,
              (const uint32_t *)c.csize, (const unsigned long long *)c.rkey, phase0, c.k32a, c.dv);
  SBX_LAUNCH_CHECK(h);
  struct {
    unsigned bad, ncomp;
    unsigned long long gcc;
    unsigned maxdeg, noroot;
  } rb;
  static_assert(sizeof(rb) == offsetof(SbDev, prefix), "read-back covers the head of SbDev");
  SBX_TRY(sbx_readback(h, &rb, c.dv, sizeof(rb)));
  *ncomp = rb.ncomp;
  *gcc = rb.gcc;
  *noroot = rb.noroot;
  c.maxdeg = rb.maxdeg;
  return SBX_OK;
}

// places the first nplace of the ncomp components listed in c.k32a (sorted here) from the back, each by BFS from its
// root; phase 0 keys (size, label), rounds (hub index?, size, root entry column) with the GCC last
static int sb_place_components(SbCall &c, int phase0, unsigned ncomp, unsigned nplace, unsigned long long gcc,
                               int64_t e_size, int64_t expect) {
  sbx_handle_t h = c.h;
  if (nplace == 0) return SBX_OK;
  // sort 1: by root (the list moves from k32a into v32a as the payload)
  uint32_t *list = c.k32a;
  uint32_t *ka = c.k32b, *kb = c.cidx, *va = c.v32a, *vb = c.v32b;  // (cidx is free until level 0)
  SBX_KLAUNCH(h, SBX_K_MISC, k_sb_comp_keys1, dim3(sb_grid(c, ncomp)), dim3(ST), (const uint32_t *)list, (int64_t)ncomp,
              phase0, (const unsigned long long *)c.rkey, ka, va);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_sort_pairs(h, &ka, &kb, &va, &vb, ncomp, 0, sbx_bits_for((uint64_t)(c.n - 1))));
  // sort 2: stable by (hub index?, size)
  const int size_bits = sbx_bits_for((uint64_t)e_size);
  const int hub_bits = (!phase0 && c.hub_order) ? sbx_bits_for((uint64_t)(c.k - 1)) : 0;
  const uint64_t gcc_key = ((hub_bits ? ((1ull << hub_bits) - 1) : 0ull) << 32) | ((1ull << size_bits) - 1);
  uint64_t *k64a = c.k64a, *k64b = c.k64b;
  SBX_KLAUNCH(h, SBX_K_MISC, k_sb_comp_keys2, dim3(sb_grid(c, ncomp)), dim3(ST), (const uint32_t *)va, (int64_t)ncomp,
              phase0, (int)c.hub_order, (const unsigned long long *)c.rkey, (const uint32_t *)c.csize,
              (const uint32_t *)c.hoff, c.k, gcc, gcc_key, k64a);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_sort_pairs(h, &k64a, &k64b, &va, &vb, ncomp, 0, size_bits, 32, 32 + hub_bits));
  const uint32_t *comp = va;
  SBX_KLAUNCH(h, SBX_K_MISC, k_sb_level0, dim3(sb_grid(c, nplace)), dim3(ST), comp, (int64_t)nplace, phase0,
              (const unsigned long long *)c.rkey, c.cidx, c.inE, c.fr, c.seq, c.dv);
  SBX_LAUNCH_CHECK(h);
  // BFS
  const int idx_bits = sbx_bits_for((uint64_t)c.maxdeg);
  int64_t f = nplace, off = nplace;
  for (;;) {
    int64_t cnt = 0;
    if (f <= (int64_t)SB_CAP) {
      SBX_KLAUNCH(h, SBX_K_BFS_SMALL, k_sb_bfs_narrow, dim3(1), dim3(SB_WG), (const uint32_t *)c.srp,
                  (const uint32_t *)c.scol, c.inE, (const uint32_t *)c.fr, c.key, c.nxt, c.seq, c.dv);
      SBX_LAUNCH_CHECK(h);
      unsigned rb[4];
      SBX_TRY(sbx_readback(h, rb, &c.dv->f, sizeof(rb)));
      off = rb[1];
      if (rb[3] == SB_BFS_DONE) break;
      f = rb[0];
      cnt = rb[2];
    } else {
      SBX_KLAUNCH(h, SBX_K_BFS_EXPAND, k_sb_bfs_expand, dim3(sb_grid(c, f * 64)), dim3(ST), (const uint32_t *)c.srp,
                  (const uint32_t *)c.scol, (const unsigned char *)c.inE, (const uint32_t *)c.fr, f, c.key, c.nxt, c.dv);
      SBX_LAUNCH_CHECK(h);
      unsigned rb[4];
      SBX_TRY(sbx_readback(h, rb, &c.dv->f, sizeof(rb)));
      cnt = rb[2];
      if (cnt == 0) break;
    }
    // a wide level: gather (key, vertex), sort by key, commit
    uint64_t *ka64 = c.k64a, *kb64 = c.k64b;
    uint32_t *pa = c.v32a, *pb = c.v32b;
    SBX_KLAUNCH(h, SBX_K_LEVEL_ORDER, k_sb_bfs_gather, dim3(sb_grid(c, cnt)), dim3(ST), (const uint32_t *)c.nxt, cnt,
                (const unsigned long long *)c.key, ka64, pa);
    SBX_LAUNCH_CHECK(h);
    SBX_TRY(sbx_sort_pairs(h, &ka64, &kb64, &pa, &pb, cnt, 0, idx_bits, 32, 32 + sbx_bits_for((uint64_t)(f - 1))));
    SBX_KLAUNCH(h, SBX_K_LEVEL_ORDER, k_sb_bfs_commit, dim3(sb_grid(c, cnt)), dim3(ST), (const uint32_t *)pa, cnt,
                (uint32_t)off, c.inE, c.fr, c.seq, c.dv);
    SBX_LAUNCH_CHECK(h);
    f = cnt;
    off += cnt;
  }
  if (off != expect)
    SBX_FAIL(h, SBX_ERR_INTERNAL, "slashburn: placed %lld of %lld vertices", (long long)off, (long long)expect);
  // the levels sorted stably by component index; the i-th vertex goes to P - i
  uint32_t *ka2 = c.k32a, *kb2 = c.k32b, *va2 = c.v32a, *vb2 = c.v32b;
  SBX_KLAUNCH(h, SBX_K_MISC, k_sb_seq_keys, dim3(sb_grid(c, off)), dim3(ST), (const uint32_t *)c.seq, off,
              (const uint32_t *)c.parent, (const uint32_t *)c.cidx, ka2, va2);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_sort_pairs(h, &ka2, &kb2, &va2, &vb2, off, 0, sbx_bits_for((uint64_t)(nplace - 1))));
  const uint32_t top = (uint32_t)(c.n - 1 - c.placed_back);
  SBX_KLAUNCH(h, SBX_K_MISC, k_sb_place, dim3(sb_grid(c, off)), dim3(ST), (const uint32_t *)va2, off, top, c.pos);
  SBX_LAUNCH_CHECK(h);
  c.placed_back += off;
  return SBX_OK;
}

// the k hubs of E (|E| >= k), placed at base .. base + k - 1 and taken out of E
static int sb_hubs(SbCall &c, int64_t e_size, uint32_t base) {
  sbx_handle_t h = c.h;
  const unsigned gn = sb_grid(c, c.n);
  SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_degree, dim3(sb_grid(c, c.n * 64)), dim3(ST), (const uint32_t *)c.srp,
              (const uint32_t *)c.scol, (const unsigned char *)c.inE, c.n, c.deg, c.greedy ? c.cur : nullptr);
  SBX_LAUNCH_CHECK(h);
  if (c.greedy) {
    uint64_t *ka = c.k64a, *kb = c.k64b;
    SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_greedy_keys, dim3(gn), dim3(ST), (const unsigned char *)c.inE,
                (const uint32_t *)c.deg, c.n, c.maxdeg, ka);
    SBX_LAUNCH_CHECK(h);
    SBX_TRY(sbx_sort_keys(h, &ka, &kb, c.n, 0, sbx_bits_for((uint64_t)(c.n - 1)), 32,
                          32 + sbx_bits_for((uint64_t)c.maxdeg + 1)));
    SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_greedy, dim3(1), dim3(SB_WG), (const uint32_t *)c.srp, (const uint32_t *)c.scol,
                c.inE, (const uint64_t *)ka, e_size, c.maxdeg, c.k, c.cur, c.hub);
    SBX_LAUNCH_CHECK(h);
    SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_hub_commit, dim3(sb_grid(c, c.k)), dim3(ST), (const uint64_t *)nullptr, c.hub, c.k,
                c.n, base, (const uint32_t *)c.srp, c.inE, c.pos, c.hlen);
  } else {
    // tau = the k-th largest degree: one 8-bit digit per pass from the top
    SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_sel_init, dim3(1), dim3(256), c.k, c.dv);
    const int bits = sbx_bits_for((uint64_t)c.maxdeg);
    for (int shift = ((bits + 7) / 8) * 8 - 8; shift >= 0; shift -= 8) {
      SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_sel_hist, dim3(gn), dim3(ST), (const unsigned char *)c.inE,
                  (const uint32_t *)c.deg, c.n, shift, c.dv);
      SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_sel_pick, dim3(1), dim3(64), shift, c.dv);
    }
    SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_sel_flags, dim3(gn), dim3(ST), (const unsigned char *)c.inE,
                (const uint32_t *)c.deg, c.n, (const SbDev *)c.dv, c.x);
    SBX_LAUNCH_CHECK(h);
    SBX_TRY(sbx_exclusive_scan_i64(h, c.x, c.x, c.n, nullptr));
    SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_sel_T, dim3(gn), dim3(ST), (const unsigned char *)c.inE, (const uint32_t *)c.deg,
                c.n, c.k, (const int64_t *)c.x, c.dv);
    SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_sel_mark, dim3(gn), dim3(ST), (const unsigned char *)c.inE,
                (const uint32_t *)c.deg, c.n, c.k, (const int64_t *)c.x, c.dv, c.hkey);
    SBX_LAUNCH_CHECK(h);
    uint64_t *ka = c.hkey, *kb = c.hkey_b;
    SBX_TRY(sbx_sort_keys(h, &ka, &kb, c.k, 0, sbx_bits_for((uint64_t)(c.n - 1)), 32,
                          32 + sbx_bits_for((uint64_t)c.maxdeg)));
    SBX_KLAUNCH(h, SBX_K_DEGREE, k_sb_hub_commit, dim3(sb_grid(c, c.k)), dim3(ST), (const uint64_t *)ka, c.hub, c.k,
                c.n, base, (const uint32_t *)c.srp, c.inE, c.pos, c.hlen);
  }
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_exclusive_scan_u32(h, c.hlen, c.hoff, c.k, c.hoff + c.k));
  return SBX_OK;
}

template <typename I, typename N>
static int sb_typed(sbx_handle_t h, int64_t n, int64_t nnz, const void *row_ptr, const void *col_v, int64_t k,
                    unsigned flags, void *inv_out, sbx_slashburn_stats *stats_host) {
  SBX_TRY(sbx_arena_begin(h));
  SbCall c{};
  c.h = h;
  c.n = n;
  c.k = k;
  c.greedy = flags & SBX_SB_GREEDY;
  c.hub_order = flags & SBX_SB_HUB_ORDER;
  const N *rp = (const N *)row_ptr;
  const I *col = (const I *)col_v;
  SBX_TRY(sbx_salloc(h, 1, &c.dv));
  SBX_HIP(h, hipMemsetAsync(c.dv, 0, sizeof(SbDev), h->stream));
  // ---- S
  SBX_TRY(sbx_salloc(h, (size_t)n + 1, &c.srp));
  SBX_TRY(sbx_salloc(h, (size_t)(2 * nnz + 1), &c.scol));
  if (nnz > 0) {
    uint64_t *tkey = nullptr, *ttmp = nullptr;
    uint32_t *tptr = nullptr, *kscan = nullptr;
    SBX_TRY(sbx_salloc(h, (size_t)nnz, &tkey));
    SBX_TRY(sbx_salloc(h, (size_t)nnz, &ttmp));
    SBX_TRY(sbx_salloc(h, (size_t)n + 1, &tptr));
    SBX_TRY(sbx_salloc(h, (size_t)nnz + 1, &kscan));
    const unsigned gz = sb_grid(c, nnz), gn1 = sb_grid(c, n + 1);
    SBX_KLAUNCH(h, SBX_K_CSC, (k_sb_tkeys<I, N>), dim3(gz), dim3(ST), rp, col, n, nnz, tkey, c.dv);
    SBX_LAUNCH_CHECK(h);
    unsigned bad = 0;
    SBX_TRY(sbx_readback(h, &bad, &c.dv->bad, sizeof(bad)));
    if (bad) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbx_slashburn_reorder: a column lies outside [0, n)");
    SBX_TRY(sbx_sort_keys(h, &tkey, &ttmp, nnz, 0, sbx_bits_for((uint64_t)(n - 1)), 32,
                          32 + sbx_bits_for((uint64_t)(n - 1))));
    SBX_KLAUNCH(h, SBX_K_CSC, k_sb_offsets, dim3(gn1), dim3(ST), (const uint64_t *)tkey, nnz, n, tptr);
    SBX_KLAUNCH(h, SBX_K_CSC, k_sb_keep, dim3(gz), dim3(ST), (const uint64_t *)tkey, nnz, (const uint32_t *)tptr, kscan);
    SBX_LAUNCH_CHECK(h);
    SBX_TRY(sbx_exclusive_scan_u32(h, kscan, kscan, nnz, kscan + nnz));
    SBX_KLAUNCH(h, SBX_K_CSC, (k_sb_rowlen<N>), dim3(gn1), dim3(ST), rp, n, (const uint32_t *)tptr,
                (const uint32_t *)kscan, c.srp);
    SBX_LAUNCH_CHECK(h);
    SBX_TRY(sbx_exclusive_scan_u32(h, c.srp, c.srp, n, c.srp + n));
    SBX_KLAUNCH(h, SBX_K_CSC, (k_sb_emit_stored<I, N>), dim3(gz), dim3(ST), rp, col, n, nnz, (const uint32_t *)c.srp,
                c.scol);
    SBX_KLAUNCH(h, SBX_K_CSC, k_sb_emit_kept, dim3(gz), dim3(ST), (const uint64_t *)tkey, nnz, (const uint32_t *)tptr,
                (const uint32_t *)kscan, (const uint32_t *)c.srp, c.scol);
    SBX_KLAUNCH(h, SBX_K_CSC, k_sb_maxdeg, dim3(sb_grid(c, n)), dim3(ST), (const uint32_t *)c.srp, n, c.dv);
    SBX_LAUNCH_CHECK(h);
  } else {
    SBX_HIP(h, hipMemsetAsync(c.srp, 0, ((size_t)n + 1) * sizeof(uint32_t), h->stream));
  }
  // ---- per-vertex state
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.inE));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.deg));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.cur));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.parent));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.csize));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.cidx));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.pos));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.rkey));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.key));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.fr));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.nxt));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.seq));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.k32a));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.k32b));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.v32a));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.v32b));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.k64a));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.k64b));
  SBX_TRY(sbx_salloc(h, (size_t)n, &c.x));
  const int64_t kk = k < n ? k : n;  // the hub arrays are used only when k <= |E| <= n
  SBX_TRY(sbx_salloc(h, (size_t)kk, &c.hub));
  SBX_TRY(sbx_salloc(h, (size_t)kk, &c.hlen));
  SBX_TRY(sbx_salloc(h, (size_t)kk + 1, &c.hoff));
  SBX_TRY(sbx_salloc(h, (size_t)kk, &c.hkey));
  SBX_TRY(sbx_salloc(h, (size_t)kk, &c.hkey_b));
  SBX_HIP(h, hipMemsetAsync(c.inE, 1, (size_t)n, h->stream));
  SBX_HIP(h, hipMemsetAsync(c.key, 0xFF, (size_t)n * sizeof(unsigned long long), h->stream));
  // ---- phase 0
  unsigned ncomp = 0, noroot = 0;
  unsigned long long gcc = 0;
  SBX_TRY(sb_components(c, 1, &ncomp, &gcc, &noroot));
  c.st.initial_components = ncomp;
  int64_t g_size = (int64_t)(gcc >> 32);
  const bool loop = g_size >= k;
  SBX_TRY(sb_place_components(c, 1, ncomp, loop ? ncomp - 1 : ncomp, gcc, n, loop ? n - g_size : n));
  if (!loop) c.st.final_gcc = g_size;
  // ---- the slash loop
  int64_t e_size = g_size;
  for (int64_t t = 0; loop; t++) {
    SBX_TRY(sb_hubs(c, e_size, (uint32_t)(t * k)));
    c.st.rounds++;
    c.st.hubs += k;
    const int64_t rest = e_size - k;
    SBX_TRY(sb_components(c, 0, &ncomp, &gcc, &noroot));
    if (noroot) SBX_FAIL(h, SBX_ERR_INTERNAL, "slashburn: a component without a root entry");
    if (ncomp == 0) break;
    g_size = (int64_t)(gcc >> 32);
    const bool more = g_size >= k;
    c.st.spoke_components += ncomp - 1;  // (every component but the GCC)
    SBX_TRY(sb_place_components(c, 0, ncomp, more ? ncomp - 1 : ncomp, gcc, rest, more ? rest - g_size : rest));
    if (!more) {
      c.st.final_gcc = g_size;
      break;
    }
    e_size = g_size;
  }
  if (c.placed_back + c.st.hubs != n)
    SBX_FAIL(h, SBX_ERR_INTERNAL, "slashburn: %lld of %lld positions written",
             (long long)(c.placed_back + c.st.hubs), (long long)n);
  SBX_KLAUNCH(h, SBX_K_MISC, k_sb_out<I>, dim3(sb_grid(c, n)), dim3(ST), (const uint32_t *)c.pos, n, (I *)inv_out);
  SBX_LAUNCH_CHECK(h);
  if (stats_host) *stats_host = c.st;
  return SBX_OK;
}

}  // namespace

extern "C" int sbx_slashburn_reorder(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t nnz, const void *row_ptr,
                                     const void *col, int64_t k, unsigned flags, void *inv_perm_out,
                                     sbx_slashburn_stats *stats_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, n >= 0 && nnz >= 0 && (n > 0 || nnz == 0) && (n == 0 || (row_ptr && inv_perm_out)) &&
                     (nnz == 0 || col), "bad argument");
  SBX_REQUIRE(h, k >= 1, "k must be at least 1");
  SBX_REQUIRE(h, (flags & ~(SBX_SB_GREEDY | SBX_SB_HUB_ORDER)) == 0, "unknown flag");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  if (it != SBX_I64 && n >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: row count exceeds int32", __func__);
  if (it == SBX_I32 && nnz >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: nnz exceeds int32", __func__);
  if (stats_host) *stats_host = sbx_slashburn_stats{};
  if (n >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: n >= 2^31", __func__);
  if (2 * nnz >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: 2 nnz >= 2^31", __func__);
  if (n == 0) return SBX_OK;
  if (it == SBX_I32) return sb_typed<int32_t, int32_t>(h, n, nnz, row_ptr, col, k, flags, inv_perm_out, stats_host);
  if (it == SBX_I32_N64) return sb_typed<int32_t, int64_t>(h, n, nnz, row_ptr, col, k, flags, inv_perm_out, stats_host);
  return sb_typed<int64_t, int64_t>(h, n, nnz, row_ptr, col, k, flags, inv_perm_out, stats_host);
}
