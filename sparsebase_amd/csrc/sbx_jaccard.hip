// sbx_jaccard.hip — feature::JaccardWeights on the device: one fp32 Jaccard weight per nonzero of a CSR graph
// (reference: feature/jaccard_weights_cuda.cu:99-150, the reference's only __global__ kernel).
//
// The rules (see include/sbx.h): for the entry at position p of row u with column v
//   kept      unless deg(v) < deg(u), or deg(v) == deg(u) && v > u                              (:126-129)
//   I         entries t of row u (with multiplicity) that the search bst(v, t) finds in row v   (:135-138)
//   J         (float)I / (float)(deg(u) + deg(v) - I), widened for double output                 (:142-144)
//   writes    out[p] = J, and out[bst(v, u)] = J when u occurs in row v                          (:145-146)
// and, the port's own rule, every position those writes miss gets J computed from its own row.
//
// Pipeline, all on the handle's stream, nothing read back:
//   1. fill      out[] = NaN (no J is NaN: the denominator is at least deg(u) >= 1)
//   2. mark      one pass over the nonzeros, balanced by nonzero (the row of every nonzero from a search in row_ptr):
//                the keep rule, and the cost bin of every kept edge by deg(u); a byte per nonzero, counts per bin
//   3. scatter   kept edges (position, row) appended to their bin's segment of one list (wave-aggregated atomics)
//   4. bins      JB_G8 / JB_G16: 8- / 16-lane groups per edge, JB_WAVE: a wave per edge, every lane searching one
//                entry of row u in row v and the group reducing through DPP; JB_BLOCK: a workgroup per edge (a
//                static stride over the bin), row v staged in LDS when it fits
//   5. fix-up    steps 2-4 again over the positions still holding NaN, writing their own position only
// The order of edges inside a bin depends on the atomics; the output does not: every position has one value whoever
// writes it (two kept writers of one position need (u,v) and (v,u) both kept, i.e. u == v).
#include "sbx_device.h"
#include "sbx_internal.h"

namespace {

constexpr int JT = 256;     // threads per workgroup, every kernel
constexpr int JITEMS = 4;   // consecutive nonzeros per thread in mark / scatter
constexpr int JB_G8 = 0, JB_G16 = 1, JB_WAVE = 2, JB_BLOCK = 3, JB_COUNT = 4;
constexpr int64_t JB_MAX_G8 = 8, JB_MAX_G16 = 16, JB_MAX_WAVE = 128;  // deg(u) upper bounds of the first three bins
constexpr int JB_LDS_BYTES = 64 * 1024;  // row v staged when deg(v) * sizeof(id) fits: two workgroups per CU
constexpr unsigned char JB_SKIP = 0xFF;

// counters (u64): [0, 4) edges per bin, [4, 8) scatter cursors
constexpr int JC_CNT = 0, JC_CUR = 4, JC_WORDS = 8;

__device__ __forceinline__ int jac_bin(int64_t du) {
  return du <= JB_MAX_G8 ? JB_G8 : du <= JB_MAX_G16 ? JB_G16 : du <= JB_MAX_WAVE ? JB_WAVE : JB_BLOCK;
}

// the reference's bst (:69-90) over the entries row[0 .. len): 1-based midpoints (left + right) >> 1, index mid - 1.
// Returns the index the midpoint sequence lands on, or -1.
template <typename I, typename T>
__device__ __forceinline__ int64_t jac_bst(const T *row, int64_t len, I target) {
  int64_t left = 1, right = len;
  while (left <= right) {
    const int64_t mid = (int64_t)(((uint64_t)left + (uint64_t)right) >> 1);
    const I c = (I)row[mid - 1];
    if (c > target) right = mid - 1;
    else if (c < target) left = mid + 1;
    else return mid - 1;
  }
  return -1;
}

template <typename F>
__device__ __forceinline__ bool jac_is_nan(F x) { return x != x; }

// rows of a thread's JITEMS consecutive positions [p0, p0 + k): two searches over all rows, then narrow ones
template <typename N>
__device__ __forceinline__ void jac_rows(const N *__restrict__ rp, int64_t n, int64_t p0, int k, int64_t *row) {
  row[0] = sbx_row_of(rp, p0, 0, n - 1);
  const int64_t r_last = sbx_row_of(rp, p0 + k - 1, row[0], n - 1);
#pragma unroll
  for (int j = 1; j < JITEMS; j++)
    if (j < k) row[j] = sbx_row_of(rp, p0 + j, row[j - 1], r_last);
}

__global__ __launch_bounds__(JT) void k_jac_fill_f32(uint32_t *__restrict__ out, int64_t count) {
  int64_t i = (int64_t)blockIdx.x * JT + threadIdx.x;
  for (; i < count; i += (int64_t)gridDim.x * JT) out[i] = 0x7FC00000u;
}
__global__ __launch_bounds__(JT) void k_jac_fill_f64(uint64_t *__restrict__ out, int64_t count) {
  int64_t i = (int64_t)blockIdx.x * JT + threadIdx.x;
  for (; i < count; i += (int64_t)gridDim.x * JT) out[i] = 0x7FF8000000000000ull;
}

// step 2.  FIXUP = false: the keep rule; true: the positions still NaN.  A column outside [0, n) is read as a row
// without entries (never searched): such an entry is skipped, and its fix-up weight is 0.
template <typename I, typename N, typename F, bool FIXUP>
__global__ __launch_bounds__(JT) void k_jac_mark(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                 int64_t nnz, const F *__restrict__ out, unsigned char *__restrict__ code,
                                                 unsigned long long *__restrict__ ctr) {
  const int64_t stride = (int64_t)gridDim.x * JT * JITEMS;
  for (int64_t p0 = ((int64_t)blockIdx.x * JT + threadIdx.x) * JITEMS; p0 - (int64_t)threadIdx.x * JITEMS < nnz;
       p0 += stride) {
    const int k = p0 < nnz ? (int)(nnz - p0 < JITEMS ? nnz - p0 : JITEMS) : 0;
    int64_t row[JITEMS];
    if (k) jac_rows(rp, n, p0, k, row);
    int bins[JITEMS];
#pragma unroll
    for (int j = 0; j < JITEMS; j++) {
      bins[j] = -1;
      if (j < k) {
        const int64_t p = p0 + j, u = row[j];
        const int64_t du = (int64_t)rp[u + 1] - (int64_t)rp[u];
        bool take;
        if (FIXUP) {
          take = jac_is_nan(out[p]);
        } else {
          const int64_t v = (int64_t)col[p];
          const int64_t dv = (v >= 0 && v < n) ? (int64_t)rp[v + 1] - (int64_t)rp[v] : -1;
          take = !(dv < du || (dv == du && v > u));
        }
        bins[j] = take ? jac_bin(du) : -1;
        code[p] = take ? (unsigned char)bins[j] : JB_SKIP;
      }
    }
#pragma unroll
    for (int b = 0; b < JB_COUNT; b++) {
      int c = 0;
#pragma unroll
      for (int j = 0; j < JITEMS; j++) c += bins[j] == b;
      const unsigned long long tot = (unsigned long long)sbx_wave_sum(c);
      if (tot && sbx_lane() == 0) atomicAdd(&ctr[JC_CNT + b], tot);
    }
  }
}

// step 3: (position, row) of every marked nonzero into its bin's segment [sum of the counts before it, ...)
template <typename I, typename N>
__global__ __launch_bounds__(JT) void k_jac_scatter(const N *__restrict__ rp, int64_t n, int64_t nnz,
                                                    const unsigned char *__restrict__ code,
                                                    unsigned long long *__restrict__ ctr, N *__restrict__ epos,
                                                    I *__restrict__ erow) {
  unsigned long long base[JB_COUNT];
  base[0] = 0;
#pragma unroll
  for (int b = 1; b < JB_COUNT; b++) base[b] = base[b - 1] + ctr[JC_CNT + b - 1];
  const int64_t stride = (int64_t)gridDim.x * JT * JITEMS;
  for (int64_t p0 = ((int64_t)blockIdx.x * JT + threadIdx.x) * JITEMS; p0 - (int64_t)threadIdx.x * JITEMS < nnz;
       p0 += stride) {
    const int k = p0 < nnz ? (int)(nnz - p0 < JITEMS ? nnz - p0 : JITEMS) : 0;
    unsigned char c[JITEMS];
    bool any = false;
#pragma unroll
    for (int j = 0; j < JITEMS; j++) {
      c[j] = j < k ? code[p0 + j] : JB_SKIP;
      any |= c[j] != JB_SKIP;
    }
    int64_t row[JITEMS];
    if (any) jac_rows(rp, n, p0, k, row);
#pragma unroll
    for (int j = 0; j < JITEMS; j++) {
#pragma unroll
      for (int b = 0; b < JB_COUNT; b++) {
        const bool want = c[j] == b;
        const unsigned long long slot = sbx_wave_append64(&ctr[JC_CUR + b], want);
        if (want) {
          epos[base[b] + slot] = (N)(p0 + j);
          erow[base[b] + slot] = (I)row[j];
        }
      }
    }
  }
}

template <typename F>
__device__ __forceinline__ void jac_write(F *__restrict__ out, int64_t p, int64_t other, int64_t cnt, int64_t du,
                                          int64_t dv) {
  const float j = (float)cnt / (float)(du + dv - cnt);
  out[p] = (F)j;
  if (other >= 0) out[other] = (F)j;
}

// sum over each aligned group of G lanes, every lane of the group gets it (all G lanes active)
template <int G>
__device__ __forceinline__ int jac_group_sum(int x) {
  if constexpr (G == 64) {
    return sbx_wave_sum(x);
  } else {
    x += __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, false);                     // quad_perm [1,0,3,2]
    x += __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, false);                     // quad_perm [2,3,0,1]
    x += __builtin_amdgcn_mov_dpp(x, SBX_DPP_ROW_HALF_MIRROR, 0xF, 0xF, false);  // 8-lane halves
    if constexpr (G == 16) x += __builtin_amdgcn_mov_dpp(x, SBX_DPP_ROW_MIRROR, 0xF, 0xF, false);
    static_assert(G == 8 || G == 16, "8, 16 or 64 lanes");
    return x;
  }
}

// step 4, bins JB_G8 / JB_G16 / JB_WAVE: a group of G lanes per edge, lane l searches entries l, l + G, ... of row u
template <typename I, typename N, typename F, int G, bool OTHER>
__global__ __launch_bounds__(JT) void k_jac_group(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                  const N *__restrict__ epos, const I *__restrict__ erow,
                                                  const unsigned long long *__restrict__ ctr, int bin,
                                                  F *__restrict__ out) {
  unsigned long long lo = 0;
  for (int b = 0; b < bin; b++) lo += ctr[JC_CNT + b];
  const unsigned long long hi = lo + ctr[JC_CNT + bin];
  const int g = threadIdx.x % G;
  const unsigned long long groups = (unsigned long long)gridDim.x * (JT / G);
  for (unsigned long long e = lo + ((unsigned long long)blockIdx.x * JT + threadIdx.x) / G; e < hi; e += groups) {
    const int64_t p = (int64_t)epos[e], u = (int64_t)erow[e];
    const int64_t ru = (int64_t)rp[u], du = (int64_t)rp[u + 1] - ru;
    const int64_t v = (int64_t)col[p];
    const bool v_ok = v >= 0 && v < n;
    const int64_t rv = v_ok ? (int64_t)rp[v] : 0, dv = v_ok ? (int64_t)rp[v + 1] - rv : 0;
    int cnt = 0;
    for (int64_t t = g; t < du; t += G) cnt += jac_bst<I>(col + rv, dv, col[ru + t]) >= 0;
    cnt = jac_group_sum<G>(cnt);
    if (g == 0) {
      int64_t other = -1;
      if (OTHER) {
        other = jac_bst<I>(col + rv, dv, (I)u);
        if (other >= 0) other += rv;
      }
      jac_write(out, p, other, cnt, du, dv);
    }
  }
}

// step 4, bin JB_BLOCK: a workgroup per edge, edges by a static stride; row v in LDS when it fits, else searched where
// it lies.  The loop's trip count is uniform by construction (no lane-0-only step at its head: with a ticket fetched by
// lane 0 there, the compiler splits the loop into a lane-0 outer and an inner loop the other 63 lanes of wave 0 keep
// running, past the barrier, on the old ticket — the workgroup never leaves it).
template <typename I, typename N, typename F, bool OTHER>
__global__ __launch_bounds__(JT) void k_jac_block(const N *__restrict__ rp, const I *__restrict__ col, int64_t n,
                                                  const N *__restrict__ epos, const I *__restrict__ erow,
                                                  const unsigned long long *__restrict__ ctr, F *__restrict__ out) {
  constexpr int64_t CAP = JB_LDS_BYTES / sizeof(I);
  __shared__ I s_row[CAP];
  __shared__ int s_red[JT / 64];
  const unsigned long long lo = ctr[JC_CNT + 0] + ctr[JC_CNT + 1] + ctr[JC_CNT + 2];
  const unsigned long long hi = lo + ctr[JC_CNT + JB_BLOCK];
  for (unsigned long long e = lo + blockIdx.x; e < hi; e += gridDim.x) {
    const int64_t p = (int64_t)epos[e], u = (int64_t)erow[e];
    const int64_t ru = (int64_t)rp[u], du = (int64_t)rp[u + 1] - ru;
    const int64_t v = (int64_t)col[p];
    const bool v_ok = v >= 0 && v < n;
    const int64_t rv = v_ok ? (int64_t)rp[v] : 0, dv = v_ok ? (int64_t)rp[v + 1] - rv : 0;
    int cnt = 0;
    if (dv <= CAP) {
      for (int64_t t = threadIdx.x; t < dv; t += JT) s_row[t] = col[rv + t];
      __syncthreads();
      for (int64_t t = threadIdx.x; t < du; t += JT) cnt += jac_bst<I>(s_row, dv, col[ru + t]) >= 0;
    } else {
      for (int64_t t = threadIdx.x; t < du; t += JT) cnt += jac_bst<I>(col + rv, dv, col[ru + t]) >= 0;
    }
    cnt = sbx_block_sum<int, JT>(cnt, s_red);  // (its closing barrier also frees s_row for the next edge)
    if (threadIdx.x == 0) {
      int64_t other = -1;
      if (OTHER) {
        other = jac_bst<I>(col + rv, dv, (I)u);
        if (other >= 0) other += rv;
      }
      jac_write(out, p, other, cnt, du, dv);
    }
  }
}

template <typename N>
__global__ __launch_bounds__(JT) void k_jac_max_degree(const N *__restrict__ rp, int64_t n,
                                                       unsigned long long *__restrict__ mx) {
  unsigned long long m = 0;
  for (int64_t i = (int64_t)blockIdx.x * JT + threadIdx.x; i < n; i += (int64_t)gridDim.x * JT) {
    const unsigned long long d = (unsigned long long)((int64_t)rp[i + 1] - (int64_t)rp[i]);
    m = d > m ? d : m;
  }
  m = sbx_wave_max(m);
  if (sbx_lane() == 0 && m) atomicMax(mx, m);
}

}  // namespace

// steps 2-4 of one pass (FIXUP: the positions still NaN, own position only)
template <typename I, typename N, typename F, bool FIXUP>
static int jaccard_pass(sbx_handle_t h, int64_t n, int64_t nnz, const N *rp, const I *col, F *out, unsigned char *code,
                        N *epos, I *erow, unsigned long long *ctr) {
  const unsigned g_items = sbx_grid_for((nnz + JITEMS - 1) / JITEMS, JT, (int64_t)h->num_cus * 64);
  SBX_HIP(h, hipMemsetAsync(ctr, 0, JC_WORDS * sizeof(unsigned long long), h->stream));
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_jac_mark<I, N, F, FIXUP>), dim3(g_items), dim3(JT), rp, col, n, nnz, (const F *)out,
              code, ctr);
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_jac_scatter<I, N>), dim3(g_items), dim3(JT), rp, n, nnz, (const unsigned char *)code,
              ctr, epos, erow);
  // fixed grids over the bins (their sizes stay on the device): enough groups to fill every CU
  const unsigned g_bins = (unsigned)h->num_cus * 16;
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_jac_group<I, N, F, 8, !FIXUP>), dim3(g_bins), dim3(JT), rp, col, n, (const N *)epos,
              (const I *)erow, (const unsigned long long *)ctr, JB_G8, out);
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_jac_group<I, N, F, 16, !FIXUP>), dim3(g_bins), dim3(JT), rp, col, n, (const N *)epos,
              (const I *)erow, (const unsigned long long *)ctr, JB_G16, out);
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_jac_group<I, N, F, 64, !FIXUP>), dim3(g_bins), dim3(JT), rp, col, n, (const N *)epos,
              (const I *)erow, (const unsigned long long *)ctr, JB_WAVE, out);
  SBX_KLAUNCH(h, SBX_K_FEATURE, (k_jac_block<I, N, F, !FIXUP>), dim3((unsigned)h->num_cus * 2), dim3(JT), rp, col, n,
              (const N *)epos, (const I *)erow, (const unsigned long long *)ctr, out);
  SBX_LAUNCH_CHECK(h);
  return SBX_OK;
}

template <typename I, typename N, typename F>
static int jaccard_typed(sbx_handle_t h, int64_t n, int64_t nnz, const void *row_ptr, const void *col_v, void *out_v) {
  SBX_TRY(sbx_arena_begin(h));
  if (nnz == 0) return SBX_OK;
  const N *rp = (const N *)row_ptr;
  const I *col = (const I *)col_v;
  F *out = (F *)out_v;
  unsigned long long *ctr = nullptr;
  SBX_TRY(sbx_salloc(h, JC_WORDS, &ctr));
  if (nnz >= ((int64_t)1 << 31)) {  // the group counts are 32-bit: every degree must be below 2^31
    SBX_HIP(h, hipMemsetAsync(ctr, 0, sizeof(unsigned long long), h->stream));
    SBX_KLAUNCH(h, SBX_K_FEATURE, k_jac_max_degree<N>, dim3(sbx_grid_for(n, JT, (int64_t)h->num_cus * 8)), dim3(JT), rp,
                n, ctr);
    SBX_LAUNCH_CHECK(h);
    unsigned long long mx = 0;
    SBX_TRY(sbx_readback(h, &mx, ctr, sizeof(mx)));
    if (mx >= ((unsigned long long)1 << 31)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbx_csr_jaccard_weights: a degree >= 2^31");
  }
  unsigned char *code = nullptr;
  N *epos = nullptr;
  I *erow = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &code));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &epos));
  SBX_TRY(sbx_salloc(h, (size_t)nnz, &erow));
  const unsigned g_fill = sbx_grid_for(nnz, JT, (int64_t)h->num_cus * 32);
  if (sizeof(F) == 4)
    SBX_KLAUNCH(h, SBX_K_FEATURE, k_jac_fill_f32, dim3(g_fill), dim3(JT), (uint32_t *)out, nnz);
  else
    SBX_KLAUNCH(h, SBX_K_FEATURE, k_jac_fill_f64, dim3(g_fill), dim3(JT), (uint64_t *)out, nnz);
  SBX_TRY((jaccard_pass<I, N, F, false>(h, n, nnz, rp, col, out, code, epos, erow, ctr)));
  SBX_TRY((jaccard_pass<I, N, F, true>(h, n, nnz, rp, col, out, code, epos, erow, ctr)));
  SBX_PROF_BYTES(h, SBX_K_FEATURE, (int64_t)(2 * sizeof(I) + 3 * sizeof(F)) * nnz + (int64_t)sizeof(N) * (n + 1));
  return SBX_OK;
}

template <typename I, typename N>
static int jaccard_feature(sbx_handle_t h, int64_t n, int64_t nnz, const void *row_ptr, const void *col,
                           int feature_bytes, void *out) {
  return feature_bytes == 4 ? jaccard_typed<I, N, float>(h, n, nnz, row_ptr, col, out)
                            : jaccard_typed<I, N, double>(h, n, nnz, row_ptr, col, out);
}

extern "C" int sbx_csr_jaccard_weights(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t nnz, const void *row_ptr,
                                       const void *col, int feature_bytes, void *weights_out) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, n >= 0 && nnz >= 0 && (n > 0 || nnz == 0) && (nnz == 0 || (row_ptr && col && weights_out)),
              "bad argument");
  SBX_REQUIRE(h, feature_bytes == 4 || feature_bytes == 8, "feature type must be float or double");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  if (it != SBX_I64 && n >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: row count exceeds int32", __func__);
  if (it == SBX_I32 && nnz >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: nnz exceeds int32", __func__);
  if (it == SBX_I32) return jaccard_feature<int32_t, int32_t>(h, n, nnz, row_ptr, col, feature_bytes, weights_out);
  if (it == SBX_I32_N64) return jaccard_feature<int32_t, int64_t>(h, n, nnz, row_ptr, col, feature_bytes, weights_out);
  return jaccard_feature<int64_t, int64_t>(h, n, nnz, row_ptr, col, feature_bytes, weights_out);
}
