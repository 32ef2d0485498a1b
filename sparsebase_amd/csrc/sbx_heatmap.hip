// sbx_heatmap.hip — reorder::ReorderHeatmap on the device (reference: reorder/reorder_heatmap.cc:43-119): the share
// of a CSR's nonzeros in every cell of a b x b grid once rows and columns are placed by two orders.
//
// The rule (include/sbx.h): bsize = n / b; entry (i, c) counts in cell (min(order_r[i] / bsize, b - 1),
// min(order_c[c] / bsize, b - 1)); heat = (float)count / (float)nnz.  Pipeline, on the handle's stream, one read-back:
//   1. check     every entry of order_r and order_c is >= 0 (else the error word is raised)
//   2. count     one pass over the nonzeros.  A wave takes a chunk of HCHUNK consecutive nonzeros; the chunk's first
//                and last rows come from two wave-cooperative searches in row_ptr, lane l works out the row block
//                bu of row r0 + l once (read back by the lanes through a shuffle), and every entry gathers
//                order_c[col].  With b * b cells in LDS (HM_SMALL / HM_LARGE cells, several copies of the grid where
//                they fit, so that the lanes of a wave spread over them) the counts go to per-workgroup histograms
//                that are added to the 64-bit global counters at the end; otherwise every entry adds 1 to its 64-bit
//                global counter.  A column outside [0, m) raises the error word and counts nowhere.
//   3. convert   heat[i] = (float)count[i] / (float)nnz (a correctly rounded division: no fast-math), widened for
//                double output; skipped when the error word is set, so a refused call writes nothing.
// Every update is an integer add: the counts, and so every bit of the output, do not depend on arrival order.
#include "sbx_device.h"
#include "sbx_internal.h"

namespace {

constexpr int HT = 256;                 // threads per workgroup
constexpr int HITEMS = 8;               // 64-entry slices per chunk
constexpr int64_t HCHUNK = 64 * HITEMS;  // nonzeros per wave and chunk
constexpr int HM_SMALL = 2048;          // LDS cells (8 KiB) of the small-grid kernel
constexpr int HM_LARGE = 16384;         // LDS cells (64 KiB) of the large-grid kernel: b <= 128 (larger b: global)
constexpr int HM_COPIES = 16;           // at most this many copies of the grid per workgroup

template <typename I>
__global__ __launch_bounds__(HT) void k_heat_check(const I *__restrict__ order_r, int64_t n,
                                                   const I *__restrict__ order_c, int64_t m, int *err) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * HT + threadIdx.x; i < n + m; i += (int64_t)gridDim.x * HT)
    bad = bad || (i < n ? order_r[i] : order_c[i - n]) < 0;
  if (bad) *err = 1;
}

// block of a non-negative position: min(p / bsize, b - 1); lim = b * bsize (positions at or past it clamp)
__device__ __forceinline__ uint32_t heat_block(uint64_t p, uint64_t bsize, uint64_t b, uint64_t lim) {
  if (p >= lim) return (uint32_t)(b - 1);
  if (lim <= 0xFFFFFFFFull) return (uint32_t)p / (uint32_t)bsize;  // (the common case: 32-bit division)
  return (uint32_t)(p / bsize);
}

// CELLS = 0: global counters only; else an LDS histogram of CELLS 32-bit cells holding `copies` grids of `stride` cells
template <typename I, typename N, int CELLS>
__global__ __launch_bounds__(HT) void k_heat_count(const N *__restrict__ rp, const I *__restrict__ col,
                                                   const I *__restrict__ order_r, const I *__restrict__ order_c,
                                                   int64_t n, int64_t m, int64_t nnz, uint64_t bsize, uint64_t b,
                                                   int copies, int stride, unsigned long long *__restrict__ cnt,
                                                   int *err) {
  __shared__ uint32_t hist[CELLS > 0 ? CELLS : 1];
  const int lane = sbx_lane();
  const uint64_t lim = b * bsize;
  uint32_t *mine = hist;
  if constexpr (CELLS > 0) {
    for (int i = threadIdx.x; i < copies * stride; i += HT) hist[i] = 0;
    mine = hist + (threadIdx.x % copies) * stride;
    __syncthreads();
  }
  bool bad = false;
  const int64_t waves = (int64_t)gridDim.x * (HT / 64);
  for (int64_t e0 = ((int64_t)blockIdx.x * (HT / 64) + sbx_wave_in_block()) * HCHUNK; e0 < nnz; e0 += waves * HCHUNK) {
    const int64_t e1 = e0 + HCHUNK < nnz ? e0 + HCHUNK : nnz;
    // rows r0 <= r1 of the chunk's first and last nonzeros: the last row r with rp[r] <= e
    // (clamped to [0, n): row_ptr[0] = 0 and row_ptr[n] = nnz make the clamps no-ops)
    const int64_t r0 = std::min<int64_t>(std::max<int64_t>(sbx_wave_upper_bound(rp, n + 1, (N)e0) - 1, 0), n - 1);
    const int64_t r1 =
        std::min<int64_t>(r0 + std::max<int64_t>(sbx_wave_upper_bound(rp + r0, n + 1 - r0, (N)(e1 - 1)) - 1, 0), n - 1);
    uint32_t bu_lane = 0;
    if (r0 + lane <= r1) {
      const I u = order_r[r0 + lane];
      bu_lane = u >= 0 ? heat_block((uint64_t)u, bsize, b, lim) : 0xFFFFFFFFu;
    }
    int64_t r = r0;
#pragma unroll 2
    for (int k = 0; k < HITEMS; k++) {
      const int64_t e = e0 + k * 64 + lane;
      const bool live = e < e1;
      if (live) {  // the row of e: the last r in [r, r1] with rp[r] <= e
        int64_t hi = r1;
        while (r < hi) {
          const int64_t mid = (r + hi + 1) >> 1;
          if ((int64_t)rp[mid] <= e) r = mid; else hi = mid - 1;
        }
      }
      const int64_t dr = r - r0;
      const uint32_t bu_sh = (uint32_t)__shfl((int)bu_lane, (int)(dr < 64 ? dr : 0), 64);
      if (!live) continue;
      uint32_t bu = bu_sh;
      if (dr >= 64) {
        const I u = order_r[r];
        bu = u >= 0 ? heat_block((uint64_t)u, bsize, b, lim) : 0xFFFFFFFFu;
      }
      const I c = col[e];
      if (c < 0 || (int64_t)c >= m) {
        bad = true;
        continue;
      }
      const I v = order_c[c];
      if (v < 0 || bu == 0xFFFFFFFFu) continue;  // (raised by k_heat_check)
      const uint64_t cell = (uint64_t)bu * b + heat_block((uint64_t)v, bsize, b, lim);
      if constexpr (CELLS > 0) atomicAdd(&mine[cell], 1u);
      else atomicAdd(&cnt[cell], 1ull);
    }
  }
  if (bad) *err = 1;
  if constexpr (CELLS > 0) {
    __syncthreads();
    const int b2 = (int)(b * b);
    for (int i = threadIdx.x; i < b2; i += HT) {
      unsigned long long s = 0;
      for (int j = 0; j < copies; j++) s += hist[j * stride + i];
      if (s) atomicAdd(&cnt[i], s);
    }
  }
}

template <typename F>
__global__ __launch_bounds__(HT) void k_heat_convert(const unsigned long long *__restrict__ cnt, int64_t cells,
                                                     float denom, const int *__restrict__ err, F *__restrict__ out) {
  if (*err) return;
  for (int64_t i = (int64_t)blockIdx.x * HT + threadIdx.x; i < cells; i += (int64_t)gridDim.x * HT)
    out[i] = (F)((float)(long long)cnt[i] / denom);
}

template <typename I, typename N>
static int heat_typed(sbx_handle_t h, int64_t n, int64_t m, int64_t nnz, const void *row_ptr, const void *col,
                      const void *order_r, const void *order_c, int64_t b, int feature_bytes, void *out) {
  SBX_TRY(sbx_arena_begin(h));
  const int64_t cells = b * b;
  int *err = nullptr;
  unsigned long long *cnt = nullptr;
  SBX_TRY(sbx_salloc(h, 1, &err));
  SBX_TRY(sbx_salloc(h, (size_t)cells, &cnt));
  SBX_HIP(h, hipMemsetAsync(err, 0, sizeof(int), h->stream));
  SBX_HIP(h, hipMemsetAsync(cnt, 0, (size_t)cells * sizeof(unsigned long long), h->stream));
  const int64_t cap = (int64_t)h->num_cus * 8;
  SBX_KLAUNCH(h, SBX_K_FEATURE, k_heat_check<I>, dim3(sbx_grid_for(n + m, HT, cap)), dim3(HT), (const I *)order_r, n,
              (const I *)order_c, m, err);
  if (nnz > 0) {
    const uint64_t bsize = (uint64_t)(n / b), ub = (uint64_t)b;
    // every workgroup's share stays below 2^31 entries, so a 32-bit LDS cell cannot wrap
    int64_t grid = sbx_grid_for((nnz + HCHUNK - 1) / HCHUNK, HT / 64, cap);
    if (grid < (nnz >> 30) + 1) grid = (nnz >> 30) + 1;
    const dim3 g((unsigned)grid), t(HT);
    const N *rp = (const N *)row_ptr;
    const I *c = (const I *)col, *orr = (const I *)order_r, *orc = (const I *)order_c;
    if (cells <= HM_LARGE) {  // b <= 128: LDS histograms
      const int lds = cells <= HM_SMALL / 2 ? HM_SMALL : HM_LARGE;
      int stride = (int)(cells | 1);  // odd: the copies start on different banks
      int copies = (int)std::min<int64_t>(HM_COPIES, lds / stride);
      if (copies == 0) {  // (b = 128: one grid fills the LDS)
        copies = 1;
        stride = (int)cells;
      }
      if (lds == HM_SMALL)
        SBX_KLAUNCH(h, SBX_K_FEATURE, (k_heat_count<I, N, HM_SMALL>), g, t, rp, c, orr, orc, n, m, nnz, bsize, ub,
                    copies, stride, cnt, err);
      else
        SBX_KLAUNCH(h, SBX_K_FEATURE, (k_heat_count<I, N, HM_LARGE>), g, t, rp, c, orr, orc, n, m, nnz, bsize, ub,
                    copies, stride, cnt, err);
    } else {
      SBX_KLAUNCH(h, SBX_K_FEATURE, (k_heat_count<I, N, 0>), g, t, rp, c, orr, orc, n, m, nnz, bsize, ub, 1, 0, cnt,
                  err);
    }
  }
  const dim3 gc(sbx_grid_for(cells, HT, cap)), tc(HT);
  if (feature_bytes == 4)
    SBX_KLAUNCH(h, SBX_K_FEATURE, k_heat_convert<float>, gc, tc, (const unsigned long long *)cnt, cells, (float)nnz,
                (const int *)err, (float *)out);
  else
    SBX_KLAUNCH(h, SBX_K_FEATURE, k_heat_convert<double>, gc, tc, (const unsigned long long *)cnt, cells, (float)nnz,
                (const int *)err, (double *)out);
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_FEATURE, (int64_t)(2 * sizeof(I)) * nnz + (int64_t)sizeof(N) * (n + 1) +
                                       (int64_t)sizeof(I) * (n + m) + (int64_t)(8 + feature_bytes) * cells);
  int bad = 0;
  SBX_TRY(sbx_readback(h, &bad, err, sizeof(bad)));
  if (bad) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbx_csr_reorder_heatmap: a column outside [0, m) or a negative order entry");
  return SBX_OK;
}

}  // namespace

extern "C" int sbx_csr_reorder_heatmap(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t m, int64_t nnz,
                                       const void *row_ptr, const void *col, const void *order_r, const void *order_c,
                                       int64_t num_parts, int feature_bytes, void *heat_out) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, n >= 0 && m >= 0 && nnz >= 0, "bad argument");
  SBX_REQUIRE(h, feature_bytes == 4 || feature_bytes == 8, "feature type must be float or double");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  SBX_REQUIRE(h, num_parts >= 1 && num_parts <= n && num_parts <= m,
              "Cannot generate heatmap for matrix when num_parts > number of rows or columns (or num_parts < 1)");
  SBX_REQUIRE(h, row_ptr && order_r && order_c && heat_out && (nnz == 0 || col), "bad argument");
  if (it != SBX_I64 && (n >= ((int64_t)1 << 31) || m >= ((int64_t)1 << 31)))
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: dimension exceeds int32", __func__);
  if (it == SBX_I32 && nnz >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: nnz exceeds int32", __func__);
  if (num_parts > ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_OOM, "%s: num_parts^2 counters", __func__);
  if (it == SBX_I32)
    return heat_typed<int32_t, int32_t>(h, n, m, nnz, row_ptr, col, order_r, order_c, num_parts, feature_bytes, heat_out);
  if (it == SBX_I32_N64)
    return heat_typed<int32_t, int64_t>(h, n, m, nnz, row_ptr, col, order_r, order_c, num_parts, feature_bytes, heat_out);
  return heat_typed<int64_t, int64_t>(h, n, m, nnz, row_ptr, col, order_r, order_c, num_parts, feature_bytes, heat_out);
}
