// sbx_boba.hip — reorder::BOBAReorder on the device (reference: reorder/boba_reorder.cc:33-138): the "order by
// attachment" inverse permutation of the max(n, m) vertices of a COO.
//
// The rule (include/sbx.h): the vertices with a row entry by (mincol(v), v), then the vertices that occur only as a
// column by id, then the rest by id.  Pipeline, on the handle's stream, one read-back at the end:
//   1. entries   one pass over the COO: atomicMin of the column into key[row] (key[] starts at 0xFFFFFFFF) and a
//                byte seen[col] = 1.  Row-sorted input has runs of equal rows inside a wave: every run is reduced
//                across its lanes and only its first lane issues the atomic.  Every atomic and every byte store is
//                skipped when a plain read already shows the value (key[] only falls; seen[] only rises), which keeps
//                a hub's word quiet on unsorted input.  Ids outside [0, nodes) raise the error word.
//   2. keys      key[v] = mincol(v) for group 1, nodes for group 2, nodes + 1 for group 3; val[v] = v
//   3. sort      one stable radix sort of (key, v) over all vertices: the ids go in ascending, so stability gives the
//                id tie-break inside group 1 and the id order of groups 2 and 3
//   4. scatter   inv[val[p]] = p, skipped when the error word is set (so a refused call writes nothing)
// Every atomic is an integer minimum: the result does not depend on the order in which the entries arrive.
#include "sbx_device.h"
#include "sbx_internal.h"

namespace {

constexpr int BT = 256;      // threads per workgroup
constexpr int BITEMS = 4;    // 64-entry slices per wave and chunk in the entry pass
constexpr uint32_t BNONE = 0xFFFFFFFFu;

// min over the lanes of this lane's run of equal rows, at and after this lane (lanes whose row differs from this
// lane's never contribute; on row-sorted input the run's first lane gets the whole run's minimum).  A lane with
// row == BNONE holds no entry.
__device__ __forceinline__ uint32_t boba_run_min(uint32_t row, uint32_t v) {
  const int lane = sbx_lane();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t r2 = (uint32_t)__shfl_down((int)row, d, 64);
    const uint32_t v2 = (uint32_t)__shfl_down((int)v, d, 64);
    if (lane + d < 64 && r2 == row && v2 < v) v = v2;
  }
  return v;
}

template <typename I>
__global__ __launch_bounds__(BT) void k_boba_entries(const I *__restrict__ row, const I *__restrict__ col, int64_t nnz,
                                                     uint32_t nodes, uint32_t *key, unsigned char *seen, int *err) {
  const int lane = sbx_lane();
  const int64_t waves = (int64_t)gridDim.x * (BT / 64);
  const int64_t chunk = 64 * BITEMS;
  bool bad = false;
  for (int64_t base = ((int64_t)blockIdx.x * (BT / 64) + sbx_wave_in_block()) * chunk; base < nnz;
       base += waves * chunk) {
    I r[BITEMS], c[BITEMS];
#pragma unroll
    for (int k = 0; k < BITEMS; k++) {
      const int64_t e = base + k * 64 + lane;
      r[k] = e < nnz ? row[e] : (I)-1;
      c[k] = e < nnz ? col[e] : (I)-1;
    }
#pragma unroll
    for (int k = 0; k < BITEMS; k++) {
      const int64_t e = base + k * 64 + lane;
      const bool live = e < nnz;
      const bool ok = live && r[k] >= 0 && (uint64_t)r[k] < nodes && c[k] >= 0 && (uint64_t)c[k] < nodes;
      bad = bad || (live && !ok);
      const uint32_t rr = ok ? (uint32_t)r[k] : BNONE, cc = ok ? (uint32_t)c[k] : BNONE;
      const uint32_t mn = boba_run_min(rr, cc);
      const uint32_t prev = (uint32_t)__shfl_up((int)rr, 1, 64);
      if (ok && (lane == 0 || prev != rr) && key[rr] > mn) atomicMin(&key[rr], mn);
      if (ok && !seen[cc]) seen[cc] = 1;
    }
  }
  if (bad) *err = 1;
}

__global__ __launch_bounds__(BT) void k_boba_keys(uint32_t *key, const unsigned char *__restrict__ seen, uint32_t nodes,
                                                  uint32_t *__restrict__ val) {
  for (int64_t v = (int64_t)blockIdx.x * BT + threadIdx.x; v < nodes; v += (int64_t)gridDim.x * BT) {
    const uint32_t k = key[v];
    key[v] = k != BNONE ? k : seen[v] ? nodes : nodes + 1;
    val[v] = (uint32_t)v;
  }
}

template <typename I>
__global__ __launch_bounds__(BT) void k_boba_scatter(const uint32_t *__restrict__ sorted_v, uint32_t nodes,
                                                     const int *__restrict__ err, I *__restrict__ inv) {
  if (*err) return;
  for (int64_t p = (int64_t)blockIdx.x * BT + threadIdx.x; p < nodes; p += (int64_t)gridDim.x * BT)
    inv[sorted_v[p]] = (I)p;
}

template <typename I>
static int boba_typed(sbx_handle_t h, int64_t nodes64, int64_t nnz, const void *row, const void *col, void *inv_out) {
  SBX_TRY(sbx_arena_begin(h));
  const uint32_t nodes = (uint32_t)nodes64;
  uint32_t *ka = nullptr, *kb = nullptr, *va = nullptr, *vb = nullptr;
  unsigned char *seen = nullptr;
  int *err = nullptr;
  SBX_TRY(sbx_salloc(h, 1, &err));
  SBX_TRY(sbx_salloc(h, nodes, &ka));
  SBX_TRY(sbx_salloc(h, nodes, &kb));
  SBX_TRY(sbx_salloc(h, nodes, &va));
  SBX_TRY(sbx_salloc(h, nodes, &vb));
  SBX_TRY(sbx_salloc(h, nodes, &seen));
  SBX_HIP(h, hipMemsetAsync(err, 0, sizeof(int), h->stream));
  SBX_HIP(h, hipMemsetAsync(ka, 0xFF, (size_t)nodes * sizeof(uint32_t), h->stream));
  SBX_HIP(h, hipMemsetAsync(seen, 0, nodes, h->stream));
  const int64_t cap = (int64_t)h->num_cus * 16;
  if (nnz > 0)
    SBX_KLAUNCH(h, SBX_K_MISC, k_boba_entries<I>, dim3(sbx_grid_for((nnz + 64 * BITEMS - 1) / (64 * BITEMS), BT / 64, cap)),
                dim3(BT), (const I *)row, (const I *)col, nnz, nodes, ka, seen, err);
  SBX_KLAUNCH(h, SBX_K_MISC, k_boba_keys, dim3(sbx_grid_for(nodes, BT, cap)), dim3(BT), ka, (const unsigned char *)seen,
              nodes, va);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_sort_pairs(h, &ka, &kb, &va, &vb, nodes, 0, sbx_bits_for((uint64_t)nodes + 1)));
  SBX_KLAUNCH(h, SBX_K_MISC, k_boba_scatter<I>, dim3(sbx_grid_for(nodes, BT, cap)), dim3(BT), (const uint32_t *)va, nodes,
              (const int *)err, (I *)inv_out);
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_MISC, (int64_t)2 * sizeof(I) * nnz + (int64_t)(14 + sizeof(I)) * nodes);
  int bad = 0;
  SBX_TRY(sbx_readback(h, &bad, err, sizeof(bad)));
  if (bad) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbx_boba_reorder: an id outside [0, max(n, m))");
  return SBX_OK;
}

}  // namespace

extern "C" int sbx_boba_reorder(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t m, int64_t nnz, const void *row,
                                const void *col, void *inv_perm_out) {
  if (!h) return SBX_ERR_BAD_ARG;
  const int64_t nodes = n > m ? n : m;
  SBX_REQUIRE(h, n >= 0 && m >= 0 && nnz >= 0 && (nodes > 0 || nnz == 0) && (nodes == 0 || inv_perm_out) &&
                     (nnz == 0 || (row && col)), "bad argument");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  if (nodes >= ((int64_t)1 << 31)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: max(n, m) >= 2^31", __func__);
  if (nodes == 0) return SBX_OK;
  if (it == SBX_I64) return boba_typed<int64_t>(h, nodes, nnz, row, col, inv_perm_out);
  return boba_typed<int32_t>(h, nodes, nnz, row, col, inv_perm_out);  // SBX_I32 and SBX_I32_N64: no offset array
}
