// sbx_gray_order.hip — sbx_gray_reorder: GrayReorder with its ordering stage on the device (opt-in, stable ties).
//
//   A8  reorder/gray_reorder.cc:106-424
//
// The reference orders the row keys with unstable std::sort calls on heavily tied keys (:199-203 by degree, :293-301 and
// :354-360 the sections by decoded key — ascending and descending in turn —, :404 the dense rows), so its output depends
// on libstdc++'s introsort; the host layer's GrayReorder therefore issues those very calls over the device-computed keys
// (exact mode, the default: DESIGN.md section 5).  This entry point is the other mode SURVEY section 8(b) sketches
// (`exact_ties = 0`): every one of those sorts as a STABLE sort, which makes the whole ordering one lexicographic order
//
//     (class, section, +-key, degree, row id)         class: sparse rows (degree <= nnz_threshold) in front of dense ones
//
// and that is what three stable radix sorts of (key, row id) pairs produce, last criterion first: by degree, by the
// signed key, by (class, section).  Sections are what the reference's walk over the degree-sorted sparse rows finds
// (:271-329): empty rows in front, then runs of `group_size` distinct degrees; section k sorts ascending for even k and
// descending for odd k (a descending stable sort is an ascending one on the complemented key).  A "highly banded" class
// (:181-190) keeps the reference's early-outs: sparse rows by degree only, dense rows in their original order.
// Wherever the reference's comparators decide the order — no two rows of a section with equal keys — the result is the
// reference's; among tied rows it is the stable order instead of introsort's.
//
// ONE sort where the criteria fit one word (round 6): class / section, signed key and degree are fields of a single
// 64-bit key built in row order — no gathers through a half-sorted id list between the sorts, one histogram, one
// read-back less (the number of sections only sizes the class field: its bound, ceil(threshold / group_size), does) —
// and (key, row id) pairs go through the radix sort once: five 8-bit passes for the bench line's parameters (3 + 32 + 4
// bits) where the three sorts took six, with three histograms and three gather kernels around them.  Parameters whose
// fields need more than 64 bits (resolution 64; a threshold in the millions) keep the three sorts.
#include "sbx_device.h"
#include "sbx_internal.h"

namespace {

// pass 1: (degree key, row id) pairs — the dense rows' degree is no criterion — and the degrees the sparse rows have
template <typename I>
__global__ __launch_bounds__(256) void k_go_degree_keys(const I *__restrict__ deg, int64_t n, int64_t thr,
                                                        uint32_t *__restrict__ key, uint32_t *__restrict__ id,
                                                        uint32_t *__restrict__ present) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t d = (int64_t)deg[i];
    const bool sparse = d <= thr;
    key[i] = sparse ? (uint32_t)d : 0u;
    id[i] = (uint32_t)i;
    if (sparse && d > 0 && present[d] == 0) present[d] = 1;  // (a benign race: every writer stores 1)
  }
}

// section of a sparse degree d >= 1: 1 + (number of smaller degrees present) / group_size  (0: the empty rows);
// `rank` = exclusive scan of `present`
__global__ __launch_bounds__(256) void k_go_sections(const uint32_t *__restrict__ present, const uint32_t *__restrict__ rank,
                                                     int64_t count, uint32_t group_size, uint32_t *__restrict__ section) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= count) return;
  section[d] = (d > 0 && present[d]) ? 1u + rank[d] / group_size : 0u;
}

// pass 2: the signed key of the row at every position of the degree-sorted list
template <typename I>
__global__ __launch_bounds__(256) void k_go_signed_keys(const uint32_t *__restrict__ id, const I *__restrict__ deg,
                                                        const uint64_t *__restrict__ gkey, int64_t n, int64_t thr,
                                                        const uint32_t *__restrict__ section, int sparse_banded,
                                                        int dense_banded, uint64_t mask, uint64_t *__restrict__ key) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; p < n; p += stride) {
    const uint32_t r = id[p];
    const int64_t d = (int64_t)deg[r];
    uint64_t k = 0;
    if (d > thr) {
      if (!dense_banded) k = gkey[r] & mask;
    } else if (d > 0 && !sparse_banded) {
      const uint32_t s = section[d] - 1u;  // index of the section's sort call
      k = (s & 1u) ? (~gkey[r]) & mask : gkey[r] & mask;
    }
    key[p] = k;
  }
}

// pass 3: (class, section)
template <typename I>
__global__ __launch_bounds__(256) void k_go_class_keys(const uint32_t *__restrict__ id, const I *__restrict__ deg,
                                                       int64_t n, int64_t thr, const uint32_t *__restrict__ section,
                                                       int sparse_banded, uint32_t dense_class,
                                                       uint32_t *__restrict__ key) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; p < n; p += stride) {
    const int64_t d = (int64_t)deg[id[p]];
    key[p] = d > thr ? dense_class : (sparse_banded ? 0u : section[d]);
  }
}

template <typename I>
__global__ __launch_bounds__(256) void k_go_emit(const uint32_t *__restrict__ id, int64_t n, I *__restrict__ inv) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; p < n; p += stride) inv[id[p]] = (I)p;
}

// the degrees the sparse rows have (the one-sort path: the sections must be known before any key is built)
template <typename I>
__global__ __launch_bounds__(256) void k_go_present(const I *__restrict__ deg, int64_t n, int64_t thr,
                                                    uint32_t *__restrict__ present) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t d = (int64_t)deg[i];
    if (d <= thr && d > 0 && present[d] == 0) present[d] = 1;  // (a benign race: every writer stores 1)
  }
}

// one key per row, in row order: class / section << (kbits + dbits) | signed key << dbits | degree (sparse rows)
template <typename I>
__global__ __launch_bounds__(256) void k_go_composite(const I *__restrict__ deg, const uint64_t *__restrict__ gkey, int64_t n,
                                                      int64_t thr, const uint32_t *__restrict__ section, int sparse_banded,
                                                      int dense_banded, uint64_t mask, uint32_t dense_class, int kbits,
                                                      int dbits, int idbits, uint64_t *__restrict__ key,
                                                      uint32_t *__restrict__ id) {
  // id == nullptr: the row id is the key's low field (idbits wide) and the sort has no payload
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t d = (int64_t)deg[i];
    uint64_t cls, k = 0, dk = 0;
    if (d > thr) {
      cls = dense_class;
      if (!dense_banded) k = gkey[i] & mask;
    } else {
      const uint32_t sec = sparse_banded ? 0u : section[d];
      cls = sec;
      dk = (uint64_t)d;
      if (d > 0 && !sparse_banded) k = ((sec - 1u) & 1u) ? (~gkey[i]) & mask : gkey[i] & mask;
    }
    if (kbits == 0) k = 0;  // (both classes "highly banded": the keys are no criterion)
    const uint64_t comp = (cls << (kbits + dbits)) | (k << dbits) | dk;
    if (id) {
      key[i] = comp;
      id[i] = (uint32_t)i;
    } else {
      key[i] = (comp << idbits) | (uint64_t)i;
    }
  }
}

template <typename I>
__global__ __launch_bounds__(256) void k_go_widen(const uint32_t *__restrict__ in, int64_t n, I *__restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = (I)in[i];
}

// What both forms of a call read: the entry point's six, what gray_order_typed derives once, gray_order_scratch's buffers
template <typename I>
struct GrayOrderCall {
  sbx_handle_t h;
  int64_t n, nnz;
  const I *deg;
  const uint64_t *gkey;
  I *inv_out;
  int sparse_banded, dense_banded;  // 1: a "highly banded" class (gray_reorder.cc:181-190)
  int64_t thr, dmax;                // the nnz threshold (-1: no row is sparse); the largest degree a sparse row can have
  uint32_t gs, grid;                // distinct degrees per section: the group size, at least 1; grid of the kernels over the rows
  int bits;                         // of a key, and `mask` with those bits set
  uint64_t mask, *qa, *qb;          // scratch: 64-bit key buffers of n,
  uint32_t *ia, *ib, *present, *rank, *section;  // id buffers of n, degree tables of dmax + 2
};

// `sections`: the call finds the degrees' sections (`present` zeroed for the kernel that fills it); else `section` zeroed
template <typename I>
int gray_order_scratch(GrayOrderCall<I> &c, bool sections) {
  const size_t n = (size_t)c.n, nd = (size_t)c.dmax + 2;
  SBX_TRY(sbx_salloc(c.h, n, &c.ia));
  SBX_TRY(sbx_salloc(c.h, n, &c.ib));
  SBX_TRY(sbx_salloc(c.h, n, &c.qa));
  SBX_TRY(sbx_salloc(c.h, n, &c.qb));
  SBX_TRY(sbx_salloc(c.h, nd, &c.section));
  if (sections) SBX_TRY(sbx_salloc(c.h, nd, &c.present));
  if (sections) SBX_TRY(sbx_salloc(c.h, nd, &c.rank));
  SBX_HIP(c.h, hipMemsetAsync(sections ? c.present : c.section, 0, sizeof(uint32_t) * nd, c.h->stream));
  return SBX_OK;
}
// present -> rank -> section; n_present != nullptr: the number of degrees present is read back on the way
template <typename I>
int gray_order_sections(const GrayOrderCall<I> &c, uint32_t *n_present) {
  uint32_t *tot = nullptr;
  if (n_present) SBX_TRY(sbx_salloc(c.h, 1, &tot));
  SBX_TRY(sbx_exclusive_scan_u32(c.h, c.present, c.rank, c.dmax + 1, tot));
  if (n_present) SBX_TRY(sbx_readback(c.h, n_present, tot, sizeof(uint32_t)));
  SBX_KLAUNCH(c.h, SBX_K_GRAY, k_go_sections, dim3((unsigned)((c.dmax + 1 + 255) / 256)), dim3(256),
              (const uint32_t *)c.present, (const uint32_t *)c.rank, c.dmax + 1, c.gs, c.section);
  return SBX_OK;
}

// one sort of composite keys: cbits of class / section (dense_class: the dense rows'), kbits of signed key, dbits of degree
template <typename I>
int gray_order_one_sort(GrayOrderCall<I> &c, int cbits, int kbits, int dbits, uint32_t dense_class) {
  sbx_handle_t h = c.h;
  const int64_t n = c.n;
  const bool sections = !c.sparse_banded && c.dmax > 0;  // (a "highly banded" sparse class has none)
  SBX_TRY(gray_order_scratch(c, sections));
  if (sections) {
    SBX_KLAUNCH(h, SBX_K_GRAY, k_go_present<I>, dim3(c.grid), dim3(256), c.deg, n, c.thr, c.present);
    SBX_TRY(gray_order_sections(c, nullptr));
  }
  sbx_radix_pass passes[16];
  // Where the row id fits below the criteria (bench line: 39 + 22 bits) it is the key's low field: the sort moves 8-byte
  // keys without a payload, and its last pass writes inv[id] = position itself (sbx_radix_emit::pos_of) — no emit kernel
  const int fit = sbx_bits_for((uint64_t)(n - 1)), idbits = cbits + kbits + dbits + fit <= 64 ? fit : 0;  // 0: a payload
  SBX_KLAUNCH(h, SBX_K_GRAY, k_go_composite<I>, dim3(c.grid), dim3(256), c.deg, c.gkey, n, c.thr, (const uint32_t *)c.section,
              c.sparse_banded, c.dense_banded, c.mask, dense_class, kbits, dbits, idbits, c.qa, idbits ? (uint32_t *)nullptr : c.ia);
  SBX_LAUNCH_CHECK(h);
  const int np = sbx_radix_plan(idbits, idbits + cbits + kbits + dbits, 0, 0, passes);
  sbx_tied_hint_scope tied(h);  // (class and degree fields of a handful of values, Gray keys shared by many rows)
  if (idbits) {
    const sbx_radix_emit em = {nullptr, c.ia, nullptr, nullptr, sizeof(I) == 4 ? (unsigned *)c.inv_out : (unsigned *)c.ib,
                               idbits < 32 ? (1u << idbits) - 1u : 0u};
    SBX_TRY(sbx_radix_sort_emit(h, c.qa, c.qb, n, passes, np, &em));
    if (sizeof(I) != 4)
      SBX_KLAUNCH(h, SBX_K_GRAY, k_go_widen<I>, dim3(c.grid), dim3(256), (const uint32_t *)c.ib, n, c.inv_out);
  } else {
    int in_b = 0;
    SBX_TRY(sbx_radix_sort(h, 8, 4, c.qa, c.qb, c.ia, c.ib, n, passes, np, &in_b));
    SBX_KLAUNCH(h, SBX_K_GRAY, k_go_emit<I>, dim3(c.grid), dim3(256), (const uint32_t *)(in_b ? c.ib : c.ia), n, c.inv_out);
  }
  SBX_LAUNCH_CHECK(h);
  return SBX_OK;
}

// three stable sorts of (key, row id) pairs, last criterion first
template <typename I>
int gray_order_three_sorts(GrayOrderCall<I> &c) {
  sbx_handle_t h = c.h;
  const int64_t n = c.n;
  uint32_t *ka = nullptr, *kb = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)n, &ka));
  SBX_TRY(sbx_salloc(h, (size_t)n, &kb));
  SBX_TRY(gray_order_scratch(c, true));
  // 1: by degree (sparse rows; stable: ids ascending inside a degree)
  SBX_KLAUNCH(h, SBX_K_GRAY, k_go_degree_keys<I>, dim3(c.grid), dim3(256), c.deg, n, c.thr, ka, c.ia, c.present);
  SBX_LAUNCH_CHECK(h);
  uint32_t *id = c.ia, *id_tmp = c.ib;
  SBX_TRY(sbx_sort_pairs(h, &ka, &kb, &id, &id_tmp, n, 0, sbx_bits_for((uint64_t)c.dmax)));
  uint32_t n_present = 0;
  SBX_TRY(gray_order_sections(c, &n_present));  // the sections of the degrees
  const uint32_t n_sections = c.sparse_banded ? 0u : (n_present + c.gs - 1u) / c.gs;
  // 2: by the signed key
  if (!(c.sparse_banded && c.dense_banded)) {
    SBX_KLAUNCH(h, SBX_K_GRAY, k_go_signed_keys<I>, dim3(c.grid), dim3(256), (const uint32_t *)id, c.deg, c.gkey, n, c.thr,
                (const uint32_t *)c.section, c.sparse_banded, c.dense_banded, c.mask, c.qa);
    SBX_LAUNCH_CHECK(h);
    SBX_TRY(sbx_sort_pairs(h, &c.qa, &c.qb, &id, &id_tmp, n, 0, c.bits));
  }
  // 3: by (class, section)
  const uint32_t dense_class = n_sections + 1u;
  SBX_KLAUNCH(h, SBX_K_GRAY, k_go_class_keys<I>, dim3(c.grid), dim3(256), (const uint32_t *)id, c.deg, n, c.thr,
              (const uint32_t *)c.section, c.sparse_banded, dense_class, ka);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_sort_pairs(h, &ka, &kb, &id, &id_tmp, n, 0, sbx_bits_for((uint64_t)dense_class)));
  SBX_KLAUNCH(h, SBX_K_GRAY, k_go_emit<I>, dim3(c.grid), dim3(256), (const uint32_t *)id, n, c.inv_out);
  SBX_LAUNCH_CHECK(h);
  return SBX_OK;
}

template <typename I>
int gray_order_typed(GrayOrderCall<I> c, const int64_t *counts, int bits, int64_t thr, int group_size) {
  // gray_reorder.cc:181-190 (the reference keeps the counters in `int`)
  c.sparse_banded = double((int)counts[1]) / (int)counts[0] > 0.3;
  c.dense_banded = double((int)counts[3]) / (int)counts[2] > 0.2;
  c.thr = thr < 0 ? -1 : thr;
  // a sparse row's degree is at most the threshold (and, without duplicate columns, m; the tables cover min(threshold, nnz))
  c.dmax = thr < 0 ? 0 : (thr < c.nnz ? thr : c.nnz);
  if (c.dmax > ((int64_t)1 << 28))
    SBX_FAIL(c.h, SBX_ERR_UNSUPPORTED, "sbx_gray_reorder: nnz_threshold %lld: the degree tables would need %lld entries",
             (long long)c.thr, (long long)c.dmax);
  c.gs = (uint32_t)(group_size > 0 ? group_size : 1);
  c.bits = bits, c.mask = bits >= 64 ? ~0ull : ((1ull << bits) - 1ull);
  c.grid = sbx_grid_for(c.n, 256, (int64_t)c.h->num_cus * 16);
  // the one-sort form: do the three fields fit a word?  (at most dmax degrees are present: that many sections at most)
  const uint32_t dense_class = c.sparse_banded ? 1u : (uint32_t)((c.dmax + c.gs - 1) / c.gs) + 1u;
  const int cbits = sbx_bits_for((uint64_t)dense_class), dbits = sbx_bits_for((uint64_t)c.dmax);
  const int kbits = (c.sparse_banded && c.dense_banded) ? 0 : bits;
  if (cbits + kbits + dbits <= 64 && !sbx_sw().gray_three_sorts) return gray_order_one_sort(c, cbits, kbits, dbits, dense_class);
  return gray_order_three_sorts(c);
}

}  // namespace

extern "C" int sbx_gray_reorder(sbx_handle_t h, sbx_index_type it, int64_t n, int64_t m, int64_t nnz,
                                const void *row_ptr, const void *col, int resolution, int nnz_threshold,
                                int group_size, int exact_ties, void *inv_perm_out) {
  if (!h) return SBX_ERR_BAD_ARG;
  if (it == SBX_I32_N64)
    return sbx_mixed_gray_reorder(h, n, m, nnz, row_ptr, col, resolution, nnz_threshold, group_size, exact_ties, inv_perm_out);
  if (n < 0 || m < 0 || !row_ptr || (n > 0 && !inv_perm_out) || (nnz > 0 && !col) || group_size < 1)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbx_gray_reorder: bad argument");
  if (exact_ties)
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED,
             "sbx_gray_reorder: the reference's tie order is libstdc++'s introsort visiting order and is reproduced by "
             "the host layer (reorder::GrayReorder over sbx_gray_row_keys); this entry point orders ties stably");
  if (n >= ((int64_t)1 << 32)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbx_gray_reorder: more than 2^32 rows");
  SBX_TRY(sbx_arena_begin(h));
  if (n == 0) return SBX_OK;
  if (n == 1) {
    SBX_HIP(h, hipMemsetAsync(inv_perm_out, 0, it == SBX_I64 ? 8 : 4, h->stream));
    return SBX_OK;
  }
  NestGuard guard(h);
  void *deg = nullptr;
  uint64_t *gkey = nullptr;
  SBX_TRY(sbx_arena_alloc(h, (size_t)n * (it == SBX_I64 ? 8 : 4), &deg));
  SBX_TRY(sbx_salloc(h, (size_t)n, &gkey));
  int64_t counts[4] = {0, 0, 0, 0};
  SBX_TRY(sbx_gray_row_keys(h, it, n, m, nnz, row_ptr, col, resolution, nnz_threshold, deg, gkey, counts));
  const int bits = sbx_gray_bits(resolution, m), thr = nnz_threshold;
  if (it == SBX_I64)
    return gray_order_typed<int64_t>({h, n, nnz, (const int64_t *)deg, gkey, (int64_t *)inv_perm_out}, counts, bits, thr, group_size);
  return gray_order_typed<int32_t>({h, n, nnz, (const int32_t *)deg, gkey, (int32_t *)inv_perm_out}, counts, bits, thr, group_size);
}
