// sbx_spmm.hip — Y = A X of a CSR matrix and a dense row-major block of k columns, deterministic, balanced over the stored
// entries (include/sbmm.h).  Rows, columns and positions are 64-bit inside; the arrays are read at the width
// of their index tuple.
//
// The lanes of a wave lie on the columns of X, not on the entries: an entry's row of X is one coalesced load.
//
//   zero     Y[i, 0:k] = 0 (a memset where ldy == k): a row without entries is never touched again
//   spans    first[t] = the row of entry t * MM_SPAN (k_tile_first_rows of sbx_device.h, as the SpMV)
//   span     one wave per span of MM_SPAN consecutive entries and per block of columns.  A lane holds VEC columns (16 bytes
//            where x, y, ldx, ldy and k allow it, else one value); a GROUP of G lanes covers the block's G * VEC columns,
//            and the wave holds NG = 64 / G groups.  The span is cut into NG equal runs of consecutive entries, one per
//            group (NG == 1, the wide form: the whole span; else whole 8s).  A group walks its run in batches: its lanes
//            load a batch's columns, values and rows (a search in row_ptr between first[t] and first[t + 1], and one more
//            wherever a row ends) coalesced, one entry per lane in the wide form and MM_ITEMS consecutive entries per lane
//            (sbx_load_items8) in a group; then the batch's entries are broadcast one by one (the wide form: v_readlane into
//            scalar registers, the row of X addressed from them; else ds_bpermute inside the group), MM_INFLIGHT rows of
//            X loaded before the first is added.  A group adds its products entry by entry; where the row changes, the
//            sum so far is a row complete in this group and goes to Y — except the group's first, which is kept (the
//            head), and its last (the tail).  The tails enter a segmented scan over the groups (keyed by row: a fixed
//            tree of __shfl_up at a stride of G lanes), which closes the rows that cross groups, and a head is added
//            to what the groups before it hold of its row.  The span's LAST sum never goes to Y: (row, k sums) goes to
//            the carry arrays.
//   carry    one thread per span and column: where a span's carry row differs from the span before, the carries of that
//            row are added in span order and then the part of the row that a span wrote to Y (or the 0 of `zero`).
// Every Y[i, j] is written once per kernel at most, every sum has an order fixed by the positions of the entries and by
// k: no atomics, the same bits on every call, and the same order for every column j.
// Malformed input: a column outside [0, m) gives a product of 0 without a load; every row a search returns lies between
// first[t] and first[t + 1], both in [0, n - 1], whatever row_ptr holds; carries are indexed by span.
#include <cstddef>

#include "sbmm.h"
#include "sbmt.h"
#include "sbmv.h"
#include "sbx_device.h"
#include "sbx_internal.h"

#ifndef MM_SPAN
#define MM_SPAN 2048  // stored entries per wave (and per partial row of the scratch); sbmm.h states the scratch with it
#endif
#ifndef MM_ITEMS
#define MM_ITEMS 8  // consecutive entries a lane of a group loads per batch: sbx_load_items8 is written for 8
#endif
#ifndef MM_INFLIGHT
#define MM_INFLIGHT 4  // rows of X a group has in flight before the first is added
#endif

namespace {

constexpr int MM = 256;  // threads per workgroup of the helper kernels (the span kernel runs one wave per workgroup)
static_assert(MM_SPAN % 64 == 0 && MM_SPAN >= 1024, "sbmm.h: a partial row per span of at least 1024 entries");
static_assert(MM_ITEMS == 8, "sbx_load_items8 and sbx_load_values8 load eight entries");
static_assert(64 % MM_INFLIGHT == 0 && MM_ITEMS % MM_INFLIGHT == 0, "whole rounds of loads");

template <typename V, int VEC>
struct alignas(sizeof(V) * VEC) MmVec {
  V a[VEC];
};

// the value of lane `src`: the wide form reads it into scalar registers (src is wave-uniform), the narrow one permutes
template <bool WIDE, typename T>
__device__ __forceinline__ T mm_bcast(T x, int src) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "4- and 8-byte types");
  if constexpr (sizeof(T) == 4) {
    const int b = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(T, WIDE ? __builtin_amdgcn_readlane(b, src) : __shfl(b, src, 64));
  } else {
    const uint64_t b = __builtin_bit_cast(uint64_t, x);
    if constexpr (WIDE) {
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, src);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), src);
      return __builtin_bit_cast(T, ((uint64_t)hi << 32) | lo);
    } else {
      return __builtin_bit_cast(T, (uint64_t)__shfl((unsigned long long)b, src, 64));
    }
  }
}

template <typename T>
__device__ __forceinline__ T mm_up(T x, int delta) {  // lane i gets lane i - delta's value (its own below delta)
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(T, __shfl_up(__builtin_bit_cast(int, x), (unsigned)delta, 64));
  } else {
    return __builtin_bit_cast(T, (uint64_t)__shfl_up((unsigned long long)__builtin_bit_cast(uint64_t, x), (unsigned)delta, 64));
  }
}

template <typename V>
__global__ __launch_bounds__(MM) void k_spmm_zero(V *__restrict__ y, int64_t ldy, int64_t k, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * MM + threadIdx.x;
  if (i >= total) return;
  const int64_t r = i / k;
  y[r * ldy + (i - r * k)] = (V)0;
}

// PERM (the transposed product of sbmt.h, where rp / col are the plan's col_ptr / row): entry p's value is val[perm[p]].
// A lane loads its positions of perm as it loads its columns and issues all its gathers from val before the first is
// used; a position outside [0, nnz) is never loaded through and its entry contributes nothing, as a column outside
// [0, m) does.  Nothing else differs: the sums and their order are those of PERM == false on the gathered values.
template <typename I, typename N, typename V, int VEC, bool WIDE, bool PERM>
__global__ __launch_bounds__(64) void k_spmm_span(const N *__restrict__ rp, const I *__restrict__ col,
                                                  const N *__restrict__ perm, const V *__restrict__ val,
                                                  const V *__restrict__ x, int64_t ldx, int64_t m,
                                                  int64_t nnz, int64_t k, int G, bool col_vec, bool val_vec,
                                                  const int64_t *__restrict__ first,
                                                  V *__restrict__ y, int64_t ldy, int64_t *__restrict__ trow,
                                                  V *__restrict__ tsum) {
  using Vec = MmVec<V, VEC>;
  constexpr int E = WIDE ? 1 : MM_ITEMS;  // consecutive entries a lane loads per batch
  const int lane = sbx_lane();
  const int NG = WIDE ? 1 : 64 / G;   // groups in the wave
  const int LP = WIDE ? 64 : G;       // lanes that load a batch: the group's (the wide form: the wave's)
  const int B = LP * E;               // entries of a batch
  const int u = WIDE ? 0 : lane / G;  // this lane's group; u == NG: the lanes left over, which carry nothing
  const int l = lane - u * G;
  const int ubase = u * G;
  const bool live = u < NG;
  const int64_t t = blockIdx.x;
  const int64_t t0 = t * MM_SPAN, t1 = t0 + MM_SPAN < nnz ? t0 + MM_SPAN : nnz;
  const int chunk = ((MM_SPAN + NG - 1) / NG + 7) & ~7;  // entries of a group's run: whole 8s, so a lane's 8 stay aligned
  const int batches = (chunk + B - 1) / B;
  const int64_t u0 = t0 + (int64_t)u * chunk;
  const int64_t u1 = u0 + chunk < t1 ? u0 + chunk : t1;  // (u1 <= u0: a run past the span's end, nothing valid in it)
  const int64_t r0 = first[t];
  const int64_t r1 = first[t + 1] < r0 ? r0 : first[t + 1];
  const int64_t j0 = ((int64_t)blockIdx.y * G + l) * VEC;  // this lane's first column
  const bool colok = live && l < G && j0 < k;             // (VEC > 1 only where k % VEC == 0: the whole vector is inside)

  V acc[VEC], head[VEC];
#pragma unroll
  for (int e = 0; e < VEC; e++) acc[e] = head[e] = (V)0;  // (a sum begins at +0: an exact zero never comes out as -0)
  int64_t cur = -1, hr = -1;  // the row of the running sum; the row of the group's first entry
  bool multi = false;         // the row has changed inside this group: `head` holds the first sum

  for (int b = 0; b < batches; b++) {
    // E consecutive entries per lane: a slot past the run's end repeats the run's (or the span's) last entry and
    // contributes nothing.  All of [t0, t1) is inside the arrays, and u1 - 1 >= t0 as t1 > t0.
    const int64_t p0 = u0 + (int64_t)b * B + (int64_t)l * E;
    I c[E];
    V v[E];
    int64_t r[E];
    bool pok[E];  // (PERM: the entry's position in val lies inside the array)
#pragma unroll
    for (int e = 0; e < E; e++) pok[e] = true;
    if constexpr (WIDE) {
      const int64_t pc = p0 < u1 ? p0 : u1 - 1;
      c[0] = col[pc];
      if constexpr (PERM) {
        const int64_t pp = (int64_t)perm[pc];
        pok[0] = p0 < u1 && (uint64_t)pp < (uint64_t)nnz;
        v[0] = (V)0;
        if (pok[0]) v[0] = val[pp];
      } else {
        v[0] = val ? val[pc] : (V)1;
      }
      r[0] = r0 == r1 ? r0 : sbx_row_of(rp, pc, r0, r1);
    } else {
      sbx_load_items8(col, p0, u1, col_vec, c);
      if constexpr (PERM) {
        N pm[E];
        sbx_load_items8(perm, p0, u1, val_vec, pm);  // (val_vec: perm's alignment here)
#pragma unroll
        for (int e = 0; e < E; e++) {
          pok[e] = p0 + e < u1 && (uint64_t)(int64_t)pm[e] < (uint64_t)nnz;
          v[e] = (V)0;
        }
#pragma unroll
        for (int e = 0; e < E; e++)  // the lane's gathers, all in flight before the first value is used
          if (pok[e]) v[e] = val[(int64_t)pm[e]];
      } else if (val) {
        sbx_load_values8(val, p0, u1, val_vec, v);
      } else {
#pragma unroll
        for (int e = 0; e < E; e++) v[e] = (V)1;
      }
      // the rows: a search for the lane's first entry, then one more wherever an entry reaches the end of the row
      int64_t rr = r0 == r1 ? r0 : sbx_row_of(rp, p0 < u1 ? p0 : u1 - 1, r0, r1);
      int64_t row_end = rr < r1 ? (int64_t)rp[rr + 1] : INT64_MAX;
      r[0] = rr;
#pragma unroll
      for (int e = 1; e < E; e++) {
        if (p0 + e < u1 && p0 + e >= row_end) {
          if (rr < r1) rr = sbx_row_of(rp, p0 + e, rr, r1);
          row_end = rr < r1 ? (int64_t)rp[rr + 1] : INT64_MAX;
        }
        r[e] = rr;
      }
    }
#pragma unroll
    for (int e = 0; e < E; e++)
      if (!(live && p0 + e < u1 && pok[e] && (uint64_t)(int64_t)c[e] < (uint64_t)m)) c[e] = (I)-1;

    // the batch's entries in order: lane by lane, and a lane's E entries in turn; MM_INFLIGHT rows of X in flight
    for (int lp = 0; lp < LP; lp += WIDE ? MM_INFLIGHT : 1) {
#pragma unroll
      for (int e0 = 0; e0 < E; e0 += WIDE ? 1 : MM_INFLIGHT) {
        I cc[MM_INFLIGHT];
        V vv[MM_INFLIGHT];
        int64_t rr[MM_INFLIGHT];
        Vec xv[MM_INFLIGHT];
#pragma unroll
        for (int s = 0; s < MM_INFLIGHT; s++) {
          const int src = ubase + lp + (WIDE ? s : 0), e = WIDE ? 0 : e0 + s;
          cc[s] = mm_bcast<WIDE>(c[e], src);
          vv[s] = val ? mm_bcast<WIDE>(v[e], src) : (V)1;
          rr[s] = mm_bcast<WIDE>(r[e], src);
#pragma unroll
          for (int q = 0; q < VEC; q++) xv[s].a[q] = (V)0;
          if (colok && cc[s] >= 0) xv[s] = *(const Vec *)(x + (int64_t)cc[s] * ldx + j0);
        }
#pragma unroll
        for (int s = 0; s < MM_INFLIGHT; s++) {
          if (rr[s] != cur) {  // the row changes: what was added so far is a row complete in this group
            if (cur < 0) {
              hr = rr[s];
            } else if (!multi) {
              multi = true;
#pragma unroll
              for (int q = 0; q < VEC; q++) head[q] = acc[q];
            } else if (colok) {
              Vec o;
#pragma unroll
              for (int q = 0; q < VEC; q++) o.a[q] = acc[q];
              *(Vec *)(y + cur * ldy + j0) = o;
            }
            cur = rr[s];
#pragma unroll
            for (int q = 0; q < VEC; q++) acc[q] = (V)0;
          }
          const bool ok = colok && cc[s] >= 0;
#pragma unroll
          for (int q = 0; q < VEC; q++) acc[q] = ok ? (V)(acc[q] + vv[s] * xv[s].a[q]) : acc[q];
        }
      }
    }
  }

  // segmented inclusive scan of the tails over the groups; a segment begins where a row does
  const int64_t tr = cur;
  int64_t prev_tr = -1, next_hr = -1;
  V before[VEC];
#pragma unroll
  for (int e = 0; e < VEC; e++) before[e] = (V)0;
  if constexpr (!WIDE) {
    prev_tr = mm_up(tr, G);
    bool f = multi || u == 0 || prev_tr != hr;
    for (int d = 1; d < NG; d <<= 1) {
      V o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; e++) o[e] = mm_up(acc[e], d * G);
      const int of = mm_up((int)f, d * G);
      if (u >= d && !f) {
#pragma unroll
        for (int e = 0; e < VEC; e++) acc[e] = o[e] + acc[e];
        f = of != 0;
      }
    }
#pragma unroll
    for (int e = 0; e < VEC; e++) before[e] = mm_up(acc[e], G);
    next_hr = __builtin_bit_cast(int64_t, (uint64_t)__shfl_down((unsigned long long)hr, (unsigned)G, 64));
  }

  if (multi && colok) {  // the first row ended here: what the groups before added to it, then this group's part
    const bool joined = u > 0 && prev_tr == hr;
    Vec o;
#pragma unroll
    for (int e = 0; e < VEC; e++) o.a[e] = (joined ? before[e] : (V)0) + head[e];
    *(Vec *)(y + hr * ldy + j0) = o;
  }
  Vec o;
#pragma unroll
  for (int e = 0; e < VEC; e++) o.a[e] = acc[e];
  if (u == NG - 1) {  // the span's last sum: to the carry arrays, whether or not the row ends here
    if (colok) *(Vec *)(tsum + t * k + j0) = o;
    if (blockIdx.y == 0 && l == 0) trow[t] = tr;
  } else if (colok && next_hr != tr) {
    *(Vec *)(y + tr * ldy + j0) = o;
  }
}

// the carries of one row and column, in span order, then what a span wrote to Y for that row (its end) or the 0 of `zero`
template <typename V>
__global__ __launch_bounds__(MM) void k_spmm_carry(const int64_t *__restrict__ trow, const V *__restrict__ tsum,
                                                   int64_t spans, int64_t k, V *__restrict__ y, int64_t ldy) {
  const int64_t i = (int64_t)blockIdx.x * MM + threadIdx.x;
  if (i >= spans * k) return;
  const int64_t t = i / k, j = i - t * k;
  const int64_t r = trow[t];
  if (t > 0 && trow[t - 1] == r) return;
  V s = (V)0;
  for (int64_t w = t; w < spans && trow[w] == r; w++) s = s + tsum[w * k + j];
  y[r * ldy + j] = s + y[r * ldy + j];
}

// perm != nullptr (with val): the transposed product of sbmt.h on the plan's arrays, profiled as its own kernel group
template <typename I, typename N, typename V>
static int mm_spmm(sbx_handle_t h, int64_t n, int64_t m, int64_t nnz, int64_t k, const void *row_ptr, const void *col,
                   const void *val, const void *x, int64_t ldx, void *y, int64_t ldy, const void *perm = nullptr,
                   int kid = SBX_K_SPMM) {
  SBX_HIP(h, hipSetDevice(h->device));
  if (ldy == k) {
    SBX_HIP(h, hipMemsetAsync(y, 0, (size_t)n * (size_t)k * sizeof(V), h->stream));
  } else {
    SBX_KLAUNCH(h, kid, (k_spmm_zero<V>), dim3((unsigned)((n * k + MM - 1) / MM)), dim3(MM), (V *)y, ldy, k, n * k);
  }
  if (nnz == 0) {  // (the same declaration as below with nnz = 0: the zero fill is the whole product)
    SBX_LAUNCH_CHECK(h);
    SBX_PROF_BYTES(h, kid, n * (int64_t)sizeof(N) + (m + n) * k * (int64_t)sizeof(V));
    return SBX_OK;
  }
  SBX_TRY(sbx_arena_begin(h));
  const int64_t spans = (nnz + MM_SPAN - 1) / MM_SPAN;
  int64_t *first = nullptr, *trow = nullptr;
  V *tsum = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)spans + 1, &first));
  SBX_TRY(sbx_salloc(h, (size_t)spans, &trow));
  SBX_TRY(sbx_salloc(h, (size_t)spans * (size_t)k, &tsum));
  SBX_KLAUNCH(h, kid, (k_tile_first_rows<N, MM_SPAN, MM>), dim3((unsigned)((spans + 1 + MM - 1) / MM)), dim3(MM),
              (const N *)row_ptr, n, spans, first);

  // 16 bytes of columns per lane where every row of X and Y begins on 16 bytes and k is whole vectors; else one column
  constexpr int W = 16 / (int)sizeof(V);
  const bool vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0 && ldx % W == 0 && ldy % W == 0 && k % W == 0;
  const int64_t lanes = vec ? k / W : k;         // lanes that cover the k columns
  const int64_t blocks = (lanes + 63) / 64;      // blocks of columns (the grid's second dimension; at most 2^14)
  const int G = (int)((lanes + blocks - 1) / blocks);  // lanes of a group: the blocks are equal up to one lane
  const dim3 grid((unsigned)spans, (unsigned)blocks);
  const bool gather = perm != nullptr && val != nullptr;  // (a pattern has nothing to gather: the plain kernel)
#define MM_LAUNCH_P(VEC, WIDE, PERM, VAL_VEC)                                                                          \
  SBX_KLAUNCH(h, kid, (k_spmm_span<I, N, V, VEC, WIDE, PERM>), grid, dim3(64), (const N *)row_ptr, (const I *)col,     \
              (const N *)perm, (const V *)val, (const V *)x, ldx, m, nnz, k, G, ((uintptr_t)col & 15) == 0, VAL_VEC,   \
              (const int64_t *)first, (V *)y, ldy, trow, tsum)
#define MM_LAUNCH(VEC, WIDE)                                                       \
  do {                                                                             \
    if (gather) MM_LAUNCH_P(VEC, WIDE, true, ((uintptr_t)perm & 15) == 0);         \
    else MM_LAUNCH_P(VEC, WIDE, false, ((uintptr_t)val & 15) == 0);                \
  } while (0)
  if (64 / G == 1) {
    if (vec) MM_LAUNCH(W, true); else MM_LAUNCH(1, true);
  } else {
    if (vec) MM_LAUNCH(W, false); else MM_LAUNCH(1, false);
  }
#undef MM_LAUNCH
#undef MM_LAUNCH_P
  SBX_KLAUNCH(h, kid, (k_spmm_carry<V>), dim3((unsigned)((spans * k + MM - 1) / MM)), dim3(MM),
              (const int64_t *)trow, (const V *)tsum, spans, k, (V *)y, ldy);
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, kid, nnz * (int64_t)(sizeof(I) + (val ? sizeof(V) : 0) + (gather ? sizeof(N) : 0)) + n * (int64_t)sizeof(N) +
                                    (m + n) * k * (int64_t)sizeof(V));
  return SBX_OK;
}

template <typename I, typename N>
static int mm_spmm_v(sbx_handle_t h, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, int64_t k, const void *row_ptr,
                     const void *col, const void *val, const void *x, int64_t ldx, void *y, int64_t ldy,
                     const void *perm = nullptr, int kid = SBX_K_SPMM) {
  switch (vt) {
    case SBX_V_F32: return mm_spmm<I, N, float>(h, n, m, nnz, k, row_ptr, col, val, x, ldx, y, ldy, perm, kid);
    case SBX_V_F64: return mm_spmm<I, N, double>(h, n, m, nnz, k, row_ptr, col, val, x, ldx, y, ldy, perm, kid);
    case SBX_V_I32: case SBX_V_U32:
      return mm_spmm<I, N, uint32_t>(h, n, m, nnz, k, row_ptr, col, val, x, ldx, y, ldy, perm, kid);
    default: return mm_spmm<I, N, uint64_t>(h, n, m, nnz, k, row_ptr, col, val, x, ldx, y, ldy, perm, kid);  // I64, U64
  }
}

}  // namespace

extern "C" int sbmm_csr_spmm(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz,
                             int64_t k, const void *row_ptr, const void *col, const void *val, const void *x, int64_t ldx,
                             void *y, int64_t ldy) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, n >= 0, "n is negative");
  SBX_REQUIRE(h, m >= 0, "m is negative");
  SBX_REQUIRE(h, nnz >= 0, "nnz is negative");
  SBX_REQUIRE(h, k >= 0, "k is negative");
  SBX_REQUIRE(h, ldx >= k, "ldx is below k");
  SBX_REQUIRE(h, ldy >= k, "ldy is below k");
  SBX_REQUIRE(h, n > 0 || nnz == 0, "nnz > 0 with n == 0");
  SBX_REQUIRE(h, row_ptr != nullptr || n == 0, "row_ptr is NULL");
  SBX_REQUIRE(h, col != nullptr || nnz == 0, "col is NULL");
  SBX_REQUIRE(h, x != nullptr || m == 0 || nnz == 0, "x is NULL");
  SBX_REQUIRE(h, y != nullptr || n == 0, "y is NULL");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  SBX_REQUIRE(h, vt != SBX_V_NONE && sbx_value_bytes(vt) > 0, "the value type must be one of F32, F64, I32, U32, I64, U64");
  if (k > ((int64_t)1 << 20)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: k = %lld > 2^20", __func__, (long long)k);
  if (nnz >= ((int64_t)1 << 42)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: nnz = %lld >= 2^42", __func__, (long long)nnz);
  if (n == 0 || k == 0) return SBX_OK;
  // one column at unit strides is the matrix-vector product: its kernels give a lane to every entry
  if (k == 1 && ldx == 1 && ldy == 1) return sbmv_csr_spmv(h, it, vt, n, m, nnz, row_ptr, col, val, x, y);
  if (it == SBX_I32) return mm_spmm_v<int32_t, int32_t>(h, vt, n, m, nnz, k, row_ptr, col, val, x, ldx, y, ldy);
  if (it == SBX_I32_N64) return mm_spmm_v<int32_t, int64_t>(h, vt, n, m, nnz, k, row_ptr, col, val, x, ldx, y, ldy);
  return mm_spmm_v<int64_t, int64_t>(h, vt, n, m, nnz, k, row_ptr, col, val, x, ldx, y, ldy);
}

// Y = A^T X from a plan (include/sbmt.h): sbmm_csr_spmm of the m x n matrix (col_ptr, row) with every value read through
// perm inside the span kernel.  One column at unit strides stays on the span kernel too: the SpMV has no indirection.
extern "C" int sbmt_csr_spmm_t(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz,
                               int64_t k, const void *col_ptr, const void *row, const void *perm, const void *val,
                               const void *x, int64_t ldx, void *y, int64_t ldy) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, n >= 0, "n is negative");
  SBX_REQUIRE(h, m >= 0, "m is negative");
  SBX_REQUIRE(h, nnz >= 0, "nnz is negative");
  SBX_REQUIRE(h, k >= 0, "k is negative");
  SBX_REQUIRE(h, ldx >= k, "ldx is below k");
  SBX_REQUIRE(h, ldy >= k, "ldy is below k");
  SBX_REQUIRE(h, m > 0 || nnz == 0, "nnz > 0 with m == 0");
  SBX_REQUIRE(h, col_ptr != nullptr || m == 0, "col_ptr is NULL");
  SBX_REQUIRE(h, row != nullptr || nnz == 0, "row is NULL");
  SBX_REQUIRE(h, perm != nullptr || val == nullptr || nnz == 0, "perm is NULL");
  SBX_REQUIRE(h, x != nullptr || n == 0 || nnz == 0, "x is NULL");
  SBX_REQUIRE(h, y != nullptr || m == 0, "y is NULL");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  SBX_REQUIRE(h, vt != SBX_V_NONE && sbx_value_bytes(vt) > 0, "the value type must be one of F32, F64, I32, U32, I64, U64");
  if (k > ((int64_t)1 << 20)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: k = %lld > 2^20", __func__, (long long)k);
  if (nnz >= ((int64_t)1 << 42)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: nnz = %lld >= 2^42", __func__, (long long)nnz);
  if (m == 0 || k == 0) return SBX_OK;
  const void *pm = val ? perm : nullptr;  // (a pattern never reads perm)
  if (it == SBX_I32)
    return mm_spmm_v<int32_t, int32_t>(h, vt, m, n, nnz, k, col_ptr, row, val, x, ldx, y, ldy, pm, SBX_K_SPMM_T);
  if (it == SBX_I32_N64)
    return mm_spmm_v<int32_t, int64_t>(h, vt, m, n, nnz, k, col_ptr, row, val, x, ldx, y, ldy, pm, SBX_K_SPMM_T);
  return mm_spmm_v<int64_t, int64_t>(h, vt, m, n, nnz, k, col_ptr, row, val, x, ldx, y, ldy, pm, SBX_K_SPMM_T);
}
