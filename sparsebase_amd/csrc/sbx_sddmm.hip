// sbx_sddmm.hip — out[p] = val[p] * (U[row(p), 0:k] . V[col[p], 0:k]) for every stored entry p of a CSR pattern: the
// sampled dense-dense product, deterministic, balanced over the stored entries (include/sbdd.h).  Rows,
// columns and positions are 64-bit inside; the arrays are read at the width of their index tuple.
//
// The lanes of a wave lie on the k columns, as in sbx_spmm.hip: an entry's row of V is one coalesced load.
//
//   spans    first[t] = the row of entry t * DD_SPAN (k_tile_first_rows of sbx_device.h, as the SpMV and the SpMM)
//   span     one wave per span of DD_SPAN consecutive entries.  A lane holds VEC columns (16 bytes where u, v, ldu, ldv
//            and k allow it, else one value).  L = ceil(k / VEC) lanes cover the k columns:
//              groups   L <= 32: a GROUP is G = the power of two >= L lanes (the lanes from L on hold +0), the wave holds
//                       64 / G groups;
//              wide     L > 32: G = 64, the wave is one group, and where L > 64 the lane walks CB = ceil(L / 64) blocks
//                       of 64 * VEC columns, block b of lane l being the columns (b * 64 + l) * VEC ... + VEC - 1.
//            The span is walked in batches of 512 entries: lane i loads the DD_ITEMS = 8 consecutive entries from
//            t0 + batch * 512 + 8 i on (sbx_load_items8 / sbx_load_values8) and finds their rows (a search in row_ptr
//            between first[t] and first[t + 1], and one more wherever a row ends).  A group then works through the 8 G
//            entries that its own lanes hold, in order: the entry's column and row are broadcast inside the group (the
//            wide form: v_readlane into scalar registers), DD_INFLIGHT rows of V are loaded before the first is
//            multiplied, and the group's slice of U's row stays in registers until the row changes (one block of
//            columns; with several, U is loaded beside V block by block and comes from the cache).  The lane's sum
//            begins at +0 and takes its columns in ascending order, block by block; the lanes of the group are then
//            added by a fixed butterfly (partners at distance 1, 2, 4, ... G / 2), after which every lane of the group
//            holds the dot.  The lane that loaded the entry multiplies by its value and keeps the result; after the
//            batch a lane stores its 8 consecutive results (16 bytes at a time where `out` allows it).
// Nothing crosses a span and nothing is added to memory: no carry pass, no atomics, every out[p] written once.
// What an entry's bits depend on: val[p], the two rows, k and VEC — not p, the group, the batch, the row's length.
// Malformed input: a column outside [0, m) gives +0 without a load from V; every row a search returns lies between
// first[t] and first[t + 1], both in [0, n - 1], whatever row_ptr holds, so every load from U is inside it.
#include <cstddef>

#include "sbdd.h"
#include "sbx_device.h"
#include "sbx_internal.h"

#ifndef DD_SPAN
#define DD_SPAN 2048  // stored entries per wave; sbdd.h states the scratch with it
#endif
#ifndef DD_ITEMS
#define DD_ITEMS 8  // consecutive entries a lane loads per batch: sbx_load_items8 is written for 8
#endif
#ifndef DD_INFLIGHT
#define DD_INFLIGHT 4  // rows of V a group has in flight before the first is multiplied
#endif

namespace {

constexpr int DD = 256;                  // threads per workgroup of the helper kernel (the span kernel runs one wave)
constexpr int DD_BATCH = 64 * DD_ITEMS;  // entries of a batch
static_assert(DD_ITEMS == 8, "sbx_load_items8 and sbx_load_values8 load eight entries");
static_assert(DD_SPAN % DD_BATCH == 0, "whole batches");
static_assert(DD_ITEMS % DD_INFLIGHT == 0, "whole rounds of loads");

template <typename V, int VEC>
struct alignas(sizeof(V) * VEC) DdVec {
  V a[VEC];
};

// the value of lane `src`: the wide form reads it into scalar registers (src is wave-uniform), the groups permute
template <bool WIDE, typename T>
__device__ __forceinline__ T dd_bcast(T x, int src) {
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

// a * b + c: for the float types ONE fused multiply-add, written out.  Left to the compiler's contraction, some of the
// unrolled copies of the loop below came out as v_fma and others as v_mul + v_add, and an entry's bits depended on which
// copy — on its position — took it.
template <typename V>
__device__ __forceinline__ V dd_muladd(V a, V b, V c) {
  if constexpr (sizeof(V) == 4 && (V)0.5 != (V)0) return __builtin_fmaf(a, b, c);
  else if constexpr ((V)0.5 != (V)0) return __builtin_fma(a, b, c);
  else return (V)(a * b + c);
}

template <typename V>
__device__ __forceinline__ V dd_xor(V x, int mask) {  // the value of lane ^ mask
  if constexpr (sizeof(V) == 4) {
    return __builtin_bit_cast(V, __shfl_xor(__builtin_bit_cast(int, x), mask, 64));
  } else {
    return __builtin_bit_cast(V, (uint64_t)__shfl_xor((unsigned long long)__builtin_bit_cast(uint64_t, x), mask, 64));
  }
}

template <int CTRL, typename V>
__device__ __forceinline__ V dd_dpp(V x) {  // a full permutation inside a 16-lane row: every lane has a source
  return __builtin_bit_cast(V, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}

// The sum over the G lanes of a group (G a power of two, wave-uniform; all 64 lanes call it): a butterfly, lane i and
// its partner at distance 1, then 2, 4, ... G / 2 both add the other's value to their own, so after step d every aligned
// block of 2 d lanes holds one value.  4-byte types take the first four steps through DPP: the quad permutations are
// lane ^ 1 and lane ^ 2; row_half_mirror and row_mirror read lane 7 - i and 15 - i, which after the steps before hold
// what lane ^ 4 and lane ^ 8 hold.  a + b == b + a bit for bit, so the partners agree.
template <typename V>
__device__ __forceinline__ V dd_group_sum(V x, int G) {
  if constexpr (sizeof(V) == 4) {
    if (G > 1) x = x + dd_dpp<0xB1>(x);                     // quad_perm [1, 0, 3, 2]
    if (G > 2) x = x + dd_dpp<0x4E>(x);                     // quad_perm [2, 3, 0, 1]
    if (G > 4) x = x + dd_dpp<SBX_DPP_ROW_HALF_MIRROR>(x);
    if (G > 8) x = x + dd_dpp<SBX_DPP_ROW_MIRROR>(x);
    if (G > 16) x = x + dd_xor(x, 16);
    if (G > 32) x = x + dd_xor(x, 32);
  } else {
    for (int d = 1; d < G; d <<= 1) x = x + dd_xor(x, d);
  }
  return x;
}

template <typename I, typename N, typename V, int VEC, bool WIDE>
__global__ __launch_bounds__(64) void k_sddmm_span(const N *__restrict__ rp, const I *__restrict__ col,
                                                   const V *__restrict__ val, const V *__restrict__ u, int64_t ldu,
                                                   const V *__restrict__ v, int64_t ldv, int64_t m, int64_t nnz, int64_t k,
                                                   int G, int CB, bool col_vec, bool val_vec, bool out_vec,
                                                   const int64_t *__restrict__ first, V *__restrict__ out) {
  using Vec = DdVec<V, VEC>;
  constexpr int E = DD_ITEMS;
  constexpr int OW = 16 / (int)sizeof(V);  // values of a 16-byte store
  const int lane = sbx_lane();
  const int g = WIDE ? 0 : lane / G;  // this lane's group (G divides 64: no lane is left over)
  const int l = lane - g * G;
  const int ubase = g * G;
  const int64_t t = blockIdx.x;
  const int64_t t0 = t * DD_SPAN, t1 = t0 + DD_SPAN < nnz ? t0 + DD_SPAN : nnz;
  const int64_t r0 = first[t];
  const int64_t r1 = first[t + 1] < r0 ? r0 : first[t + 1];
  const int64_t j0 = (int64_t)l * VEC;  // this lane's first column (of block 0)
  const bool colok = j0 < k;            // (VEC > 1 only where k % VEC == 0: the whole vector is inside)

  Vec ucur;  // the group's slice of U's row `cur` (one block of columns)
#pragma unroll
  for (int q = 0; q < VEC; q++) ucur.a[q] = (V)0;
  int64_t cur = -1;

  for (int64_t b0 = t0; b0 < t1; b0 += DD_BATCH) {
    // E consecutive entries per lane: a slot past the span's end repeats its last entry and is never stored.  All of
    // [t0, t1) is inside the arrays, and t1 - 1 >= t0.
    const int64_t p0 = b0 + (int64_t)lane * E;
    I c[E];
    V a[E], o[E];
    int64_t r[E];
    sbx_load_items8(col, p0, t1, col_vec, c);
    if (val) {
      sbx_load_values8(val, p0, t1, val_vec, a);
    } else {
#pragma unroll
      for (int e = 0; e < E; e++) a[e] = (V)1;
    }
    {  // the rows: a search for the lane's first entry, then one more wherever an entry reaches the end of the row
      int64_t rr = r0 == r1 ? r0 : sbx_row_of(rp, p0 < t1 ? p0 : t1 - 1, r0, r1);
      int64_t row_end = rr < r1 ? (int64_t)rp[rr + 1] : INT64_MAX;
      r[0] = rr;
#pragma unroll
      for (int e = 1; e < E; e++) {
        if (p0 + e < t1 && p0 + e >= row_end) {
          if (rr < r1) rr = sbx_row_of(rp, p0 + e, rr, r1);
          row_end = rr < r1 ? (int64_t)rp[rr + 1] : INT64_MAX;
        }
        r[e] = rr;
      }
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
      if (!(p0 + e < t1 && (uint64_t)(int64_t)c[e] < (uint64_t)m)) c[e] = (I)-1;
      o[e] = (V)0;
    }

    // the group's 8 G entries in order: lane by lane, and a lane's E entries in turn; DD_INFLIGHT rows of V in flight
    for (int lp = 0; lp < G; lp++) {
      const int src = ubase + lp;
#pragma unroll
      for (int e0 = 0; e0 < E; e0 += DD_INFLIGHT) {
        I cc[DD_INFLIGHT];
        int64_t rr[DD_INFLIGHT];
        V acc[DD_INFLIGHT];
#pragma unroll
        for (int s = 0; s < DD_INFLIGHT; s++) {
          cc[s] = G == 1 ? c[e0 + s] : dd_bcast<WIDE>(c[e0 + s], src);
          rr[s] = G == 1 ? r[e0 + s] : dd_bcast<WIDE>(r[e0 + s], src);
          acc[s] = (V)0;  // (a sum begins at +0: an exact zero never comes out as -0)
        }
        if (CB == 1) {
          Vec xv[DD_INFLIGHT], un[DD_INFLIGHT];
          bool nr[DD_INFLIGHT];
#pragma unroll
          for (int s = 0; s < DD_INFLIGHT; s++) {
#pragma unroll
            for (int q = 0; q < VEC; q++) xv[s].a[q] = un[s].a[q] = (V)0;
            if (colok && cc[s] >= 0) xv[s] = *(const Vec *)(v + (int64_t)cc[s] * ldv + j0);
            nr[s] = colok && rr[s] != (s ? rr[s - 1] : cur);
            if (nr[s]) un[s] = *(const Vec *)(u + rr[s] * ldu + j0);
          }
          cur = rr[DD_INFLIGHT - 1];
#pragma unroll
          for (int s = 0; s < DD_INFLIGHT; s++) {
            if (nr[s]) ucur = un[s];
            const bool ok = colok && cc[s] >= 0;
#pragma unroll
            for (int q = 0; q < VEC; q++) acc[s] = ok ? dd_muladd(ucur.a[q], xv[s].a[q], acc[s]) : acc[s];
          }
        } else {  // (the wide form alone) block by block; U beside V
          for (int bb = 0; bb < CB; bb++) {
            const int64_t j = ((int64_t)bb * 64 + lane) * VEC;
            const bool inside = j < k;
            Vec xv[DD_INFLIGHT], uv[DD_INFLIGHT];
#pragma unroll
            for (int s = 0; s < DD_INFLIGHT; s++) {
#pragma unroll
              for (int q = 0; q < VEC; q++) xv[s].a[q] = uv[s].a[q] = (V)0;
              if (inside && cc[s] >= 0) {
                xv[s] = *(const Vec *)(v + (int64_t)cc[s] * ldv + j);
                uv[s] = *(const Vec *)(u + rr[s] * ldu + j);
              }
            }
#pragma unroll
            for (int s = 0; s < DD_INFLIGHT; s++) {
              const bool ok = inside && cc[s] >= 0;
#pragma unroll
              for (int q = 0; q < VEC; q++) acc[s] = ok ? dd_muladd(uv[s].a[q], xv[s].a[q], acc[s]) : acc[s];
            }
          }
        }
#pragma unroll
        for (int s = 0; s < DD_INFLIGHT; s++) {
          const V dot = dd_group_sum(acc[s], G);
          // the lane that loaded the entry keeps it: the one IEEE product val * dot, or the dot itself for a pattern;
          // +0 where the column lies outside the matrix
          if (l == lp) o[e0 + s] = c[e0 + s] >= 0 ? (val ? (V)(a[e0 + s] * dot) : dot) : (V)0;
        }
      }
    }

    if (out_vec && p0 + E <= t1) {
#pragma unroll
      for (int e = 0; e < E; e += OW) {
        DdVec<V, OW> w;
#pragma unroll
        for (int q = 0; q < OW; q++) w.a[q] = o[e + q];
        *(DdVec<V, OW> *)(out + p0 + e) = w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; e++)
        if (p0 + e < t1) out[p0 + e] = o[e];
    }
  }
}

template <typename I, typename N, typename V>
static int dd_sddmm(sbx_handle_t h, int64_t n, int64_t m, int64_t nnz, int64_t k, const void *row_ptr, const void *col,
                    const void *val, const void *u, int64_t ldu, const void *v, int64_t ldv, void *out) {
  SBX_HIP(h, hipSetDevice(h->device));
  if (k == 0) {  // an empty sum: +0 for every entry
    SBX_HIP(h, hipMemsetAsync(out, 0, (size_t)nnz * sizeof(V), h->stream));
    return SBX_OK;
  }
  SBX_TRY(sbx_arena_begin(h));
  const int64_t spans = (nnz + DD_SPAN - 1) / DD_SPAN;
  int64_t *first = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)spans + 1, &first));
  SBX_KLAUNCH(h, SBX_K_SDDMM, (k_tile_first_rows<N, DD_SPAN, DD>), dim3((unsigned)((spans + 1 + DD - 1) / DD)), dim3(DD),
              (const N *)row_ptr, n, spans, first);

  // 16 bytes of columns per lane where every row of U and V begins on 16 bytes and k is whole vectors; else one column
  constexpr int W = 16 / (int)sizeof(V);
  const bool vec = (((uintptr_t)u | (uintptr_t)v) & 15) == 0 && ldu % W == 0 && ldv % W == 0 && k % W == 0;
  const int64_t lanes = vec ? k / W : k;  // lanes that cover the k columns
  int G = 64, CB = 1;
  if (lanes <= 32) {
    for (G = 1; G < lanes; G <<= 1) {}
  } else {
    CB = (int)((lanes + 63) / 64);  // (at most 2^14)
  }
#define DD_LAUNCH(VEC, WIDE)                                                                                            \
  SBX_KLAUNCH(h, SBX_K_SDDMM, (k_sddmm_span<I, N, V, VEC, WIDE>), dim3((unsigned)spans), dim3(64), (const N *)row_ptr,   \
              (const I *)col, (const V *)val, (const V *)u, ldu, (const V *)v, ldv, m, nnz, k, G, CB,                    \
              ((uintptr_t)col & 15) == 0, ((uintptr_t)val & 15) == 0, ((uintptr_t)out & 15) == 0, (const int64_t *)first, \
              (V *)out)
  if (G == 64) {
    if (vec) DD_LAUNCH(W, true); else DD_LAUNCH(1, true);
  } else {
    if (vec) DD_LAUNCH(W, false); else DD_LAUNCH(1, false);
  }
#undef DD_LAUNCH
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_SDDMM, nnz * (int64_t)(sizeof(I) + (val ? 2 : 1) * sizeof(V)) + n * (int64_t)sizeof(N) +
                                     (n + m) * k * (int64_t)sizeof(V));
  return SBX_OK;
}

template <typename I, typename N>
static int dd_sddmm_v(sbx_handle_t h, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, int64_t k, const void *row_ptr,
                      const void *col, const void *val, const void *u, int64_t ldu, const void *v, int64_t ldv, void *out) {
  switch (vt) {
    case SBX_V_F32: return dd_sddmm<I, N, float>(h, n, m, nnz, k, row_ptr, col, val, u, ldu, v, ldv, out);
    case SBX_V_F64: return dd_sddmm<I, N, double>(h, n, m, nnz, k, row_ptr, col, val, u, ldu, v, ldv, out);
    case SBX_V_I32: case SBX_V_U32: return dd_sddmm<I, N, uint32_t>(h, n, m, nnz, k, row_ptr, col, val, u, ldu, v, ldv, out);
    default: return dd_sddmm<I, N, uint64_t>(h, n, m, nnz, k, row_ptr, col, val, u, ldu, v, ldv, out);  // SBX_V_I64, SBX_V_U64
  }
}

}  // namespace

extern "C" int sbdd_csr_sddmm(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz,
                              int64_t k, const void *row_ptr, const void *col, const void *val, const void *u, int64_t ldu,
                              const void *v, int64_t ldv, void *out) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, n >= 0, "n is negative");
  SBX_REQUIRE(h, m >= 0, "m is negative");
  SBX_REQUIRE(h, nnz >= 0, "nnz is negative");
  SBX_REQUIRE(h, k >= 0, "k is negative");
  SBX_REQUIRE(h, ldu >= k, "ldu is below k");
  SBX_REQUIRE(h, ldv >= k, "ldv is below k");
  SBX_REQUIRE(h, n > 0 || nnz == 0, "nnz > 0 with n == 0");
  SBX_REQUIRE(h, row_ptr != nullptr || n == 0, "row_ptr is NULL");
  SBX_REQUIRE(h, col != nullptr || nnz == 0, "col is NULL");
  SBX_REQUIRE(h, out != nullptr || nnz == 0, "out is NULL");
  SBX_REQUIRE(h, u != nullptr || nnz == 0 || k == 0, "u is NULL");
  SBX_REQUIRE(h, v != nullptr || nnz == 0 || k == 0, "v is NULL");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  SBX_REQUIRE(h, vt != SBX_V_NONE && sbx_value_bytes(vt) > 0, "the value type must be one of F32, F64, I32, U32, I64, U64");
  if (k > ((int64_t)1 << 20)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: k = %lld > 2^20", __func__, (long long)k);
  if (nnz >= ((int64_t)1 << 42)) SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: nnz = %lld >= 2^42", __func__, (long long)nnz);
  if (n == 0 || nnz == 0) return SBX_OK;
  if (it == SBX_I32) return dd_sddmm_v<int32_t, int32_t>(h, vt, n, m, nnz, k, row_ptr, col, val, u, ldu, v, ldv, out);
  if (it == SBX_I32_N64) return dd_sddmm_v<int32_t, int64_t>(h, vt, n, m, nnz, k, row_ptr, col, val, u, ldu, v, ldv, out);
  return dd_sddmm_v<int64_t, int64_t>(h, vt, n, m, nnz, k, row_ptr, col, val, u, ldu, v, ldv, out);
}
