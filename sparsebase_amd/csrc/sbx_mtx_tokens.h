// sbx_mtx_tokens.h — the tokenizer of the text parsers: whitespace-separated tokens of a device text buffer, their
// starts counted per tile and compacted in file order (count, scan, write).  Shared by the coordinate / edge-list
// parsers (sbx_mtx.hip), the array-format parser (sbx_dense.hip) and the METIS graph and PaToH parsers (sbx_metis.hip,
// sbx_patoh.hip), with the conversion of a value token, the launch grid (mx_grid) and the dispatch over the kernels'
// <VKIND, VB> instantiations (mx_value_kind, MX_FOR_VALUE_KIND).
#pragma once
#include "sbx_dec2bin.h"
#include "sbx_device.h"
#include "sbx_internal.h"

namespace {  // (kernels in a header shared by several translation units: internal linkage)

constexpr int MX_THREADS = 256;
constexpr int MX_BPT = 16;                       // text bytes per thread
constexpr int MX_TILE = MX_THREADS * MX_BPT;     // text bytes per workgroup

__device__ __forceinline__ bool mx_space(char c) {
  return c == ' ' || c == '\n' || c == '\t' || c == '\r' || c == '\v' || c == '\f';
}

// token starts of this thread's MX_BPT bytes as a bit mask
__device__ __forceinline__ unsigned mx_starts(const char *__restrict__ text, int64_t bytes, int64_t p0) {
  static_assert(MX_BPT == 16, "one 16-byte load per thread");
  unsigned mask = 0;
  const char before = p0 == 0 ? ' ' : text[p0 - 1];
  if (p0 + MX_BPT <= bytes && (((uintptr_t)text + (uintptr_t)p0) & 15) == 0) {
    // the thread's 16 bytes in one load (byte by byte, under the end-of-text test, the compiler made them 17 loads
    // that wait for one another: tools/isa_waits.py)
    const uint4 v = *(const uint4 *)(text + p0);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    bool prev_space = mx_space(before);
#pragma unroll
    for (int k = 0; k < MX_BPT; k++) {
      const bool sp = mx_space((char)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu));
      if (!sp && prev_space) mask |= 1u << k;
      prev_space = sp;
    }
    return mask;
  }
  bool prev_space = mx_space(before);
#pragma unroll
  for (int k = 0; k < MX_BPT; k++) {
    if (p0 + k >= bytes) break;
    const bool sp = mx_space(text[p0 + k]);
    if (!sp && prev_space) mask |= 1u << k;
    prev_space = sp;
  }
  return mask;
}

__global__ __launch_bounds__(MX_THREADS) void k_mtx_count(const char *__restrict__ text, int64_t bytes,
                                                          unsigned *__restrict__ tile_tokens) {
  __shared__ unsigned s_red[MX_THREADS / 64 + 1];
  const int64_t p0 = (int64_t)blockIdx.x * MX_TILE + (int64_t)threadIdx.x * MX_BPT;
  const unsigned c = p0 < bytes ? (unsigned)__popc(mx_starts(text, bytes, p0)) : 0u;
  const unsigned tot = sbx_block_sum<unsigned, MX_THREADS>(c, s_red);
  if (threadIdx.x == 0) tile_tokens[blockIdx.x] = tot;
}

__global__ __launch_bounds__(MX_THREADS) void k_mtx_offsets(const char *__restrict__ text, int64_t bytes,
                                                            const unsigned *__restrict__ tile_base,
                                                            int64_t max_tokens, unsigned *__restrict__ tok_off) {
  __shared__ unsigned s_scan[MX_THREADS / 64 + 1];
  const int64_t p0 = (int64_t)blockIdx.x * MX_TILE + (int64_t)threadIdx.x * MX_BPT;
  unsigned mask = p0 < bytes ? mx_starts(text, bytes, p0) : 0u;
  unsigned all;
  unsigned t = tile_base[blockIdx.x] + sbx_block_exclusive_sum<unsigned, MX_THREADS>((unsigned)__popc(mask), s_scan, &all);
  while (mask) {
    const int k = __ffs(mask) - 1;
    mask &= mask - 1;
    if ((int64_t)t < max_tokens) tok_off[t] = (unsigned)(p0 + k);
    t++;
  }
}

__device__ __forceinline__ int64_t mx_token_len(const char *__restrict__ text, int64_t bytes, int64_t start) {
  int64_t e = start;
  while (e < bytes && !mx_space(text[e])) e++;
  return e - start;
}

// A value token -> the bits of a value of the type (VKIND 1 integer, 2 float, 3 double; VB its bytes): decimal integers
// checked against the type's range, floating point by the exact decimal conversion of sbx_dec2bin.h.  *flags gets
// MX_VALUE_BAD for a token the type cannot hold or that is no number, MX_VALUE_DIGITS for more than 38 significant digits.
enum : unsigned { MX_VALUE_BAD = 1u, MX_VALUE_DIGITS = 2u };
template <int VKIND, int VB>
__device__ __forceinline__ uint64_t mx_parse_value(const char *__restrict__ s, int64_t len, int value_signed,
                                                   const uint64_t *__restrict__ pow5, unsigned *flags) {
  if (VKIND == 1) {
    long long v = 0;
    if (sbx_parse_integer(s, len, &v)) *flags |= MX_VALUE_BAD;
    if (VB == 4) {
      if (value_signed ? (v < -2147483648ll || v > 2147483647ll) : (v < 0 || v > 4294967295ll)) *flags |= MX_VALUE_BAD;
    } else if (!value_signed && v < 0) {
      *flags |= MX_VALUE_BAD;
    }
    return (uint64_t)v;
  }
  const sbx_decimal d = sbx_parse_decimal(s, len);
  if (d.status == 1) *flags |= MX_VALUE_BAD;
  if (d.status == 2) *flags |= MX_VALUE_DIGITS;
  if (VKIND == 2) return (uint64_t)(sbx_decimal_to_float_bits(d, pow5) | ((uint32_t)d.neg << 31));
  return sbx_decimal_to_double_bits(d, pow5) | ((uint64_t)d.neg << 63);
}

static inline unsigned mx_grid(int64_t count) { return (unsigned)((count + MX_THREADS - 1) / MX_THREADS); }

// The parsers' kernels are instantiated per <VKIND, VB>.  mx_value_kind: the VKIND of a value type (0 where no values are
// read); MX_FOR_VALUE_KIND: CALL(VKIND, VB) for the one of the five instantiations that (vkind, vbytes) names.
static inline int mx_value_kind(sbx_value_type vt, bool has_values) {
  return !has_values ? 0 : vt == SBX_V_F32 ? 2 : vt == SBX_V_F64 ? 3 : 1;
}
static inline int mx_value_signed(sbx_value_type vt) { return (vt == SBX_V_I32 || vt == SBX_V_I64) ? 1 : 0; }
#define MX_FOR_VALUE_KIND(vkind, vbytes, CALL)          \
  do {                                                  \
    if ((vkind) == 0) CALL(0, 4);                       \
    else if ((vkind) == 1 && (vbytes) == 4) CALL(1, 4); \
    else if ((vkind) == 1) CALL(1, 8);                  \
    else if ((vkind) == 2) CALL(2, 4);                  \
    else CALL(3, 8);                                    \
  } while (0)

}  // namespace
