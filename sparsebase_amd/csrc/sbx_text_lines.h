// sbx_text_lines.h — what the parsers of line-structured text share (sbx_metis.hip, sbx_patoh.hip): the starts of the
// lines of a device text buffer, counted per 4096-byte tile and compacted in file order the way sbx_mtx_tokens.h does it
// for tokens; the lower bound that gives a line its first token and a token its line; the store of a parsed value.
#pragma once
#include "sbx_device.h"
#include "sbx_internal.h"
#include "sbx_mtx_tokens.h"

namespace {  // (kernels in a header shared by several translation units: internal linkage)

// ---- line starts: byte 0 and every byte behind a '\n' (a '\n' that ends the text starts nothing)
__device__ __forceinline__ unsigned tl_line_starts(const char *__restrict__ text, int64_t bytes, int64_t p0) {
  static_assert(MX_BPT == 16, "one 16-byte load per thread");
  unsigned mask = 0;
  bool prev_nl = p0 == 0 || text[p0 - 1] == '\n';
  if (p0 + MX_BPT <= bytes && (((uintptr_t)text + (uintptr_t)p0) & 15) == 0) {
    const uint4 v = *(const uint4 *)(text + p0);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < MX_BPT; k++) {
      if (prev_nl) mask |= 1u << k;
      prev_nl = (char)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) == '\n';
    }
    return mask;
  }
#pragma unroll
  for (int k = 0; k < MX_BPT; k++) {
    if (p0 + k >= bytes) break;
    if (prev_nl) mask |= 1u << k;
    prev_nl = text[p0 + k] == '\n';
  }
  return mask;
}

__global__ __launch_bounds__(MX_THREADS) void k_tl_line_count(const char *__restrict__ text, int64_t bytes,
                                                              unsigned *__restrict__ tile_lines) {
  __shared__ unsigned s_red[MX_THREADS / 64 + 1];
  const int64_t p0 = (int64_t)blockIdx.x * MX_TILE + (int64_t)threadIdx.x * MX_BPT;
  const unsigned c = p0 < bytes ? (unsigned)__popc(tl_line_starts(text, bytes, p0)) : 0u;
  const unsigned tot = sbx_block_sum<unsigned, MX_THREADS>(c, s_red);
  if (threadIdx.x == 0) tile_lines[blockIdx.x] = tot;
}

__global__ __launch_bounds__(MX_THREADS) void k_tl_line_offsets(const char *__restrict__ text, int64_t bytes,
                                                                const unsigned *__restrict__ tile_base, int64_t lines,
                                                                unsigned *__restrict__ line_off) {
  __shared__ unsigned s_scan[MX_THREADS / 64 + 1];
  const int64_t p0 = (int64_t)blockIdx.x * MX_TILE + (int64_t)threadIdx.x * MX_BPT;
  unsigned mask = p0 < bytes ? tl_line_starts(text, bytes, p0) : 0u;
  unsigned all;
  unsigned t = tile_base[blockIdx.x] + sbx_block_exclusive_sum<unsigned, MX_THREADS>((unsigned)__popc(mask), s_scan, &all);
  while (mask) {
    const int k = __ffs(mask) - 1;
    mask &= mask - 1;
    if ((int64_t)t < lines) line_off[t] = (unsigned)(p0 + k);
    t++;
  }
}

// first index i in [0, len) with arr[i] >= target, or len
__device__ __forceinline__ int64_t tl_lower_bound(const unsigned *__restrict__ arr, int64_t len, unsigned target) {
  int64_t lo = 0, hi = len;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (arr[mid] < target) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <int VB>
__device__ __forceinline__ void tl_store_value(char *__restrict__ dst, int64_t i, uint64_t bits) {
  if (VB == 4) ((uint32_t *)dst)[i] = (uint32_t)bits;
  else ((uint64_t *)dst)[i] = bits;
}

// Line and token starts of `bytes` bytes of text (steps 1 of the line-structured parsers): the counts, read back, and
// the two ascending offset arrays (lines + 1 and tokens + 1 words; the last word of each is not written).  The caller
// has begun the arena.
static int tl_lines_and_tokens(sbx_handle_t h, const char *text, int64_t bytes, unsigned *lines_out, unsigned *tokens_out,
                               unsigned **line_off_out, unsigned **tok_off_out) {
  const unsigned tiles = (unsigned)((bytes + MX_TILE - 1) / MX_TILE);
  unsigned lines = 0, tokens = 0;
  unsigned *tile_lines = nullptr, *tile_tokens = nullptr, *line_off = nullptr, *tok_off = nullptr;
  if (tiles) {
    SBX_TRY(sbx_salloc(h, (size_t)tiles + 1, &tile_lines));
    SBX_TRY(sbx_salloc(h, (size_t)tiles + 1, &tile_tokens));
    SBX_HIP(h, hipMemsetAsync(tile_lines + tiles, 0, sizeof(unsigned), h->stream));
    SBX_HIP(h, hipMemsetAsync(tile_tokens + tiles, 0, sizeof(unsigned), h->stream));
    SBX_KLAUNCH(h, SBX_K_MTX, k_tl_line_count, dim3(tiles), dim3(MX_THREADS), text, bytes, tile_lines);
    SBX_KLAUNCH(h, SBX_K_MTX, k_mtx_count, dim3(tiles), dim3(MX_THREADS), text, bytes, tile_tokens);
    SBX_LAUNCH_CHECK(h);
    SBX_TRY(sbx_exclusive_scan_u32(h, tile_lines, tile_lines, (int64_t)tiles + 1, nullptr));
    SBX_TRY(sbx_exclusive_scan_u32(h, tile_tokens, tile_tokens, (int64_t)tiles + 1, nullptr));
    SBX_TRY(sbx_readback(h, &lines, tile_lines + tiles, sizeof(unsigned)));
    SBX_TRY(sbx_readback(h, &tokens, tile_tokens + tiles, sizeof(unsigned)));
  }
  SBX_TRY(sbx_salloc(h, (size_t)lines + 1, &line_off));
  SBX_TRY(sbx_salloc(h, (size_t)tokens + 1, &tok_off));
  if (lines) {
    SBX_KLAUNCH(h, SBX_K_MTX, k_tl_line_offsets, dim3(tiles), dim3(MX_THREADS), text, bytes, (const unsigned *)tile_lines,
                (int64_t)lines, line_off);
    if (tokens)
      SBX_KLAUNCH(h, SBX_K_MTX, k_mtx_offsets, dim3(tiles), dim3(MX_THREADS), text, bytes, (const unsigned *)tile_tokens,
                  (int64_t)tokens, tok_off);
    SBX_LAUNCH_CHECK(h);
  }
  *lines_out = lines;
  *tokens_out = tokens;
  *line_off_out = line_off;
  *tok_off_out = tok_off;
  return SBX_OK;
}

}  // namespace
