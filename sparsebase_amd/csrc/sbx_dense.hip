// sbx_dense.hip — the dense side of the Matrix Market path (include/sbio.h).
//
//   io/mtx_reader.cc:141-143, :522-526  `fin >> w`, M * N times            sbio_mtx_parse_values
//   io/mtx_reader.cc:141-165 + the COO constructor's sort                  sbio_dense_to_coo
//   io/mtx_reader.cc:296-301  ReadCoordinateIntoArray's scatter            sbio_coo_to_dense_vector
//
// The value section is tokenized by the kernels of the coordinate parser (sbx_mtx_tokens.h) and one thread per token
// parses it with the same integer and exact decimal conversions (sbx_dec2bin.h).
//
// sbio_dense_to_coo: the file is column-major and a COO is ordered by (row, col), so the compaction is a transpose.
// The matrix is cut into DN_T x DN_T tiles.  A tile is read down its columns (lane = row: a wave's load is DN_T
// consecutive values).  Count: every lane counts the nonzeros of its row inside the tile, one counter per (row, tile
// column) stored at [row * tile_cols + tile column] — global row-major order, inside a row the tiles in column order —
// so one exclusive scan over that array gives every segment its place in the output.  Place: the tile goes through a
// padded LDS tile, every wave then walks rows of it (lane = column), a ballot ranks the nonzeros of the row segment
// and they are written behind the segment's offset: coalesced reads, and writes that are runs of up to DN_T entries.
// Three launches (count, scan, place); no sort.
#include "sbx_dec2bin.h"
#include "sbx_device.h"
#include "sbx_internal.h"
#include "sbx_mtx_tokens.h"
#include "sbio.h"

namespace {

enum : unsigned { DN_BAD_VALUE = 1u, DN_TOO_MANY_DIGITS = 2u, DN_POSITION = 4u };

// ---- values: one thread per token
template <int VKIND /*1 integer, 2 float, 3 double*/, int VB>
__global__ __launch_bounds__(MX_THREADS) void k_dense_parse(const char *__restrict__ text, int64_t bytes,
                                                            const unsigned *__restrict__ tok_off, int64_t count,
                                                            int value_signed, const uint64_t *__restrict__ pow5,
                                                            char *__restrict__ val, unsigned *__restrict__ status) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= count) return;
  unsigned bad = 0;
  const int64_t s = tok_off[l];
  static_assert(DN_BAD_VALUE == MX_VALUE_BAD && DN_TOO_MANY_DIGITS == MX_VALUE_DIGITS, "the status bits of mx_parse_value");
  const uint64_t vbits = mx_parse_value<VKIND, VB>(text + s, mx_token_len(text, bytes, s), value_signed, pow5, &bad);
  if (VB == 4) ((uint32_t *)val)[l] = (uint32_t)vbits;
  else ((uint64_t *)val)[l] = vbits;
  if (bad) atomicOr(status, bad);
}

// ---- dense -> COO
constexpr int DN_T = 64;               // tile edge: one wave is one column of a tile on the way in, one row on the way out
constexpr int DN_THREADS = 256;
constexpr int DN_WAVES = DN_THREADS / 64;
constexpr int DN_PER_WAVE = DN_T / DN_WAVES;  // columns (in) / rows (out) of a tile per wave
constexpr int DN_PAD = DN_T + 1;       // words per LDS column: lane = row on the way in, lane = column on the way out — both
                                       // walk all 64 banks (bank = (column + row) mod 64)
constexpr int64_t DN_MAX_GRID = 1 << 20;

template <int VB>
__device__ __forceinline__ uint64_t dn_load(const char *__restrict__ dense, int64_t cell) {
  return VB == 4 ? (uint64_t)((const uint32_t *)dense)[cell] : ((const uint64_t *)dense)[cell];
}

// tiles are numbered down the tile columns (tile = tile column * tile_rows + tile row): neighbouring workgroups read
// neighbouring pieces of the same columns
template <int VB>
__global__ __launch_bounds__(DN_THREADS) void k_dense_count(const char *__restrict__ dense, int64_t n, int64_t m,
                                                            int64_t tile_rows, int64_t tile_cols, uint64_t nz_mask,
                                                            unsigned *__restrict__ counts) {
  __shared__ unsigned s_cnt[DN_WAVES][DN_T];
  const int lane = sbx_lane(), w = sbx_wave_in_block();
  const int64_t tiles = tile_rows * tile_cols;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t tc = t / tile_rows, tr = t - tc * tile_rows;
    const int64_t r = tr * DN_T + lane, c0 = tc * DN_T;
    unsigned cnt = 0;
    if (r < n) {
#pragma unroll
      for (int k = 0; k < DN_PER_WAVE; k++) {
        const int64_t c = c0 + w + k * DN_WAVES;
        if (c < m) cnt += (dn_load<VB>(dense, c * n + r) & nz_mask) != 0 ? 1u : 0u;
      }
    }
    s_cnt[w][lane] = cnt;
    __syncthreads();
    if (w == 0 && r < n) {
      unsigned tot = 0;
#pragma unroll
      for (int i = 0; i < DN_WAVES; i++) tot += s_cnt[i][lane];
      counts[r * tile_cols + tc] = tot;
    }
    __syncthreads();
  }
}

template <typename I, int VB>
__global__ __launch_bounds__(DN_THREADS) void k_dense_place(const char *__restrict__ dense, int64_t n, int64_t m,
                                                            int64_t tile_rows, int64_t tile_cols, uint64_t nz_mask,
                                                            const unsigned *__restrict__ offsets, I *__restrict__ row_out,
                                                            I *__restrict__ col_out, char *__restrict__ val_out) {
  __shared__ uint32_t s_lo[DN_T * DN_PAD];
  __shared__ uint32_t s_hi[VB == 8 ? DN_T * DN_PAD : 1];  // (a 64-bit value as two planes of words: both conflict-free)
  const int lane = sbx_lane(), w = sbx_wave_in_block();
  const int64_t tiles = tile_rows * tile_cols;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t tc = t / tile_rows, tr = t - tc * tile_rows;
    const int64_t r0 = tr * DN_T, c0 = tc * DN_T;
    // in: lane = row, the wave's columns w, w + DN_WAVES, ...; cells outside the matrix are zeros
#pragma unroll
    for (int k = 0; k < DN_PER_WAVE; k++) {
      const int cl = w + k * DN_WAVES;
      const int64_t r = r0 + lane, c = c0 + cl;
      const uint64_t v = (r < n && c < m) ? dn_load<VB>(dense, c * n + r) : 0ull;
      s_lo[cl * DN_PAD + lane] = (uint32_t)v;
      if (VB == 8) s_hi[cl * DN_PAD + lane] = (uint32_t)(v >> 32);
    }
    __syncthreads();
    // out: lane = column, the wave's rows w, w + DN_WAVES, ...
    for (int k = 0; k < DN_PER_WAVE; k++) {
      const int rl = w + k * DN_WAVES;
      const int64_t r = r0 + rl;
      if (r >= n) break;  // (the same for the whole wave)
      uint64_t v = s_lo[lane * DN_PAD + rl];
      if (VB == 8) v |= (uint64_t)s_hi[lane * DN_PAD + rl] << 32;
      const bool nz = (v & nz_mask) != 0;
      const uint64_t b = __ballot(nz);
      if (nz) {
        const int64_t o = (int64_t)offsets[r * tile_cols + tc] + __popcll(b & sbx_lanemask_lt());
        row_out[o] = (I)r;
        col_out[o] = (I)(c0 + lane);
        if (val_out) {
          if (VB == 4) ((uint32_t *)val_out)[o] = (uint32_t)v;
          else ((uint64_t *)val_out)[o] = v;
        }
      }
    }
    __syncthreads();
  }
}

// ---- sorted COO of a vector -> dense
template <typename I, int VB>
__global__ __launch_bounds__(MX_THREADS) void k_coo_to_vector(const I *__restrict__ row, const I *__restrict__ col,
                                                              const char *__restrict__ val, int64_t nnz, int64_t len,
                                                              char *__restrict__ out, unsigned *__restrict__ status) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  const int64_t p = (int64_t)row[k] + (int64_t)col[k];
  if (p < 0 || p >= len) {
    atomicOr(status, (unsigned)DN_POSITION);
    return;
  }
  // the last of a run of equal positions writes
  if (k + 1 < nnz && (int64_t)row[k + 1] + (int64_t)col[k + 1] == p) return;
  if (VB == 4) ((uint32_t *)out)[p] = ((const uint32_t *)val)[k];
  else ((uint64_t *)out)[p] = ((const uint64_t *)val)[k];
}

// bits of a value that decide `value != 0`: all of an integer, all but the sign of a float (-0.0 == 0)
uint64_t dn_nz_mask(sbx_value_type vt) {
  if (vt == SBX_V_F32) return 0x7FFFFFFFull;
  if (vt == SBX_V_F64) return 0x7FFFFFFFFFFFFFFFull;
  return ~0ull;
}

}  // namespace

#define SBIO_REQUIRE(h, cond, msg)                                      \
  do {                                                                  \
    if (!(cond)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: %s", __func__, msg); \
  } while (0)

extern "C" int sbio_mtx_parse_values(sbx_handle_t h, sbx_value_type vt, const void *text_dev, int64_t bytes, int64_t count,
                                     void *val_out) {
  if (!h) return SBX_ERR_BAD_ARG;
  const int vb = sbx_value_bytes(vt);
  SBIO_REQUIRE(h, vb > 0, "a value type is needed (not SBX_V_NONE)");
  SBIO_REQUIRE(h, bytes >= 0 && count >= 0 && (count == 0 || val_out) && (bytes == 0 || text_dev), "bad argument");
  SBIO_REQUIRE(h, bytes < ((int64_t)1 << 32), "text sections of 4 GiB and more are not supported (32-bit token offsets)");
  SBX_TRY(sbx_arena_begin(h));
  if (count == 0) return SBX_OK;
  if (count > (bytes + 1) / 2)  // (a token and the blank behind it are two bytes: no scratch sized by an impossible count)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbio_mtx_parse_values: %lld bytes of text cannot hold %lld values", (long long)bytes,
             (long long)count);
  NestGuard guard(h);
  const uint64_t *pow5 = nullptr;
  SBX_TRY(sbx_pow5_table(h, &pow5));
  const char *text = (const char *)text_dev;
  const unsigned tiles = (unsigned)((bytes + MX_TILE - 1) / MX_TILE);
  unsigned *tile_tokens = nullptr, *tok_off = nullptr, *status = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)tiles + 1, &tile_tokens));
  SBX_TRY(sbx_salloc(h, (size_t)count, &tok_off));
  SBX_TRY(sbx_salloc(h, 2, &status));
  SBX_HIP(h, hipMemsetAsync(status, 0, 2 * sizeof(unsigned), h->stream));
  SBX_HIP(h, hipMemsetAsync(tile_tokens + tiles, 0, sizeof(unsigned), h->stream));
  SBX_KLAUNCH(h, SBX_K_MTX, k_mtx_count, dim3(tiles), dim3(MX_THREADS), text, bytes, tile_tokens);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_exclusive_scan_u32(h, tile_tokens, tile_tokens, (int64_t)tiles + 1, nullptr));
  unsigned total_tokens = 0;
  SBX_TRY(sbx_readback(h, &total_tokens, tile_tokens + tiles, sizeof(unsigned)));
  if ((int64_t)total_tokens < count)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbio_mtx_parse_values: the text holds %u tokens, %lld values are needed", total_tokens,
             (long long)count);
  SBX_KLAUNCH(h, SBX_K_MTX, k_mtx_offsets, dim3(tiles), dim3(MX_THREADS), text, bytes, (const unsigned *)tile_tokens, count,
              tok_off);
  const int vkind = vt == SBX_V_F32 ? 2 : vt == SBX_V_F64 ? 3 : 1;
  const int vsigned = (vt == SBX_V_I32 || vt == SBX_V_I64) ? 1 : 0;
  const unsigned grid = (unsigned)((count + MX_THREADS - 1) / MX_THREADS);
#define PARSE(VK, VBX)                                                                                       \
  SBX_KLAUNCH(h, SBX_K_MTX, (k_dense_parse<VK, VBX>), dim3(grid), dim3(MX_THREADS), text, bytes,             \
              (const unsigned *)tok_off, count, vsigned, pow5, (char *)val_out, status)
  if (vkind == 1 && vb == 4) PARSE(1, 4);
  else if (vkind == 1) PARSE(1, 8);
  else if (vkind == 2) PARSE(2, 4);
  else PARSE(3, 8);
#undef PARSE
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_MTX, bytes + count * (int64_t)vb);
  unsigned st[2] = {0, 0};
  SBX_TRY(sbx_readback(h, st, status, sizeof(st)));
  if (st[0] & DN_TOO_MANY_DIGITS)
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbio_mtx_parse_values: a value has more than 38 significant digits");
  if (st[0]) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbio_mtx_parse_values: malformed value token in the array section");
  return SBX_OK;
}

extern "C" int sbio_dense_to_coo(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t n, int64_t m,
                                 const void *dense, int64_t capacity, void *row_out, void *col_out, void *val_out,
                                 int64_t *nnz_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  if (it == SBX_I32_N64) it = SBX_I32;  // (no offset array)
  const int vb = sbx_value_bytes(vt);
  SBIO_REQUIRE(h, it == SBX_I32 || it == SBX_I64, "unknown index type");
  SBIO_REQUIRE(h, vb > 0, "a value type is needed (not SBX_V_NONE)");
  SBIO_REQUIRE(h, nnz_host && n >= 0 && m >= 0 && capacity >= 0, "bad argument");
  SBIO_REQUIRE(h, row_out == nullptr || col_out != nullptr, "row_out without col_out");
  *nnz_host = 0;
  if (n >= ((int64_t)1 << 31) || m >= ((int64_t)1 << 31) || n * m >= ((int64_t)1 << 31))
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbio_dense_to_coo: %lld x %lld cells: 2^31 and more are not supported", (long long)n,
             (long long)m);
  SBX_TRY(sbx_arena_begin(h));
  if (n == 0 || m == 0) return SBX_OK;
  SBIO_REQUIRE(h, dense != nullptr, "dense is NULL");
  if (n == 1 && m > 1) {  // a row vector is its own transpose in memory: read it as the column it is, swap the ids
    n = m;
    m = 1;
    void *t = row_out;
    if (row_out) {
      row_out = col_out;
      col_out = t;
    }
  }
  NestGuard guard(h);
  const int64_t tile_rows = (n + DN_T - 1) / DN_T, tile_cols = (m + DN_T - 1) / DN_T;
  const int64_t segments = n * tile_cols;  // < 2^31: at most one per cell
  const unsigned grid = sbx_grid_for(tile_rows * tile_cols, 1, DN_MAX_GRID);
  const uint64_t nz_mask = dn_nz_mask(vt);
  const char *d = (const char *)dense;
  unsigned *counts = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)segments + 1, &counts));
  SBX_HIP(h, hipMemsetAsync(counts + segments, 0, sizeof(unsigned), h->stream));
  if (vb == 4) SBX_KLAUNCH(h, SBX_K_MTX, k_dense_count<4>, dim3(grid), dim3(DN_THREADS), d, n, m, tile_rows, tile_cols, nz_mask, counts);
  else SBX_KLAUNCH(h, SBX_K_MTX, k_dense_count<8>, dim3(grid), dim3(DN_THREADS), d, n, m, tile_rows, tile_cols, nz_mask, counts);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_exclusive_scan_u32(h, counts, counts, segments + 1, nullptr));
  unsigned total = 0;
  SBX_TRY(sbx_readback(h, &total, counts + segments, sizeof(unsigned)));
  const int64_t nnz = (int64_t)total;
  if (row_out == nullptr) {  // count mode
    *nnz_host = nnz;
    return SBX_OK;
  }
  if (capacity < nnz)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbio_dense_to_coo: %lld entries, the outputs hold %lld", (long long)nnz, (long long)capacity);
  if (nnz > 0) {
#define PLACE(I, VBX)                                                                                                 \
  SBX_KLAUNCH(h, SBX_K_MTX, (k_dense_place<I, VBX>), dim3(grid), dim3(DN_THREADS), d, n, m, tile_rows, tile_cols, nz_mask, \
              (const unsigned *)counts, (I *)row_out, (I *)col_out, (char *)val_out)
    if (it == SBX_I32 && vb == 4) PLACE(int32_t, 4);
    else if (it == SBX_I32) PLACE(int32_t, 8);
    else if (vb == 4) PLACE(int64_t, 4);
    else PLACE(int64_t, 8);
#undef PLACE
    SBX_LAUNCH_CHECK(h);
  }
  SBX_PROF_BYTES(h, SBX_K_MTX, n * m * (int64_t)vb + nnz * (int64_t)(2 * sbx_index_bytes(it) + vb));
  *nnz_host = nnz;  // (the outputs are complete in stream order)
  return SBX_OK;
}

extern "C" int sbio_coo_to_dense_vector(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t len, int64_t nnz,
                                        const void *row, const void *col, const void *val, void *out) {
  if (!h) return SBX_ERR_BAD_ARG;
  if (it == SBX_I32_N64) it = SBX_I32;  // (no offset array)
  const int vb = sbx_value_bytes(vt);
  SBIO_REQUIRE(h, it == SBX_I32 || it == SBX_I64, "unknown index type");
  SBIO_REQUIRE(h, vb > 0, "a value type is needed (not SBX_V_NONE)");
  SBIO_REQUIRE(h, len >= 0 && nnz >= 0 && (len == 0 || out) && (nnz == 0 || (row && col && val)), "bad argument");
  SBX_TRY(sbx_arena_begin(h));
  if (len > 0) SBX_HIP(h, hipMemsetAsync(out, 0, (size_t)len * vb, h->stream));
  if (nnz == 0) {
    SBX_HIP(h, hipStreamSynchronize(h->stream));
    return SBX_OK;
  }
  unsigned *status = nullptr;
  SBX_TRY(sbx_salloc(h, 2, &status));
  SBX_HIP(h, hipMemsetAsync(status, 0, 2 * sizeof(unsigned), h->stream));
  const unsigned grid = (unsigned)((nnz + MX_THREADS - 1) / MX_THREADS);
#define VECTOR(I, VBX)                                                                                          \
  SBX_KLAUNCH(h, SBX_K_MTX, (k_coo_to_vector<I, VBX>), dim3(grid), dim3(MX_THREADS), (const I *)row, (const I *)col, \
              (const char *)val, nnz, len, (char *)out, status)
  if (it == SBX_I32 && vb == 4) VECTOR(int32_t, 4);
  else if (it == SBX_I32) VECTOR(int32_t, 8);
  else if (vb == 4) VECTOR(int64_t, 4);
  else VECTOR(int64_t, 8);
#undef VECTOR
  SBX_LAUNCH_CHECK(h);
  unsigned st[2] = {0, 0};
  SBX_TRY(sbx_readback(h, st, status, sizeof(st)));
  if (st[0]) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbio_coo_to_dense_vector: row + col outside [0, %lld)", (long long)len);
  return SBX_OK;
}
