// sbx_metis.hip — the METIS graph format on the device (include/sbgr.h).
//
//   io/metis_graph_reader.cc:42-101   the vertex lines of MetisGraphReader::ReadGraph    sbgr_metis_parse
//   io/metis_graph_writer.cc:45-82    the vertex lines of MetisGraphWriter::WriteGraph   sbgr_metis_format
//
// The reference reads with getline and one istringstream per line.  The format is the one text format here whose lines
// carry structure — line k is vertex k — but a hub vertex puts a million neighbours on one line, so the work is per token
// and per line start, never a walk along a line:
//   1. line starts (byte 0 and every byte behind a '\n') and token starts (sbx_mtx_tokens.h) are counted per 4096-byte
//      tile and compacted in file order: two ascending offset arrays;
//   2. k_gr_lines    one thread per line: the index of its first token (a search in the token starts), from that and the
//                    next line's the number of its tokens and of its entries, and whether it is a comment; two scans over
//                    the lines give every line its first entry and its vertex;
//   3. k_gr_tokens   one thread per token: its line (a search in the line starts), its ordinal in the line and from that
//                    its role — vertex weight, neighbour, edge weight — and the slot it fills; parsed as the coordinate
//                    parser parses (sbx_dec2bin.h, exact);
//   4. the entries are grouped by row already: the row offsets are the scan of step 2, and only if some row is out of
//      order (sbx_csr_rows_sorted) its inside is sorted, stably (sbx_sort_segments).
// The writer is a formatter of sbx_text.hip's kind over ITEMS — per row one head (the '\n' of the row before), its vertex
// weights, its entries, and one last '\n': GrJob, a job of the emit back end (sbx_text_emit.h), which sums the lengths per
// workgroup, scans them, and writes through LDS.
#include "sbgr.h"
#include "sbx_dec2bin.h"
#include "sbx_device.h"
#include "sbx_internal.h"
#include "sbx_mtx_tokens.h"
#include "sbx_text_emit.h"
#include "sbx_text_lines.h"

namespace {

enum : unsigned { GR_BAD_ID = 1u, GR_BAD_VALUE = 2u, GR_TOO_MANY_DIGITS = 4u, GR_ID_RANGE = 8u, GR_ODD_LINE = 16u };

// one thread per line, and one for the end of the arrays: first token, entries, comment or not
__global__ __launch_bounds__(MX_THREADS) void k_gr_lines(const char *__restrict__ text, const unsigned *__restrict__ line_off,
                                                         int64_t lines, const unsigned *__restrict__ tok_off, int64_t tokens,
                                                         int nvw, int edge_weighted, unsigned *__restrict__ line_tok,
                                                         unsigned *__restrict__ line_cnt, unsigned *__restrict__ line_nc,
                                                         unsigned *__restrict__ status) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l > lines) return;
  if (l == lines) {
    line_tok[l] = (unsigned)tokens;
    line_cnt[l] = 0;
    line_nc[l] = 0;
    return;
  }
  const unsigned start = line_off[l];
  const int64_t a = tl_lower_bound(tok_off, tokens, start);
  const int64_t b = l + 1 < lines ? tl_lower_bound(tok_off, tokens, line_off[l + 1]) : tokens;
  const bool comment = text[start] == '%';
  int64_t k = b - a - nvw;  // neighbour (and edge weight) tokens
  if (k < 0) k = 0;
  if (!comment && edge_weighted && (k & 1)) atomicOr(status, GR_ODD_LINE);
  line_tok[l] = (unsigned)a;
  line_cnt[l] = comment ? 0u : (unsigned)(edge_weighted ? k >> 1 : k);
  line_nc[l] = comment ? 0u : 1u;
}

// row offsets: the row of the j-th line that is no comment begins at that line's first entry ...
__global__ __launch_bounds__(MX_THREADS) void k_gr_row_ptr_lines(const unsigned *__restrict__ line_ent,
                                                                 const unsigned *__restrict__ line_ncb, int64_t lines, int base,
                                                                 int32_t *__restrict__ rp) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= lines || line_ncb[l + 1] == line_ncb[l]) return;
  rp[(int64_t)line_ncb[l] + base] = (int32_t)line_ent[l];
}
// ... row 0 of a 1-based graph at 0, and the rows without a line (and the end) at nnz
__global__ __launch_bounds__(MX_THREADS) void k_gr_row_ptr_rest(int64_t n_dim, int base, int64_t vertex_lines, int32_t nnz,
                                                                int32_t *__restrict__ rp) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n_dim) return;
  if (r < base) rp[r] = 0;
  else if (r >= vertex_lines + base) rp[r] = nnz;
}

// one thread per token
template <int VKIND /*0 none, 1 integer, 2 float, 3 double*/, int VB>
__global__ __launch_bounds__(MX_THREADS) void k_gr_tokens(const char *__restrict__ text, int64_t bytes,
                                                          const unsigned *__restrict__ tok_off, int64_t tokens,
                                                          const unsigned *__restrict__ line_off, int64_t lines,
                                                          const unsigned *__restrict__ line_tok,
                                                          const unsigned *__restrict__ line_ent,
                                                          const unsigned *__restrict__ line_ncb, int nvw, int ncon,
                                                          int edge_weighted, int zero_index, int64_t n_dim, int64_t nnz,
                                                          int value_signed, const uint64_t *__restrict__ pow5,
                                                          int32_t *__restrict__ row, int32_t *__restrict__ col,
                                                          char *__restrict__ val, char *__restrict__ vwgt,
                                                          unsigned *__restrict__ status) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= tokens) return;
  const unsigned s = tok_off[t];
  const int64_t l = tl_lower_bound(line_off, lines, s + 1u) - 1;  // the last line that starts at or before the token
  if (l < 0 || line_ncb[l + 1] == line_ncb[l]) return;            // (a token of a comment line does not exist)
  const int64_t vertex = (int64_t)line_ncb[l] + (zero_index ? 0 : 1);
  const int64_t ord = t - (int64_t)line_tok[l];
  const int64_t len = mx_token_len(text, bytes, s);
  unsigned bad = 0;
  if (ord < nvw) {  // a vertex weight
    if (VKIND != 0 && vwgt) {
      unsigned vf = 0;
      const uint64_t bits = mx_parse_value<VKIND == 0 ? 1 : VKIND, VB>(text + s, len, value_signed, pow5, &vf);
      if (vf & MX_VALUE_BAD) bad |= GR_BAD_VALUE;
      if (vf & MX_VALUE_DIGITS) bad |= GR_TOO_MANY_DIGITS;
      tl_store_value<VB>(vwgt, vertex * ncon + ord, bits);
    }
  } else {
    const int64_t k = ord - nvw;
    const int64_t pos = (int64_t)line_ent[l] + (edge_weighted ? k >> 1 : k);
    if (pos < nnz) {  // (always, once the host has compared the counts)
      if (edge_weighted && (k & 1)) {
        if (VKIND != 0 && val) {
          unsigned vf = 0;
          const uint64_t bits = mx_parse_value<VKIND == 0 ? 1 : VKIND, VB>(text + s, len, value_signed, pow5, &vf);
          if (vf & MX_VALUE_BAD) bad |= GR_BAD_VALUE;
          if (vf & MX_VALUE_DIGITS) bad |= GR_TOO_MANY_DIGITS;
          tl_store_value<VB>(val, pos, bits);
        }
      } else {
        long long id = 0;
        if (sbx_parse_integer(text + s, len, &id)) {  // (malformed, not out of range: the message names which)
          bad |= GR_BAD_ID;
          id = 0;
        } else {
          if (zero_index) id--;
          if (id < 0 || id >= n_dim) {
            bad |= GR_ID_RANGE;
            id = 0;
          }
        }
        row[pos] = (int32_t)vertex;
        col[pos] = (int32_t)id;
      }
    }
  }
  if (bad) atomicOr(status, bad);
}

// ---- the formatter: a job of the emit back end (sbx_text_emit.h).  A row has 1 + nvw + (its entries) items: the head,
// the vertex weights, the entries; behind the last row comes one item more (the last '\n').
template <typename RP, typename CI>
struct GrJob {
  const RP *rp;
  const CI *col;
  const void *val, *vwgt;
  const sbx_decrec *rec_val, *rec_vw;  // TI_RECORD: of entry e at [e - e0], of weight j of row r at [(r - rb) * ncon + j]
  int64_t rb, re, e0, items, base;
  int nvw, ncon, ew, vw, vkind, vb, precision;
  // key(r) = the first item of row r; key(re) is that last item
  __device__ __forceinline__ int64_t key(int64_t r) const { return ((int64_t)rp[r] - e0) + (r - rb) * (int64_t)(1 + nvw); }
  __device__ __forceinline__ void locate(int64_t k, int64_t *row, int64_t *sub) const {
    int64_t lo = rb, hi = re;  // the last row r in [rb, re] with key(r) <= k
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (key(mid) <= k) lo = mid;
      else hi = mid - 1;
    }
    *row = lo;
    *sub = k - key(lo);
  }
  __device__ __forceinline__ int value(const void *arr, const sbx_decrec *rec, int64_t i, int64_t irel, char *dst) const {
    return dst ? tx_item_value_emit(vkind, vb, precision, arr, rec, i, irel, dst)
               : tx_item_value_length(vkind, vb, precision, arr, rec, i, irel);
  }
  __device__ __forceinline__ unsigned item(int64_t r, int64_t sub, char *dst) const {
    int o = 0;
    if (r == re) {  // behind the last row
      if (dst) dst[0] = '\n';
      return 1;
    }
    if (sub == 0) {  // the head: the row before ends; a vertex-weighted row without weights still gets the two blanks
      if (r > rb) {
        if (dst) dst[o] = '\n';
        o++;
      }
      if (vw && nvw == 0) {
        if (dst) dst[o] = ' ', dst[o + 1] = ' ';
        o += 2;
      }
      return (unsigned)o;
    }
    if (sub <= nvw) {  // vertex weight sub - 1: "w ", and two blanks more behind the last one
      o = value(vwgt, rec_vw, r * ncon + (sub - 1), (r - rb) * ncon + (sub - 1), dst);
      const int blanks = sub == nvw ? 3 : 1;
      if (dst)
        for (int b = 0; b < blanks; b++) dst[o + b] = ' ';
      return (unsigned)(o + blanks);
    }
    const int64_t e = (int64_t)rp[r] + (sub - 1 - nvw);
    const bool last = e + 1 == (int64_t)rp[r + 1];
    const int64_t c = (int64_t)col[e] + base;
    if (dst) dst[0] = ' ';
    o = 1;
    o += dst ? tx_emit_signed(c, dst + o) : tx_len_signed(c);
    if (ew) {
      if (dst) dst[o] = ' ';
      o++;
      o += value(val, rec_val, e, e - e0, dst ? dst + o : nullptr);
    }
    if (!last) {
      const int blanks = ew ? 2 : 1;
      if (dst)
        for (int b = 0; b < blanks; b++) dst[o + b] = ' ';
      o += blanks;
    }
    return (unsigned)o;
  }
};
constexpr int GR_ITEM_MAX = 1 + 20 + 1 + SBX_DEC_MAX_CHARS + 2;  // the longest item: an entry with its value and two blanks
static_assert(GR_ITEM_MAX <= TX_LINE_MAX && SBX_DEC_MAX_CHARS + 3 <= TX_LINE_MAX, "an item fits its LDS slot");

}  // namespace

extern "C" int sbgr_metis_parse(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, const void *text_dev, int64_t bytes,
                                int64_t n, int64_t m, int fmt, int ncon, unsigned flags, int64_t capacity, void *row_out,
                                void *col_out, void *val_out, void *vwgt_out, void *row_ptr_out, int64_t *dims_nnz_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, dims_nnz_host && bytes >= 0 && (bytes == 0 || text_dev), "bad argument");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  SBX_REQUIRE(h, n >= 0 && m >= 0 && ncon >= 0 && capacity >= 0, "n, m, ncon and capacity must not be negative");
  SBX_REQUIRE(h, (flags & ~SBGR_ZERO_INDEX) == 0, "unknown flag");
  const int vbytes = sbx_value_bytes(vt);
  SBX_REQUIRE(h, vbytes >= 0, "unknown value type");
  dims_nnz_host[0] = dims_nnz_host[1] = 0;
  if (fmt != 0 && fmt != 1 && fmt != 10 && fmt != 11)
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbgr_metis_parse: FMT %d (vertex sizes) is not supported: 0, 1, 10 or 11", fmt);
  if (bytes >= ((int64_t)1 << 32))
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbgr_metis_parse: texts of 4 GiB and more are not supported (32-bit token offsets)");
  const bool zero_index = (flags & SBGR_ZERO_INDEX) != 0;
  const int base = zero_index ? 0 : 1;
  const int64_t n_dim = n + base;
  if (n_dim >= ((int64_t)1 << 31) - 1 || m >= ((int64_t)1 << 30))
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbgr_metis_parse: n and 2 * m must be below 2^31");
  const int64_t nnz = 2 * m;
  const bool edge_weighted = fmt == 1 || fmt == 11, vertex_weighted = fmt >= 10 && ncon > 0;
  const int nvw = vertex_weighted ? ncon : 0;
  SBX_REQUIRE(h, capacity >= nnz, "output capacity: 2 * m entries");
  SBX_REQUIRE(h, nnz == 0 || (row_out && col_out), "row_out and col_out are needed");
  char *val = (edge_weighted && vbytes) ? (char *)val_out : nullptr;
  char *vwgt = (vertex_weighted && vbytes) ? (char *)vwgt_out : nullptr;
  const bool wide_ids = it == SBX_I64, wide_offsets = it != SBX_I32;
  SBX_TRY(sbx_arena_begin(h));
  NestGuard guard(h);
  const char *text = (const char *)text_dev;
  unsigned *status = nullptr;
  SBX_TRY(sbx_salloc(h, 1, &status));
  SBX_HIP(h, hipMemsetAsync(status, 0, sizeof(unsigned), h->stream));
  // (1) line starts and token starts
  unsigned lines = 0, tokens = 0;
  unsigned *line_off = nullptr, *tok_off = nullptr;
  SBX_TRY(tl_lines_and_tokens(h, text, bytes, &lines, &tokens, &line_off, &tok_off));
  // (2) per line: first token, entries, comment; scans: first entry and vertex of every line
  unsigned *line_tok = nullptr, *line_ent = nullptr, *line_ncb = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)lines + 1, &line_tok));
  SBX_TRY(sbx_salloc(h, (size_t)lines + 1, &line_ent));
  SBX_TRY(sbx_salloc(h, (size_t)lines + 1, &line_ncb));
  SBX_KLAUNCH(h, SBX_K_MTX, k_gr_lines, dim3(mx_grid((int64_t)lines + 1)), dim3(MX_THREADS), text,
              (const unsigned *)line_off, (int64_t)lines, (const unsigned *)tok_off, (int64_t)tokens, nvw,
              edge_weighted ? 1 : 0, line_tok, line_ent, line_ncb, status);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_exclusive_scan_u32(h, line_ent, line_ent, (int64_t)lines + 1, nullptr));
  SBX_TRY(sbx_exclusive_scan_u32(h, line_ncb, line_ncb, (int64_t)lines + 1, nullptr));
  unsigned found = 0, vertex_lines = 0, st = 0;
  SBX_TRY(sbx_readback(h, &found, line_ent + lines, sizeof(unsigned)));
  SBX_TRY(sbx_readback(h, &vertex_lines, line_ncb + lines, sizeof(unsigned)));
  SBX_TRY(sbx_readback(h, &st, status, sizeof(unsigned)));
  if ((int64_t)vertex_lines > n)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbgr_metis_parse: the text has %u vertex lines, the header's n is %lld", vertex_lines,
             (long long)n);
  if (st & GR_ODD_LINE)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbgr_metis_parse: a line of an edge-weighted file has a neighbour without a weight");
  if ((int64_t)found != nnz)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbgr_metis_parse: the lines hold %u neighbours, the header's m = %lld needs %lld", found,
             (long long)m, (long long)nnz);
  // (3) row offsets, then the tokens
  int32_t *rp = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)n_dim + 1, &rp));
  if (lines)
    SBX_KLAUNCH(h, SBX_K_MTX, k_gr_row_ptr_lines, dim3(mx_grid(lines)), dim3(MX_THREADS), (const unsigned *)line_ent,
                (const unsigned *)line_ncb, (int64_t)lines, base, rp);
  SBX_KLAUNCH(h, SBX_K_MTX, k_gr_row_ptr_rest, dim3(mx_grid(n_dim + 1)), dim3(MX_THREADS), n_dim, base,
              (int64_t)vertex_lines, (int32_t)nnz, rp);
  SBX_LAUNCH_CHECK(h);
  if (vwgt) SBX_HIP(h, hipMemsetAsync(vwgt, 0, (size_t)n_dim * (size_t)ncon * (size_t)vbytes, h->stream));
  int32_t *r32 = (int32_t *)row_out, *c32 = (int32_t *)col_out;
  if (wide_ids && nnz) {
    SBX_TRY(sbx_salloc(h, (size_t)nnz, &r32));
    SBX_TRY(sbx_salloc(h, (size_t)nnz, &c32));
  }
  if (tokens) {
    const uint64_t *pow5 = nullptr;
    const bool values = val || vwgt;
    if (values) SBX_TRY(sbx_pow5_table(h, &pow5));
    const int vkind = mx_value_kind(vt, values), vsigned = mx_value_signed(vt);
#define TOKENS(VK, VBX)                                                                                                  \
  SBX_KLAUNCH(h, SBX_K_MTX, (k_gr_tokens<VK, VBX>), dim3(mx_grid(tokens)), dim3(MX_THREADS), text, bytes,                  \
              (const unsigned *)tok_off, (int64_t)tokens, (const unsigned *)line_off, (int64_t)lines,                      \
              (const unsigned *)line_tok, (const unsigned *)line_ent, (const unsigned *)line_ncb, nvw, ncon,               \
              edge_weighted ? 1 : 0, zero_index ? 1 : 0, n_dim, nnz, vsigned, pow5, r32, c32, val, vwgt, status)
    MX_FOR_VALUE_KIND(vkind, vbytes, TOKENS);
#undef TOKENS
    SBX_LAUNCH_CHECK(h);
    SBX_PROF_BYTES(h, SBX_K_MTX, bytes + nnz * (int64_t)(8 + (val ? vbytes : 0)));
    SBX_TRY(sbx_readback(h, &st, status, sizeof(unsigned)));
    if (st & GR_TOO_MANY_DIGITS)
      SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbgr_metis_parse: a value has more than 38 significant digits");
    if (st & GR_ID_RANGE)
      SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbgr_metis_parse: a neighbour id outside [%d, %lld]", zero_index ? 1 : 0,
               (long long)(zero_index ? n_dim : n_dim - 1));
    if (st)
      SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbgr_metis_parse: malformed %s",
               (st & GR_BAD_ID) && (st & GR_BAD_VALUE) ? "neighbour id and weight tokens"
               : (st & GR_BAD_ID)                      ? "neighbour id token"
                                                       : "weight token");
  }
  // (4) the inside of the rows, if one of them is out of order
  if (nnz > 1) {
    int sorted = 1;
    SBX_TRY(sbx_csr_rows_sorted(h, SBX_I32, n_dim, rp, c32, &sorted));
    if (!sorted) {
      int32_t *ctmp = nullptr;
      char *vtmp = nullptr;
      const int vb = val ? vbytes : 0;
      SBX_TRY(sbx_salloc(h, (size_t)nnz, &ctmp));
      SBX_HIP(h, hipMemcpyAsync(ctmp, c32, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
      if (vb) {
        SBX_TRY(sbx_salloc(h, (size_t)nnz * vb, &vtmp));
        SBX_HIP(h, hipMemcpyAsync(vtmp, val, (size_t)nnz * vb, hipMemcpyDeviceToDevice, h->stream));
      }
      SBX_TRY(sbx_sort_segments(h, vb, n_dim, n_dim, nnz, rp, ctmp, vtmp, c32, val));  // stable: file order among equals
    }
  }
  if (wide_ids && nnz) {
    SBX_TRY(sbx_widen_i32(h, r32, row_out, nnz));
    SBX_TRY(sbx_widen_i32(h, c32, col_out, nnz));
  }
  if (row_ptr_out) {
    if (wide_offsets) SBX_TRY(sbx_widen_i32(h, rp, row_ptr_out, n_dim + 1));
    else SBX_HIP(h, hipMemcpyAsync(row_ptr_out, rp, (size_t)(n_dim + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  }
  dims_nnz_host[0] = n_dim;
  dims_nnz_host[1] = nnz;
  return SBX_OK;
}

template <typename RP, typename CI>
static int gr_format_typed(sbx_handle_t h, GrJob<RP, CI> job, void *text_out, int64_t capacity, int64_t *bytes_host) {
  // the ends of the range, and that the offsets between them ascend (the item search relies on it)
  const int64_t rows = job.re - job.rb;
  int64_t hends[2] = {0, 0};
  bool hdesc = false;
  SBX_TRY(tx_range_ends<RP>(h, job.rp, job.rb, job.re, hends, &hdesc));
  if (hdesc) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbgr_metis_format: row_ptr descends inside the row range");
  const int64_t entries = hends[1] - hends[0];
  job.e0 = hends[0];
  job.items = entries + rows * (int64_t)(1 + job.nvw) + 1;
  if (job.items >= ((int64_t)1 << 32))
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbgr_metis_format: 2^32 items and more in one call (pass the rows in sub-ranges)");
  if (job.vkind == TI_RECORD) {
    sbx_decrec *rec = nullptr;
    if (job.ew && entries) {
      SBX_TRY(tx_records(h, (const char *)job.val + hends[0] * job.vb, nullptr, entries, job.vb, job.precision, &rec));
      job.rec_val = rec;
    }
    if (job.nvw) {
      SBX_TRY(tx_records(h, (const char *)job.vwgt + job.rb * job.ncon * (int64_t)job.vb, nullptr, rows * job.ncon, job.vb,
                         job.precision, &rec));
      job.rec_vw = rec;
    }
  }
  return tx_emit(h, "sbgr_metis_format", job, entries * (int64_t)(sizeof(CI) + job.vb), text_out, capacity, bytes_host);
}

extern "C" int sbgr_metis_format(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t row_begin, int64_t row_end,
                                 const void *row_ptr, const void *col, const void *val, const void *vwgt, int ncon,
                                 int64_t index_base, int precision, unsigned flags, void *text_out, int64_t capacity,
                                 int64_t *bytes_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, bytes_host && capacity >= 0 && ncon >= 0, "bad argument");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  SBX_REQUIRE(h, row_begin >= 0 && row_end >= row_begin, "row range");
  SBX_REQUIRE(h, precision >= 1 && precision <= 17, "precision: 1..17");
  SBX_REQUIRE(h, (flags & ~(SBGR_EDGE_WEIGHTS | SBGR_VERTEX_WEIGHTS)) == 0, "unknown flag");
  const int vbytes = sbx_value_bytes(vt);
  SBX_REQUIRE(h, vbytes >= 0, "unknown value type");
  const bool ew = (flags & SBGR_EDGE_WEIGHTS) != 0, vw = (flags & SBGR_VERTEX_WEIGHTS) != 0;
  SBX_REQUIRE(h, !ew || (val && vt != SBX_V_NONE), "SBGR_EDGE_WEIGHTS needs values");
  SBX_REQUIRE(h, !vw || vt != SBX_V_NONE, "SBGR_VERTEX_WEIGHTS needs a value type");
  SBX_REQUIRE(h, !vw || ncon == 0 || vwgt, "SBGR_VERTEX_WEIGHTS with ncon > 0 needs vwgt");
  *bytes_host = 0;
  SBX_TRY(sbx_arena_begin(h));
  if (row_end == row_begin) return SBX_OK;
  SBX_REQUIRE(h, row_ptr, "row_ptr is needed");
  NestGuard guard(h);
#define GR_JOB(RP, CI)                 \
  GrJob<RP, CI> job = {};              \
  job.rp = (const RP *)row_ptr;        \
  job.col = (const CI *)col;           \
  job.val = val;                       \
  job.vwgt = vwgt;                     \
  job.rb = row_begin;                  \
  job.re = row_end;                    \
  job.base = index_base;               \
  job.ncon = ncon;                     \
  job.nvw = vw ? ncon : 0;             \
  job.ew = ew ? 1 : 0;                 \
  job.vw = vw ? 1 : 0;                 \
  job.vb = vbytes;                     \
  job.precision = precision;           \
  job.vkind = tx_item_kind(vt);        \
  return gr_format_typed<RP, CI>(h, job, text_out, capacity, bytes_host)
  if (it == SBX_I64) {
    GR_JOB(int64_t, int64_t);
  }
  if (it == SBX_I32_N64) {
    GR_JOB(int64_t, int32_t);
  }
  GR_JOB(int32_t, int32_t);
#undef GR_JOB
}
