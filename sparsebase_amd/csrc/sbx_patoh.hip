// sbx_patoh.hip — the PaToH hypergraph format on the device (include/sbhg.h).
//
//   io/patoh_reader.cc:145-186   the line loop of PatohReader::ReadHyperGraph            sbhg_patoh_parse
//   io/patoh_reader.cc:187-231   its cells x pins loops for the cell -> net side         sbhg_cells_to_nets
//   io/patoh_writer.cc           the net lines and the cell-weight line of PatohWriter   sbhg_patoh_format[_weights]
//
// The parse is the METIS parse (sbx_metis.hip) with another role rule.  A net of a million pins and the cell-weight line
// of 10^7 tokens are single lines, so the work is per token and per line start, never a walk along a line:
//   1. line starts and token starts per 4096-byte tile, compacted in file order (sbx_text_lines.h, sbx_mtx_tokens.h);
//   2. k_hg_lines    one thread per line: its first token (a search in the token starts), its pins, whether it is a net;
//                    the last line decides whether it is the cell-weight line; two scans over the lines give every line
//                    its first pin and its net;
//   3. k_hg_tokens   one thread per token: its line (a search in the line starts), its ordinal in the line and from that
//                    its role — net weight, pin, cell weight — and the slot it fills.
// The transpose is a stable sort of (cell, net) pairs by cell (sbx_countsort.h up to 2^20 pins, the one-sweep radix sort
// of sbx_prims.hip above): the net of a pin position is the row it lies in (sbx_row_of), looked up in position order
// before the sort; nets come out ascending because positions do and the sort is stable, and the offsets are a lower
// bound of every cell in the sorted keys.  Nothing is read back between the steps and no row is sorted afterwards.
// The writers are formatters of sbx_text.hip's kind over ITEMS — per net one head (its weight, or nothing) and its pins,
// the '\n' riding on the net's last item: HgNetJob and HgWeightJob, jobs of the emit back end (sbx_text_emit.h), which sums
// the lengths per workgroup, scans them, and writes through LDS.
#include "sbhg.h"
#include "sbx_countsort.h"
#include "sbx_dec2bin.h"
#include "sbx_device.h"
#include "sbx_internal.h"
#include "sbx_mtx_tokens.h"
#include "sbx_text_emit.h"
#include "sbx_text_lines.h"

namespace {

enum : unsigned { HG_BAD_PIN = 1u, HG_BAD_WEIGHT = 2u, HG_PIN_RANGE = 4u, HG_EMPTY_WEIGHTED = 8u };

// one thread per line, and one for the end of the arrays: first token, pins, net or not.  info[0]: the last line is the
// cell-weight line; info[1]: its tokens
__global__ __launch_bounds__(MX_THREADS) void k_hg_lines(const char *__restrict__ text, int64_t bytes,
                                                         const unsigned *__restrict__ line_off, int64_t lines,
                                                         const unsigned *__restrict__ tok_off, int64_t tokens,
                                                         int cells_weighted, int nets_weighted, unsigned *__restrict__ line_tok,
                                                         unsigned *__restrict__ line_cnt, unsigned *__restrict__ line_nc,
                                                         unsigned *__restrict__ info, unsigned *__restrict__ status) {
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
  const bool cw = cells_weighted && l == lines - 1 && !comment && text[bytes - 1] != '\n';
  if (cw) {
    info[0] = 1u;
    info[1] = (unsigned)(b - a);
  }
  const bool net = !comment && !cw;
  int64_t k = b - a;
  if (net && nets_weighted) {
    if (k == 0) atomicOr(status, HG_EMPTY_WEIGHTED);
    else k--;
  }
  line_tok[l] = (unsigned)a;
  line_cnt[l] = net ? (unsigned)k : 0u;
  line_nc[l] = net ? 1u : 0u;
}

// xpin: net j begins at the first pin of its line; the end at the number of pins
__global__ __launch_bounds__(MX_THREADS) void k_hg_xpin(const unsigned *__restrict__ line_ent,
                                                        const unsigned *__restrict__ line_ncb, int64_t lines,
                                                        int32_t *__restrict__ xp) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l > lines) return;
  if (l == lines || line_ncb[l + 1] != line_ncb[l]) xp[line_ncb[l]] = (int32_t)line_ent[l];
}

template <int VB>
__global__ __launch_bounds__(MX_THREADS) void k_hg_fill(char *__restrict__ dst, int64_t count, uint64_t bits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) tl_store_value<VB>(dst, i, bits);
}

// a weight token: a decimal integer (the reference reads an int), converted to the value type
template <int VKIND, int VB>
__device__ __forceinline__ uint64_t hg_weight(const char *__restrict__ s, int64_t len, int value_signed, unsigned *bad) {
  if (VKIND == 1) {
    unsigned vf = 0;
    const uint64_t bits = mx_parse_value<1, VB>(s, len, value_signed, nullptr, &vf);
    if (vf) *bad |= HG_BAD_WEIGHT;
    return bits;
  }
  long long v = 0;
  if (sbx_parse_integer(s, len, &v)) *bad |= HG_BAD_WEIGHT;
  if (VKIND == 2) return (uint64_t)__float_as_uint((float)v);
  return (uint64_t)__double_as_longlong((double)v);
}

// one thread per token
template <int VKIND /*0 none, 1 integer, 2 float, 3 double*/, int VB>
__global__ __launch_bounds__(MX_THREADS) void k_hg_tokens(const char *__restrict__ text, int64_t bytes,
                                                          const unsigned *__restrict__ tok_off, int64_t tokens,
                                                          const unsigned *__restrict__ line_off, int64_t lines,
                                                          const unsigned *__restrict__ line_tok,
                                                          const unsigned *__restrict__ line_ent,
                                                          const unsigned *__restrict__ line_ncb,
                                                          const unsigned *__restrict__ info, int nets_weighted, int base,
                                                          int64_t cells, int64_t nets, int64_t pins, int value_signed,
                                                          int32_t *__restrict__ pin, char *__restrict__ nwgt,
                                                          char *__restrict__ cwgt, unsigned *__restrict__ status) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= tokens) return;
  const unsigned s = tok_off[t];
  const int64_t l = tl_lower_bound(line_off, lines, s + 1u) - 1;  // the last line that starts at or before the token
  if (l < 0) return;
  const int64_t ord = t - (int64_t)line_tok[l];
  const int64_t len = mx_token_len(text, bytes, s);
  unsigned bad = 0;
  if (l == lines - 1 && info[0]) {  // a cell weight
    if (VKIND != 0 && cwgt && ord < cells) tl_store_value<VB>(cwgt, ord, hg_weight<VKIND == 0 ? 1 : VKIND, VB>(text + s, len, value_signed, &bad));
  } else if (line_ncb[l + 1] != line_ncb[l]) {  // (a token of a comment line does not exist)
    const int64_t net = line_ncb[l];
    if (nets_weighted && ord == 0) {
      if (VKIND != 0 && nwgt && net < nets) tl_store_value<VB>(nwgt, net, hg_weight<VKIND == 0 ? 1 : VKIND, VB>(text + s, len, value_signed, &bad));
    } else {
      const int64_t pos = (int64_t)line_ent[l] + ord - (nets_weighted ? 1 : 0);
      if (pos < pins) {  // (always, once the host has compared the counts)
        long long id = 0;
        if (sbx_parse_integer(text + s, len, &id)) {
          bad |= HG_BAD_PIN;
          id = base;
        } else if (id < base || id >= cells + base) {
          bad |= HG_PIN_RANGE;
          id = base;
        }
        pin[pos] = (int32_t)id;
      }
    }
  }
  if (bad) atomicOr(status, bad);
}

// ---- the transpose
// (cell, net) of every pin position: the net is the row the position lies in.  Neighbouring positions lie in the same or
// in neighbouring rows, so the searches of a wave walk the same few cache lines; looked up behind the sort, at positions
// in cell order, the same search missed at every step (508 us of the 870 us the call took at 10^7 pins)
template <typename XP, typename CI>
__global__ __launch_bounds__(256) void k_hg_keys(const XP *__restrict__ xpin, int64_t nets, const CI *__restrict__ pin,
                                                 int64_t pins, int base, int64_t cells, uint32_t *__restrict__ key,
                                                 uint32_t *__restrict__ net, unsigned *__restrict__ status) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pins) return;
  int64_t c = (int64_t)pin[p] - base;
  if (c < 0 || c >= cells) {
    atomicOr(status, HG_PIN_RANGE);
    c = 0;
  }
  key[p] = (uint32_t)c;
  net[p] = (uint32_t)(sbx_row_of(xpin, nets, p) + base);
}

// the last digit's placement of the counting sort: the sorted key stays (the offsets are searched in it), the net goes
// to its place
template <typename CI>
struct HgEmit {
  uint32_t *skey;
  CI *net_out;
  __device__ void operator()(unsigned pos, uint32_t key, uint32_t val) const {
    skey[pos] = key;
    net_out[pos] = (CI)val;
  }
};

template <typename CI>
__global__ __launch_bounds__(256) void k_hg_nets(const uint32_t *__restrict__ snet, int64_t pins, CI *__restrict__ net_out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < pins) net_out[p] = (CI)snet[p];
}

template <typename XP>
__global__ __launch_bounds__(256) void k_hg_xnet(const uint32_t *__restrict__ skey, int64_t pins, int64_t cells,
                                                 XP *__restrict__ xnet) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= cells) xnet[c] = (XP)tl_lower_bound(skey, pins, (unsigned)c);
}

static unsigned hg_grid(int64_t count) { return (unsigned)((count + 255) / 256); }

// xnet_out / net_out of xpin / pin; *status_host != 0: a pin outside its range, and nothing was written.  The caller has
// begun the arena and checked the counts.
template <typename XP, typename CI>
static int hg_transpose(sbx_handle_t h, int64_t cells, int64_t nets, int64_t pins, const XP *xpin, const CI *pin, int base,
                        XP *xnet_out, CI *net_out, unsigned *status_host) {
  uint32_t *ka = nullptr, *kb = nullptr, *va = nullptr, *vb = nullptr, *skey = nullptr;
  *status_host = 0;
  if (pins) {
    unsigned *status = nullptr;
    SBX_TRY(sbx_salloc(h, 1, &status));
    SBX_HIP(h, hipMemsetAsync(status, 0, sizeof(unsigned), h->stream));
    SBX_TRY(sbx_salloc(h, (size_t)pins, &ka));
    SBX_TRY(sbx_salloc(h, (size_t)pins, &kb));
    SBX_TRY(sbx_salloc(h, (size_t)pins, &va));
    SBX_TRY(sbx_salloc(h, (size_t)pins, &vb));
    SBX_KLAUNCH(h, SBX_K_CSC, (k_hg_keys<XP, CI>), dim3(hg_grid(pins)), dim3(256), xpin, nets, pin, pins, base, cells, ka, va,
                status);
    SBX_LAUNCH_CHECK(h);
    SBX_TRY(sbx_readback(h, status_host, status, sizeof(unsigned)));
    if (*status_host) return SBX_OK;
    const int bits = sbx_bits_for((uint64_t)(cells - 1));
    if (pins <= sbx_cs::MAX_PAIRS) {
      SBX_TRY(sbx_salloc(h, (size_t)pins, &skey));
      const HgEmit<CI> emit = {skey, net_out};
      SBX_TRY(sbx_cs::sort_emit(h, SBX_K_CSC, ka, va, kb, vb, pins, bits, emit));
    } else {
      SBX_TRY(sbx_sort_pairs(h, &ka, &kb, &va, &vb, pins, 0, bits));
      SBX_KLAUNCH(h, SBX_K_CSC, k_hg_nets<CI>, dim3(hg_grid(pins)), dim3(256), (const uint32_t *)va, pins, net_out);
      skey = ka;
    }
  }
  SBX_KLAUNCH(h, SBX_K_CSC, k_hg_xnet<XP>, dim3(hg_grid(cells + 1)), dim3(256), (const uint32_t *)skey, pins, cells, xnet_out);
  SBX_LAUNCH_CHECK(h);
  SBX_PROF_BYTES(h, SBX_K_CSC, pins * (int64_t)(2 * sizeof(CI)) + (cells + nets) * (int64_t)sizeof(XP));
  return SBX_OK;
}

// ---- the formatters' jobs (tx_emit, sbx_text_emit.h)
template <typename XP, typename CI>
struct HgNetJob {
  const XP *xpin;
  const CI *pin;
  const void *wgt;
  const sbx_decrec *rec;  // TI_RECORD: of net r at [r - rb]
  int64_t rb, re, e0, items, delta;
  int weighted, vkind, vb, precision, no_last_nl;
  // net r has 1 + (its pins) items: the head, the pins.  key(r) = the first item of net r
  __device__ __forceinline__ int64_t key(int64_t r) const { return ((int64_t)xpin[r] - e0) + (r - rb); }
  __device__ __forceinline__ void locate(int64_t k, int64_t *row, int64_t *sub) const {
    int64_t lo = rb, hi = re - 1;  // the last net r in [rb, re) with key(r) <= k
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (key(mid) <= k) lo = mid;
      else hi = mid - 1;
    }
    *row = lo;
    *sub = k - key(lo);
  }
  __device__ __forceinline__ unsigned item(int64_t r, int64_t sub, char *dst) const {
    int o = 0;
    if (sub == 0) {
      if (weighted) o = dst ? tx_item_value_emit(vkind, vb, precision, wgt, rec, r, r - rb, dst)
                            : tx_item_value_length(vkind, vb, precision, wgt, rec, r, r - rb);
    } else {
      if (sub > 1 || weighted) {
        if (dst) dst[0] = ' ';
        o = 1;
      }
      const int64_t c = (int64_t)pin[(int64_t)xpin[r] + sub - 1] + delta;
      o += dst ? tx_emit_signed(c, dst + o) : tx_len_signed(c);
    }
    if (sub == (int64_t)xpin[r + 1] - (int64_t)xpin[r] && !(no_last_nl && r == re - 1)) {  // the net's last item
      if (dst) dst[o] = '\n';
      o++;
    }
    return (unsigned)o;
  }
};

struct HgWeightJob {
  const void *wgt;
  const sbx_decrec *rec;  // TI_RECORD: of value i at [i - begin]
  int64_t begin, items;
  int vkind, vb, precision;
  __device__ __forceinline__ void locate(int64_t k, int64_t *row, int64_t *sub) const {
    *row = begin + k;
    *sub = 0;
  }
  __device__ __forceinline__ unsigned item(int64_t i, int64_t, char *dst) const {
    int o = 0;
    if (i > 0) {
      if (dst) dst[0] = ' ';
      o = 1;
    }
    o += dst ? tx_item_value_emit(vkind, vb, precision, wgt, rec, i, i - begin, dst + o)
             : tx_item_value_length(vkind, vb, precision, wgt, rec, i, i - begin);
    return (unsigned)o;
  }
};
static_assert(1 + SBX_DEC_MAX_CHARS + 1 <= TX_LINE_MAX && 1 + 20 + 1 <= TX_LINE_MAX, "an item fits its LDS slot");

}  // namespace

static int hg_check_counts(sbx_handle_t h, const char *who, int64_t cells, int64_t nets, int64_t pins) {
  const int64_t lim = ((int64_t)1 << 31) - 1;
  if (cells >= lim || nets >= lim || pins >= lim)
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "%s: cells, nets and pins must be below 2^31 - 1", who);
  return SBX_OK;
}

extern "C" int sbhg_patoh_parse(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, const void *text_dev, int64_t bytes,
                                int64_t cells, int64_t nets, int64_t pins, int base, int scheme, int64_t capacity,
                                void *xpin_out, void *pin_out, void *xnet_out, void *net_out, void *net_wgt_out,
                                void *cell_wgt_out, int64_t *counts_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, counts_host && bytes >= 0 && (bytes == 0 || text_dev), "bad argument");
  counts_host[0] = counts_host[1] = counts_host[2] = 0;
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  const int vbytes = sbx_value_bytes(vt);
  SBX_REQUIRE(h, vbytes >= 0, "unknown value type");
  SBX_REQUIRE(h, cells >= 0 && nets >= 0 && pins >= 0 && capacity >= 0, "cells, nets, pins and capacity must not be negative");
  SBX_REQUIRE(h, base == 0 || base == 1, "base: 0 or 1");
  SBX_REQUIRE(h, scheme >= 0 && scheme <= 3, "scheme: 0..3");
  SBX_REQUIRE(h, capacity >= pins, "output capacity: pins ids");
  SBX_REQUIRE(h, xpin_out && (pins == 0 || pin_out), "xpin_out and pin_out are needed");
  SBX_REQUIRE(h, (xnet_out == nullptr) == (net_out == nullptr) || (pins == 0 && xnet_out), "xnet_out and net_out come as a pair");
  if (bytes >= ((int64_t)1 << 32))
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbhg_patoh_parse: texts of 4 GiB and more are not supported (32-bit token offsets)");
  SBX_TRY(hg_check_counts(h, "sbhg_patoh_parse", cells, nets, pins));
  const bool cells_weighted = (scheme & 1) != 0, nets_weighted = (scheme & 2) != 0;
  char *nwgt = vbytes ? (char *)net_wgt_out : nullptr, *cwgt = vbytes ? (char *)cell_wgt_out : nullptr;
  const bool wide_ids = it == SBX_I64, wide_offsets = it != SBX_I32;
  SBX_TRY(sbx_arena_begin(h));
  NestGuard guard(h);
  const char *text = (const char *)text_dev;
  unsigned *status = nullptr;  // [0] the status word, [1] the last line is the cell-weight line, [2] its tokens
  SBX_TRY(sbx_salloc(h, 3, &status));
  SBX_HIP(h, hipMemsetAsync(status, 0, 3 * sizeof(unsigned), h->stream));
  // (1) line starts and token starts
  unsigned lines = 0, tokens = 0;
  unsigned *line_off = nullptr, *tok_off = nullptr;
  SBX_TRY(tl_lines_and_tokens(h, text, bytes, &lines, &tokens, &line_off, &tok_off));
  // (2) per line: first token, pins, net or not; scans: first pin and net of every line
  unsigned *line_tok = nullptr, *line_ent = nullptr, *line_ncb = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)lines + 1, &line_tok));
  SBX_TRY(sbx_salloc(h, (size_t)lines + 1, &line_ent));
  SBX_TRY(sbx_salloc(h, (size_t)lines + 1, &line_ncb));
  SBX_KLAUNCH(h, SBX_K_MTX, k_hg_lines, dim3(mx_grid((int64_t)lines + 1)), dim3(MX_THREADS), text, bytes,
              (const unsigned *)line_off, (int64_t)lines, (const unsigned *)tok_off, (int64_t)tokens, cells_weighted ? 1 : 0,
              nets_weighted ? 1 : 0, line_tok, line_ent, line_ncb, status + 1, status);
  SBX_LAUNCH_CHECK(h);
  SBX_TRY(sbx_exclusive_scan_u32(h, line_ent, line_ent, (int64_t)lines + 1, nullptr));
  SBX_TRY(sbx_exclusive_scan_u32(h, line_ncb, line_ncb, (int64_t)lines + 1, nullptr));
  unsigned found = 0, net_lines = 0, st[3] = {0, 0, 0};
  SBX_TRY(sbx_readback(h, &found, line_ent + lines, sizeof(unsigned)));
  SBX_TRY(sbx_readback(h, &net_lines, line_ncb + lines, sizeof(unsigned)));
  SBX_TRY(sbx_readback(h, st, status, sizeof(st)));
  counts_host[0] = net_lines;
  counts_host[1] = found;
  counts_host[2] = st[2];
  if ((int64_t)net_lines != nets)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbhg_patoh_parse: the text has %u net lines, the header's nets is %lld%s", net_lines,
             (long long)nets,
             cells_weighted && !st[1] ? " (a cell-weight line is read only from a text that does not end in a newline)" : "");
  if (st[0] & HG_EMPTY_WEIGHTED)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbhg_patoh_parse: a net line of a net-weighted file has no weight");
  if ((int64_t)found != pins)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbhg_patoh_parse: the net lines hold %u pins, the header's pins is %lld", found,
             (long long)pins);
  if ((int64_t)st[2] > cells)
    SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbhg_patoh_parse: the last line holds %u cell weights, the header's cells is %lld", st[2],
             (long long)cells);
  // (3) offsets, default weights, then the tokens
  int32_t *xp = nullptr;
  SBX_TRY(sbx_salloc(h, (size_t)nets + 1, &xp));
  SBX_KLAUNCH(h, SBX_K_MTX, k_hg_xpin, dim3(mx_grid((int64_t)lines + 1)), dim3(MX_THREADS), (const unsigned *)line_ent,
              (const unsigned *)line_ncb, (int64_t)lines, xp);
  const uint64_t one = vt == SBX_V_F32 ? 0x3f800000ull : vt == SBX_V_F64 ? 0x3ff0000000000000ull : 1ull;
  if (nwgt && nets) {
    if (vbytes == 4) SBX_KLAUNCH(h, SBX_K_MTX, k_hg_fill<4>, dim3(mx_grid(nets)), dim3(MX_THREADS), nwgt, nets, one);
    else SBX_KLAUNCH(h, SBX_K_MTX, k_hg_fill<8>, dim3(mx_grid(nets)), dim3(MX_THREADS), nwgt, nets, one);
  }
  if (cwgt && cells) {
    if (vbytes == 4) SBX_KLAUNCH(h, SBX_K_MTX, k_hg_fill<4>, dim3(mx_grid(cells)), dim3(MX_THREADS), cwgt, cells, one);
    else SBX_KLAUNCH(h, SBX_K_MTX, k_hg_fill<8>, dim3(mx_grid(cells)), dim3(MX_THREADS), cwgt, cells, one);
  }
  SBX_LAUNCH_CHECK(h);
  int32_t *p32 = (int32_t *)pin_out;
  if (wide_ids && pins) SBX_TRY(sbx_salloc(h, (size_t)pins, &p32));
  if (tokens) {
    const int vkind = mx_value_kind(vt, vbytes != 0), vsigned = mx_value_signed(vt);
#define TOKENS(VK, VBX)                                                                                                  \
  SBX_KLAUNCH(h, SBX_K_MTX, (k_hg_tokens<VK, VBX>), dim3(mx_grid(tokens)), dim3(MX_THREADS), text, bytes,                  \
              (const unsigned *)tok_off, (int64_t)tokens, (const unsigned *)line_off, (int64_t)lines,                      \
              (const unsigned *)line_tok, (const unsigned *)line_ent, (const unsigned *)line_ncb,                          \
              (const unsigned *)(status + 1), nets_weighted ? 1 : 0, base, cells, nets, pins, vsigned, p32, nwgt, cwgt,    \
              status)
    MX_FOR_VALUE_KIND(vkind, vbytes, TOKENS);
#undef TOKENS
    SBX_LAUNCH_CHECK(h);
    SBX_PROF_BYTES(h, SBX_K_MTX, bytes + pins * (int64_t)4);
    SBX_TRY(sbx_readback(h, st, status, sizeof(unsigned)));
    if (st[0] & HG_PIN_RANGE)
      SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbhg_patoh_parse: a pin outside [%d, %lld]", base, (long long)(cells + base - 1));
    if (st[0])
      SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbhg_patoh_parse: malformed %s (a complete decimal integer is needed)",
               (st[0] & HG_BAD_PIN) && (st[0] & HG_BAD_WEIGHT) ? "pin and weight tokens"
               : (st[0] & HG_BAD_PIN)                          ? "pin token"
                                                               : "weight token");
  }
  // (4) the cell -> net side
  int32_t *xn = nullptr;
  if (xnet_out) {
    int32_t *n32 = (int32_t *)net_out;
    SBX_TRY(sbx_salloc(h, (size_t)cells + 1, &xn));
    if (wide_ids && pins) SBX_TRY(sbx_salloc(h, (size_t)pins, &n32));
    unsigned tst = 0;
    SBX_TRY((hg_transpose<int32_t, int32_t>(h, cells, nets, pins, xp, p32, base, xn, n32, &tst)));
    if (tst) SBX_FAIL(h, SBX_ERR_INTERNAL, "sbhg_patoh_parse: a checked pin is out of range");
    if (wide_ids && pins) SBX_TRY(sbx_widen_i32(h, n32, net_out, pins));
  }
  if (wide_ids && pins) SBX_TRY(sbx_widen_i32(h, p32, pin_out, pins));
  if (wide_offsets) {
    SBX_TRY(sbx_widen_i32(h, xp, xpin_out, nets + 1));
    if (xn) SBX_TRY(sbx_widen_i32(h, xn, xnet_out, cells + 1));
  } else {
    SBX_HIP(h, hipMemcpyAsync(xpin_out, xp, (size_t)(nets + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    if (xn) SBX_HIP(h, hipMemcpyAsync(xnet_out, xn, (size_t)(cells + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  }
  return SBX_OK;
}

template <typename XP, typename CI>
static int hg_cells_to_nets_typed(sbx_handle_t h, int64_t cells, int64_t nets, const XP *xpin, const CI *pin, int base,
                                  XP *xnet_out, CI *net_out) {
  int64_t pins = 0;
  if (nets) {
    int64_t ends[2] = {0, 0};
    bool desc = false;
    SBX_TRY(tx_range_ends<XP>(h, xpin, 0, nets, ends, &desc));
    if (desc || ends[0] != 0) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbhg_cells_to_nets: xpin descends or does not start at 0");
    pins = ends[1];
  }
  SBX_TRY(hg_check_counts(h, "sbhg_cells_to_nets", cells, nets, pins));
  SBX_REQUIRE(h, pins == 0 || (pin && net_out), "pin and net_out are needed");
  SBX_REQUIRE(h, pins == 0 || cells > 0, "pins without cells");
  unsigned st = 0;
  SBX_TRY((hg_transpose<XP, CI>(h, cells, nets, pins, xpin, pin, base, xnet_out, net_out, &st)));
  if (st) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbhg_cells_to_nets: a pin outside [%d, %lld]", base, (long long)(cells + base - 1));
  return SBX_OK;
}

extern "C" int sbhg_cells_to_nets(sbx_handle_t h, sbx_index_type it, int64_t cells, int64_t nets, const void *xpin,
                                  const void *pin, int base, void *xnet_out, void *net_out) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  SBX_REQUIRE(h, cells >= 0 && nets >= 0, "cells and nets must not be negative");
  SBX_REQUIRE(h, base == 0 || base == 1, "base: 0 or 1");
  SBX_REQUIRE(h, xnet_out && (nets == 0 || xpin), "xpin and xnet_out are needed");
  SBX_TRY(hg_check_counts(h, "sbhg_cells_to_nets", cells, nets, 0));
  SBX_TRY(sbx_arena_begin(h));
  NestGuard guard(h);
  if (it == SBX_I64)
    return hg_cells_to_nets_typed<int64_t, int64_t>(h, cells, nets, (const int64_t *)xpin, (const int64_t *)pin, base,
                                                    (int64_t *)xnet_out, (int64_t *)net_out);
  if (it == SBX_I32_N64)
    return hg_cells_to_nets_typed<int64_t, int32_t>(h, cells, nets, (const int64_t *)xpin, (const int32_t *)pin, base,
                                                    (int64_t *)xnet_out, (int32_t *)net_out);
  return hg_cells_to_nets_typed<int32_t, int32_t>(h, cells, nets, (const int32_t *)xpin, (const int32_t *)pin, base,
                                                  (int32_t *)xnet_out, (int32_t *)net_out);
}

template <typename XP, typename CI>
static int hg_format_typed(sbx_handle_t h, HgNetJob<XP, CI> job, void *text_out, int64_t capacity, int64_t *bytes_host) {
  // the ends of the range, and that the offsets between them ascend (the item search relies on it)
  int64_t hends[2] = {0, 0};
  bool hdesc = false;
  SBX_TRY(tx_range_ends<XP>(h, job.xpin, job.rb, job.re, hends, &hdesc));
  if (hdesc) SBX_FAIL(h, SBX_ERR_BAD_ARG, "sbhg_patoh_format: xpin descends inside the net range");
  const int64_t rows = job.re - job.rb;
  job.e0 = hends[0];
  job.items = (hends[1] - hends[0]) + rows;
  if (job.items >= ((int64_t)1 << 32))
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbhg_patoh_format: 2^32 items and more in one call (pass the nets in sub-ranges)");
  if (job.weighted && job.vkind == TI_RECORD) {
    sbx_decrec *rec = nullptr;
    SBX_TRY(tx_records(h, (const char *)job.wgt + job.rb * (int64_t)job.vb, nullptr, rows, job.vb, job.precision, &rec));
    job.rec = rec;
  }
  return tx_emit(h, "sbhg_patoh_format", job, job.items * (int64_t)4, text_out, capacity, bytes_host);
}

extern "C" int sbhg_patoh_format(sbx_handle_t h, sbx_index_type it, sbx_value_type vt, int64_t net_begin, int64_t net_end,
                                 const void *xpin, const void *pin, const void *net_wgt, int64_t index_delta, int precision,
                                 unsigned flags, void *text_out, int64_t capacity, int64_t *bytes_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, bytes_host && capacity >= 0, "bad argument");
  SBX_REQUIRE(h, it == SBX_I32 || it == SBX_I64 || it == SBX_I32_N64, "unknown index type");
  SBX_REQUIRE(h, net_begin >= 0 && net_end >= net_begin, "net range");
  SBX_REQUIRE(h, precision >= 1 && precision <= 17, "precision: 1..17");
  SBX_REQUIRE(h, (flags & ~(SBHG_NET_WEIGHTS | SBHG_NO_LAST_NEWLINE)) == 0, "unknown flag");
  const int vbytes = sbx_value_bytes(vt);
  SBX_REQUIRE(h, vbytes >= 0, "unknown value type");
  const bool weighted = (flags & SBHG_NET_WEIGHTS) != 0;
  SBX_REQUIRE(h, !weighted || (net_wgt && vt != SBX_V_NONE), "SBHG_NET_WEIGHTS needs values");
  *bytes_host = 0;
  SBX_TRY(sbx_arena_begin(h));
  if (net_end == net_begin) return SBX_OK;
  SBX_REQUIRE(h, xpin, "xpin is needed");
  NestGuard guard(h);
#define HG_JOB(XP, CI)                                             \
  HgNetJob<XP, CI> job = {};                                       \
  job.xpin = (const XP *)xpin;                                     \
  job.pin = (const CI *)pin;                                       \
  job.wgt = net_wgt;                                               \
  job.rb = net_begin;                                              \
  job.re = net_end;                                                \
  job.delta = index_delta;                                         \
  job.weighted = weighted ? 1 : 0;                                 \
  job.vkind = tx_item_kind(vt);                                   \
  job.vb = vbytes;                                                 \
  job.precision = precision;                                       \
  job.no_last_nl = (flags & SBHG_NO_LAST_NEWLINE) ? 1 : 0;         \
  return hg_format_typed<XP, CI>(h, job, text_out, capacity, bytes_host)
  if (it == SBX_I64) {
    HG_JOB(int64_t, int64_t);
  }
  if (it == SBX_I32_N64) {
    HG_JOB(int64_t, int32_t);
  }
  HG_JOB(int32_t, int32_t);
#undef HG_JOB
}

extern "C" int sbhg_patoh_format_weights(sbx_handle_t h, sbx_value_type vt, int64_t begin, int64_t end, const void *wgt,
                                         int precision, void *text_out, int64_t capacity, int64_t *bytes_host) {
  if (!h) return SBX_ERR_BAD_ARG;
  SBX_REQUIRE(h, bytes_host && capacity >= 0, "bad argument");
  SBX_REQUIRE(h, begin >= 0 && end >= begin, "value range");
  SBX_REQUIRE(h, precision >= 1 && precision <= 17, "precision: 1..17");
  const int vbytes = sbx_value_bytes(vt);
  SBX_REQUIRE(h, vbytes > 0, "a value type is needed");
  *bytes_host = 0;
  SBX_TRY(sbx_arena_begin(h));
  if (end == begin) return SBX_OK;
  SBX_REQUIRE(h, wgt, "wgt is needed");
  if (end - begin >= ((int64_t)1 << 32))
    SBX_FAIL(h, SBX_ERR_UNSUPPORTED, "sbhg_patoh_format_weights: 2^32 values and more in one call (pass them in sub-ranges)");
  NestGuard guard(h);
  HgWeightJob job = {};
  job.wgt = wgt;
  job.begin = begin;
  job.items = end - begin;
  job.vkind = tx_item_kind(vt);
  job.vb = vbytes;
  job.precision = precision;
  if (job.vkind == TI_RECORD) {
    sbx_decrec *rec = nullptr;
    SBX_TRY(tx_records(h, (const char *)wgt + begin * (int64_t)vbytes, nullptr, job.items, vbytes, precision, &rec));
    job.rec = rec;
  }
  return tx_emit(h, "sbhg_patoh_format_weights", job, job.items * (int64_t)4, text_out, capacity, bytes_host);
}
