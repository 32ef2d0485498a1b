// sbx_internal.h — handle, scratch arena and launch helpers shared by the HIP
// translation units of libsbx.  gfx950 (MI355X) only: wave64, 160 KiB LDS/CU.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "sbx.h"

#define SBX_WAVE 64

// kernel groups for the optional HIP-event profiler (sbx_profile_*)
enum sbx_kernel_id {
  SBX_K_SCAN = 0,
  SBX_K_RADIX_HIST,
  SBX_K_RADIX_SCATTER,
  SBX_K_COO_TO_CSR,
  SBX_K_CSR_TO_COO,
  SBX_K_PERMUTE_TILE,
  SBX_K_PERMUTE_LONG,
  SBX_K_PERMUTE_BLOCK,
  SBX_K_PERMUTE_PREP,
  SBX_K_BFS_EXPAND,
  SBX_K_BFS_HEAVY,
  SBX_K_BFS_BOTTOMUP,
  SBX_K_BFS_SMALL,
  SBX_K_LEVEL_ORDER,
  SBX_K_CC,
  SBX_K_RCM_SMALL,
  SBX_K_RCM_MISC,
  SBX_K_GRAY,
  SBX_K_DEGREE,
  SBX_K_CHECK,
  SBX_K_CSC,
  SBX_K_FEATURE,
  SBX_K_MTX,
  SBX_K_MISC,
  SBX_K_TEXT_FORMAT,
  SBX_K_TEXT_LONG,
  SBX_K_TEXT_WRITE,
  SBX_K_TEXT_CHECK,
  SBX_K_SPMV,
  SBX_K_SPMM,
  SBX_K_SDDMM,
  SBX_K_SOFTMAX,
  SBX_K_SPMM_T,
  SBX_K_COUNT
};
extern const char *const sbx_kernel_names[SBX_K_COUNT];

struct sbx_prof_rec {
  int kid;
  hipEvent_t start, stop;
};

struct sbx_block {
  char *ptr;
  size_t cap;
};

#define SBX_AUX_STREAMS 7  /* permute: [0] row classes (serial mode) / class 0, [1] long rows, [2..6] classes 1..5 */

struct sbx_handle_s {
  int device;
  hipStream_t stream;
  // grow-only scratch arena: a list of device blocks, bump-allocated per call.
  // After a call that needed more than one block the arena is consolidated
  // into a single block, so steady-state calls never reach hipMalloc.
  std::vector<sbx_block> blocks;
  size_t cur_block;
  size_t cur_off;
  size_t call_bytes;  // bytes handed out during the current call
  size_t high_water;
  int nest;  // > 0 while an API entry point calls another one: the arena is not rewound
  void *pinned;  // small pinned host buffer for device->host read-backs
  size_t pinned_bytes;
  // pool of pre-zeroed (digit histogram + ticket) slots for the radix sort: one memset per
  // SBX_RS_SLOTS sorts instead of one per sort (every memset is a launch on the critical path)
  void *rs_pool;
  int rs_next;
  void *pow5;       // device table of 5^k for the exact decimal conversion (sbx_mtx.hip), built on first use
  unsigned rb_seq;  // sequence number of the last polled read-back (sbx_readback)
  sbx_oom_hook oom_hook;  // asked once when a device allocation of the library's own fails (sbx_set_oom_hook)
  void *oom_user;
  int rcm_gb_backoff;  // RCM calls left to run without the persistent (grid-barrier) kernels after one of them gave up
  int num_cus;
  // side streams for independent stages of one call (permute: tile / block-row / long-row paths), created on
  // first use; aux_event[0] marks the fork point on `stream`, [1 + i] the end of side stream i
  hipStream_t aux_stream[SBX_AUX_STREAMS];
  hipEvent_t aux_event[SBX_AUX_STREAMS + 1];
  bool aux_ready;
  bool aux_dirty;     // a fork onto the side streams is open: set at the fork, cleared by the join (sbx_aux_scope)
  bool rs_tied_hint;  // set around a sort whose keys are heavily tied (Gray's composite keys): k_onesweep_hist aggregates per wave
  void *rs_override;  // next radix sort takes this zeroed slot instead of one from the pool (sorts on a side stream
                      // must not share the pool with the main stream: the pool is re-zeroed in stream order)
  // profiler: when on, every kernel launch is bracketed by HIP events on the
  // handle's stream; sbx_profile_query drains them into the accumulators
  bool prof_on;
  std::vector<sbx_prof_rec> prof_pending;
  std::vector<hipEvent_t> prof_pool;
  double prof_ms[SBX_K_COUNT];
  long long prof_launches[SBX_K_COUNT];
  long long prof_bytes[SBX_K_COUNT];  // algorithmic bytes declared by the launch sites (sbx_prof_bytes)
  char err[512];
};

int sbx_aux_streams(sbx_handle_t h);  // creates aux_stream / aux_event if needed
// joins every side stream back into `main_stream` (an event behind whatever each one holds, waited for by `main_stream`)
// and clears aux_dirty: what a call does that leaves between a fork and its join
void sbx_aux_join(sbx_handle_t h, hipStream_t main_stream);
// Held by every function that is the outermost one to fork work onto the side streams: whichever way the call leaves it
// — the end, SBX_TRY, SBX_FAIL, a successful early return — a fork that is still open (aux_dirty) is joined into the
// caller's stream first, and h->stream is the caller's again.  The joins on the paths that succeed stay where they are
// (they clear aux_dirty); this is the net under all the others.
struct sbx_aux_scope {
  sbx_handle_t h;
  hipStream_t main_stream;
  explicit sbx_aux_scope(sbx_handle_t h_) : h(h_), main_stream(h_->stream) {}
  ~sbx_aux_scope() {
    h->stream = main_stream;
    if (h->aux_dirty) sbx_aux_join(h, main_stream);
  }
  sbx_aux_scope(const sbx_aux_scope &) = delete;
  sbx_aux_scope &operator=(const sbx_aux_scope &) = delete;
};
// Work enqueued on a side stream: h->stream is that stream while the guard lives and the previous one again on every
// way out of its block, so the launches inside go through SBX_KLAUNCH / SBX_HIP / SBX_TRY like any others.  (The fork
// and join events, and aux_dirty, stay with the caller.)
struct sbx_stream_scope {
  sbx_handle_t h;
  hipStream_t prev;
  sbx_stream_scope(sbx_handle_t h_, hipStream_t side) : h(h_), prev(h_->stream) { h->stream = side; }
  ~sbx_stream_scope() { h->stream = prev; }
  sbx_stream_scope(const sbx_stream_scope &) = delete;
  sbx_stream_scope &operator=(const sbx_stream_scope &) = delete;
};
// A sort whose keys are heavily tied: h->rs_tied_hint is set while the guard lives and clear again on every way out of
// its block (the only assignments to the flag besides sbx_create's).
struct sbx_tied_hint_scope {
  sbx_handle_t h;
  explicit sbx_tied_hint_scope(sbx_handle_t h_) : h(h_) { h->rs_tied_hint = true; }
  ~sbx_tied_hint_scope() { h->rs_tied_hint = false; }
  sbx_tied_hint_scope(const sbx_tied_hint_scope &) = delete;
  sbx_tied_hint_scope &operator=(const sbx_tied_hint_scope &) = delete;
};
void sbx_prof_begin(sbx_handle_t h, int kid);
void sbx_prof_end(sbx_handle_t h);

// every kernel launch of the library goes through this macro
#define SBX_KLAUNCH(h, kid, kernel, grid, block, ...)                        \
  do {                                                                       \
    if ((h)->prof_on) sbx_prof_begin((h), (kid));                            \
    hipLaunchKernelGGL(kernel, grid, block, 0, (h)->stream, __VA_ARGS__);    \
    if ((h)->prof_on) sbx_prof_end((h));                                     \
  } while (0)

// algorithmic bytes of the launches just issued for kernel group `kid` (profiling runs only)
#define SBX_PROF_BYTES(h, kid, bytes)                          \
  do {                                                         \
    if ((h)->prof_on) (h)->prof_bytes[(kid)] += (long long)(bytes); \
  } while (0)

#define SBX_FAIL(h, code, ...)                       \
  do {                                               \
    snprintf((h)->err, sizeof((h)->err), __VA_ARGS__); \
    return (code);                                   \
  } while (0)

#define SBX_HIP(h, expr)                                                                  \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      snprintf((h)->err, sizeof((h)->err), "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,  \
               hipGetErrorString(e_));                                                    \
      return e_ == hipErrorOutOfMemory ? SBX_ERR_OOM : SBX_ERR_HIP;                       \
    }                                                                                     \
  } while (0)

#define SBX_TRY(expr)            \
  do {                           \
    int rc_ = (expr);            \
    if (rc_ != SBX_OK) return rc_; \
  } while (0)

#define SBX_LAUNCH_CHECK(h) SBX_HIP(h, hipGetLastError())

// an argument check of an entry point: the message carries the entry point's name
#define SBX_REQUIRE(h, cond, msg)                                       \
  do {                                                                  \
    if (!(cond)) SBX_FAIL(h, SBX_ERR_BAD_ARG, "%s: %s", __func__, msg); \
  } while (0)

// an entry point that calls other entry points: the arena is not rewound while one of these lives
struct NestGuard {
  sbx_handle_t h;
  explicit NestGuard(sbx_handle_t h) : h(h) { h->nest++; }
  ~NestGuard() { h->nest--; }
};

// ---- arena -----------------------------------------------------------------
int sbx_arena_begin(sbx_handle_t h);  // start of an API call: rewinds (and consolidates)
int sbx_arena_alloc(sbx_handle_t h, size_t bytes, void **out);

template <typename T>
static inline int sbx_salloc(sbx_handle_t h, size_t count, T **out) {
  void *p = nullptr;
  int rc = sbx_arena_alloc(h, count * sizeof(T), &p);
  *out = (T *)p;
  return rc;
}

#define SBX_RS_SLOTS 32
#define SBX_RS_SLOT_BYTES (8 * 256 * 8 + 256)  /* RS_MAX_PASSES x 256 u64 counts + tickets */
// next zeroed radix slot (device pointer); re-zeroes the pool in stream order when it wraps
int sbx_radix_slot(sbx_handle_t h, void **slot);

// blocking read-back of `bytes` (<= pinned buffer) from device memory
int sbx_readback(sbx_handle_t h, void *dst_host, const void *src_dev, size_t bytes);

// ---- environment switches ------------------------------------------------------------------------------------------------
// What the test-suite needs to reach a code path that production takes only under conditions a test cannot arrange (a
// grid barrier giving up, a level beyond a size limit, every row on the radix fallback).  Every switch selects code that
// also runs without it.  sbx_sw() (sbx_handle.hip, the library's one reader of the environment) fills the table on first
// use: once per process.  Tuning constants and timing ablations are compile-time macros instead (#ifndef NAME / #define
// NAME <default> where they are used), set in a variant build: tools/build_variant.py <name> <file.hip> -DNAME=...

// limits of RCM's tie walk (sbx_rcm.hip: k_ubfs_ties_small) and polls a grid barrier waits: the defaults of the switches
// that lower them
constexpr unsigned TS_CAP = 1024, TS_EDGES = 1u << 17;
constexpr unsigned TS_SINGLE = 1u << 13;  // entries of a smallest-member step the one workgroup still scans itself
constexpr unsigned GB_SPINS = 1u << 16;

struct sbx_switches {
  // RCM (sbx_rcm.hip, sbx_rcm64.hip)
  bool rcm_split_expand;     // SBX_RCM_SPLIT_EXPAND, on; 0: a wide frontier's light rows are expanded in line
  bool rcm_cc_overlap;       // SBX_RCM_CC_OVERLAP, on; 0: the labelling of the other components runs in line
  bool rcm_overlap;          // SBX_RCM_OVERLAP, on; 0: the degree ranks run in line instead of on a side stream
  bool rcm_count_sort;       // SBX_RCM_COUNT_SORT, on; 0: levels above 4096 vertices take the generic radix sort
  bool rcm_ranked_keys;      // SBX_RCM_RANKED_KEYS, on; 0: big Cuthill-McKee levels sort full (parent position, rank) keys
  bool rcm_unordered;        // SBX_RCM_UNORDERED, on; 0: every sweep of the search keeps the order inside its levels
  int rcm_ubfs_chain;        // SBX_RCM_UBFS_CHAIN, 3 (clamped to 0 ... 8); 0: unordered sweeps run the per-level loop
  bool rcm_tie_walk;         // SBX_RCM_TIE_WALK, on; 0: every tie-break through the persistent cone kernels
  bool rcm_tie_spec;         // SBX_RCM_TIE_SPEC, on; 0: the host reads back behind every tie walk before the next sweep
  bool rcm_head_chain;       // SBX_RCM_HEAD_CHAIN, on; 0: a read-back between the first sweep's head run and its chain
  bool rcm_bu_blocks;        // SBX_RCM_BU_BLOCKS, on; 0: the bottom-up kernels that give a lane to every vertex
  double bu_ratio;           // SBX_DEBUG_BU_RATIO, 4: frontier / unvisited edges above which an ordered level goes bottom-up
  int gb_backoff;            // SBX_DEBUG_GB_BACKOFF, 16: calls kept off the persistent kernels after a barrier gave up
  unsigned gb_spins;         // SBX_DEBUG_GB_SPINS, GB_SPINS: polls a grid barrier waits before it gives up (tests: 0)
  int rcm_ranked_div;        // SBX_DEBUG_RCM_RANKED_DIV, 3 (at least 1): ranked keys from levels of n_ranked / this
  unsigned ub_max_levels;    // SBX_DEBUG_UB_MAX_LEVELS, 64: deeper sweeps fall back to the ordered kind
  unsigned tie_edges;        // SBX_DEBUG_TIE_EDGES, TS_EDGES (at most): the tie walk's edge limit, lowered
  unsigned tie_single;       // SBX_DEBUG_TIE_SINGLE, TS_SINGLE (at most): entries above which a step goes to the grid
  unsigned tie_cap;          // SBX_DEBUG_TIE_CAP, TS_CAP (at most): members of a level the tie walk takes
  bool tie_walk_debug;       // SBX_DEBUG_TIE_WALK, off; set at all: the walk's exit is printed, no speculative sweep
  bool rcm_level_paths;      // SBX_DEBUG_RCM_LEVEL_PATHS, off; set at all: run_bfs prints how it orders each level above 4096
  bool rcm_check;            // SBX_DEBUG_RCM_CHECK, off; non-zero: every unordered sweep is checked, its trace printed
  bool chain_tail_abort;     // SBX_DEBUG_CHAIN_TAIL_ABORT, off; non-zero: a chain's tail run gives up at once
  // Permute2D and CSR row sort (sbx_permute.hip)
  bool permute_overlap;      // SBX_PERMUTE_OVERLAP, on; 0: tile, block-row and long-row paths back to back on one stream
  bool permute_force_radix;  // SBX_PERMUTE_FORCE_RADIX, off; bit 0 set: every tile / row takes the radix path
  bool permute_no_tile2;     // SBX_PERMUTE_NO_TILE2, off; set at all: k_permute_tile where k_permute_tile2 would run
  // Gray ordering (sbx_gray_order.hip)
  bool gray_three_sorts;     // SBX_GRAY_ORDER_THREE_SORTS, off; non-zero: three sorts even where one 64-bit key does
};
const sbx_switches &sbx_sw();

// bits of a Gray key: the resolution, clamped to the number of columns (gray_reorder.cc:206-208) — the key stage and the
// ordering stage must agree on it
static inline int sbx_gray_bits(int resolution, int64_t m) { return m < resolution ? (int)m : resolution; }

static inline int sbx_value_bytes(sbx_value_type vt) {
  switch (vt) {
    case SBX_V_NONE: return 0;
    case SBX_V_I32: case SBX_V_U32: case SBX_V_F32: return 4;
    case SBX_V_I64: case SBX_V_U64: case SBX_V_F64: return 8;
  }
  return -1;
}
static inline int sbx_index_bytes(sbx_index_type it) { return it == SBX_I32 ? 4 : 8; }

static inline int sbx_bits_for(uint64_t max_value) {  // bits needed to represent values 0..max_value
  int b = 0;
  while (max_value) { b++; max_value >>= 1; }
  return b;
}

static inline unsigned sbx_grid_for(int64_t work_items, int per_block, int64_t cap) {
  int64_t g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

// ---- primitives implemented in sbx_prims.hip --------------------------------
// exclusive prefix sum; in == out allowed.  If total_out != nullptr the grand
// total is stored there (device pointer).  T in {int32,int64,uint32,uint64}.
int sbx_exclusive_scan_i32(sbx_handle_t h, const int32_t *in, int32_t *out, int64_t count,
                           int32_t *total_out);
int sbx_exclusive_scan_i64(sbx_handle_t h, const int64_t *in, int64_t *out, int64_t count,
                           int64_t *total_out);
int sbx_exclusive_scan_u32(sbx_handle_t h, const uint32_t *in, uint32_t *out, int64_t count,
                           uint32_t *total_out);

// stable sort of every segment [seg_ptr[i], seg_ptr[i+1]) of (32-bit key < key_limit, vb-byte value) pairs by key, out
// of place (sbx_permute.hip: the permute's LDS sort stage with identity maps); the caller has begun the arena
int sbx_sort_segments(sbx_handle_t h, int vb, int64_t nseg, int64_t key_limit, int64_t nnz, const int32_t *seg_ptr,
                      const int32_t *key_in, const char *val_in, int32_t *key_out, char *val_out);

// A radix pass covers key bits [shift, shift+bits), bits <= 8.
struct sbx_radix_pass {
  int shift;
  int bits;
};
// builds the pass list for significant bit ranges [lo0,hi0) u [lo1,hi1) (second may be empty)
int sbx_radix_plan(int lo0, int hi0, int lo1, int hi1, sbx_radix_pass *passes /*>=16*/);

// Stable LSD radix sort.  keys_a/vals_a hold the input; *_b are same-sized
// temporaries.  payload_bytes in {0,4,8}; key_bytes in {4,8}.  On return
// *result_in_b tells which buffer holds the sorted sequence.
int sbx_radix_sort(sbx_handle_t h, int key_bytes, int payload_bytes, void *keys_a, void *keys_b,
                   void *vals_a, void *vals_b, int64_t count, const sbx_radix_pass *passes,
                   int num_passes, int *result_in_b);

// The same sort over the key bits [lo0,hi0) u [lo1,hi1) of ping-pong buffers: on return *keys_a / *vals_a hold the
// sorted records and *keys_b / *vals_b the other buffers (vals_a = vals_b = nullptr without a payload).  With
// count < 2 or no bit to sort by it returns at once and touches nothing.
int sbx_sort_pairs(sbx_handle_t h, int key_bytes, int payload_bytes, void **keys_a, void **keys_b, void **vals_a,
                   void **vals_b, int64_t count, int lo0, int hi0, int lo1, int hi1);
// (typed fronts: the record sizes come from the buffers' own types)
template <typename K, typename V>
inline int sbx_sort_pairs(sbx_handle_t h, K **ka, K **kb, V **va, V **vb, int64_t count, int lo0, int hi0, int lo1 = 0,
                          int hi1 = 0) {
  return sbx_sort_pairs(h, (int)sizeof(K), (int)sizeof(V), (void **)ka, (void **)kb, (void **)va, (void **)vb, count, lo0,
                        hi0, lo1, hi1);
}
template <typename K>
inline int sbx_sort_keys(sbx_handle_t h, K **ka, K **kb, int64_t count, int lo0, int hi0, int lo1 = 0, int hi1 = 0) {
  return sbx_sort_pairs(h, (int)sizeof(K), 0, (void **)ka, (void **)kb, nullptr, nullptr, count, lo0, hi0, lo1, hi1);
}

// The same sort reading its records from, and leaving them in, the caller's own arrays: the first pass loads from
// `src`, the last one stores to `dst` (which may be the arrays of `src`: needs num_passes >= 2), the passes between
// use (keys_a, vals_a) / (keys_b, vals_b) — no pack kernel before and no unpack kernel behind the sort.  A side is
//   k_split: a 64-bit key kept as two 32-bit arrays, k[0] = low word, k[1] = high word (else k[0] = the key array)
//   p_split: a 64-bit payload kept as two 32-bit arrays, p[0] = low, p[1] = high    (else p[0] = the payload array)
// Supported: k_split with 8-byte keys (payload 0 / 4 / 8 bytes, not split), p_split with 4-byte keys and 8-byte payloads.
struct sbx_radix_side {
  void *k[2];
  void *p[2];
  bool k_split, p_split;
};
int sbx_radix_sort_io(sbx_handle_t h, int key_bytes, int payload_bytes, const sbx_radix_side *src, void *keys_a,
                      void *keys_b, void *vals_a, void *vals_b, const sbx_radix_side *dst, int64_t count,
                      const sbx_radix_pass *passes, int num_passes);

// Same sort of 64-bit keys without payload (count >= 2, num_passes >= 1) whose final pass, instead of storing the
// sorted keys, emits per key at sorted position p: value = map ? map[low32(key)] : low32(key); out[p] = value;
// bit `value` set in bits_a / bits_b (each optional); pos_of[value] = p (optional).
struct sbx_radix_emit {
  const uint32_t *map;
  uint32_t *out;
  unsigned *bits_a, *bits_b;
  unsigned *pos_of;
  uint32_t low_mask;  // low32(key) is ANDed with this first (0: all 32 bits) — keys whose fields are packed tightly
};
int sbx_radix_sort_emit(sbx_handle_t h, void *keys_a, void *keys_b, int64_t count, const sbx_radix_pass *passes,
                        int num_passes, const sbx_radix_emit *emit);

int sbx_fill_i32(sbx_handle_t h, int32_t *dst, int32_t value, int64_t count);

// the handle's device table of 5^k limbs and Eisel-Lemire significands (sbx_dec2bin.h: SBX_TABLE_WORDS words), built on
// first use (sbx_mtx.hip); the parsers and the text formatters (sbx_text.hip) share it
int sbx_pow5_table(sbx_handle_t h, const uint64_t **out);

// degree ranks of the non-empty rows, (degree, id) ascending, both ways (sbx_degree.hip; for the RCM's Cuthill-McKee keys);
// n_top = rows of 255 entries and more; enqueued on h->stream, scratch from the running call's arena, no read-back
int sbx_degree_ranks(sbx_handle_t h, sbx_index_type it, const void *rp, int64_t n, int64_t n_nonempty, int64_t n_top,
                     unsigned max_deg, uint32_t *rank, uint32_t *order);

// ---- 64-bit index arrays (sbx_i64.hip): narrowed to the int32 kernels when every value fits
struct sbx_narrowed {
  int32_t *ptr;  // int32 copy in the arena (nullptr if the source was nullptr)
};
int sbx_narrow_i64(sbx_handle_t h, const void *src_i64, int64_t count, int32_t **out, int *overflow_flag_dev);
int sbx_widen_i32(sbx_handle_t h, const int32_t *src, void *dst_i64, int64_t count);
int sbx_i64_begin(sbx_handle_t h, int **overflow_flag_dev);          // arena_begin + nesting on
int sbx_i64_check(sbx_handle_t h, const int *overflow_flag_dev);     // synchronous overflow check
void sbx_i64_end(sbx_handle_t h);
int sbx_i64_coo_sort(sbx_handle_t h, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, void *row, void *col,
                     void *val);
int sbx_i64_mtx_parse_coordinate(sbx_handle_t h, sbx_value_type vt, const void *text_dev, int64_t bytes, int64_t n_rows,
                                 int64_t n_cols, int64_t entries, int fields, int symmetry, unsigned flags,
                                 int64_t capacity, void *row_out, void *col_out, void *val_out, int64_t *nnz_host);
int sbx_i64_edge_list_parse(sbx_handle_t h, sbx_value_type vt, const void *text_dev, int64_t bytes, int64_t entries,
                            int weighted, unsigned flags, int64_t capacity, void *row_out, void *col_out, void *val_out,
                            int64_t *dims_nnz_host);
int sbx_fill_i64(sbx_handle_t h, int64_t *dst, int64_t value, int64_t count);

// ---- SBX_I32_N64 (32-bit ids, 64-bit offsets): adapters of the entry points whose offsets are 32-bit inside (sbx_i64.hip)
int sbx_mixed_csr_rows_sorted(sbx_handle_t h, int64_t n, const void *row_ptr, const void *col, int *sorted_host);
int sbx_mixed_csr_sort_rows(sbx_handle_t h, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, const void *row_ptr,
                            void *col, void *val);
int sbx_mixed_coo_to_csc(sbx_handle_t h, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, const void *row,
                         const void *col, const void *val, void *col_ptr_out, void *row_out, void *val_out);
int sbx_mixed_csr_to_csc(sbx_handle_t h, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, const void *row_ptr,
                         const void *col, const void *val, void *col_ptr_out, void *row_out, void *val_out);
int sbx_mixed_csr_bandwidth(sbx_handle_t h, int64_t n, int64_t nnz, const void *row_ptr, const void *col,
                            int64_t *bandwidth_host);
int sbx_mixed_csr_profile(sbx_handle_t h, int64_t n, int64_t nnz, const void *row_ptr, const void *col,
                          int64_t *profile_host);
int sbx_mixed_rcm_reorder(sbx_handle_t h, int64_t n, int64_t nnz, const void *row_ptr, const void *col, void *inv_perm_out,
                          sbx_rcm_stats *stats_host);
int sbx_mixed_gray_row_keys(sbx_handle_t h, int64_t n, int64_t m, int64_t nnz, const void *row_ptr, const void *col,
                            int resolution, int nnz_threshold, void *degree_out, uint64_t *key_out, int64_t *counts_host);
int sbx_mixed_gray_reorder(sbx_handle_t h, int64_t n, int64_t m, int64_t nnz, const void *row_ptr, const void *col,
                           int resolution, int nnz_threshold, int group_size, int exact_ties, void *inv_perm_out);
int sbx_mixed_permute_csr_rows(sbx_handle_t h, sbx_value_type vt, int64_t n, int64_t m, int64_t nnz, const void *row_ptr,
                               const void *col, const void *val, const void *row_order, const void *col_order,
                               int64_t row_begin, int64_t row_end, void *row_ptr_out, void *col_out, void *val_out,
                               int64_t out_capacity, int64_t *shard_nnz_host);
int sbx_mixed_permute_csr_rows_nnz(sbx_handle_t h, int64_t n, const void *row_ptr, const void *row_order, int64_t row_begin,
                                   int64_t row_end, int64_t *nnz_host);
