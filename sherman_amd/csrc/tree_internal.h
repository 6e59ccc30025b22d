// tree_internal.h — what the host runtime's units (tree*.cpp) share: the
// handle (struct shm_tree), the constants more than one unit needs, HIP_OK and
// DBG, the cross-stream ordering (shm_tree::Mark, Order) and the declarations
// of the helpers that cross a unit boundary.  Host only: included by
// tree*.cpp and by nothing else (no kernel depends on it).  Every helper is
// defined in exactly one unit, named above its declaration; everything in
// shm::host is hidden from the library's dynamic symbols.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <mutex>
#include <optional>
#include <thread>
#include <vector>

#include "../../include/sherman_amd.h"
#include "kernels.h"
#include "layout.h"
#include "seq_epoch.h"
#include "tree_hooks.h"

// a group of the handle's fields: no dynamic symbol of its own
#define SHM_GROUP struct __attribute__((visibility("hidden")))

struct shm_tree {
  shm_config cfg{};
  hipStream_t stream = nullptr;
  uint8_t* arena = nullptr;
  uint64_t arena_bytes = 0;
  uint64_t cap_pages = 0;
  uint64_t* locks = nullptr;
  uint64_t* stamps = nullptr;  // k_upper phase clock (shm__upper_stamps), off when null
  uint32_t* d_err = nullptr;
  uint64_t* d_counts = nullptr;  // 16 words of device scratch
  uint32_t* route_scratch = nullptr;
  // route_bucket scratch per stream (route_scratch serves the first one), so
  // routed batches on distinct streams bucket concurrently
  std::vector<std::pair<hipStream_t, uint32_t*>> route_ws;
  uint64_t* h_pin = nullptr;     // 4 KB pinned host scratch (coherent, mapped)
  uint32_t* h_pin_dev = nullptr; // its device address (zero-copy read-backs)
  uint32_t rb_seq = 0;           // last zero-copy read-back sequence number
  uint64_t* rstage = nullptr;    // range-scan value staging (RangeArgs.stage)
  uint64_t rstage_words = 0;
  // root page (fixed; a root split relocates the left half, insert.hip) and
  // the host mirror of the device superblock (lagging between syncs)
  uint64_t root = 0;
  uint32_t root_level = 0;
  uint64_t next_page = 0;
  uint64_t splits = 0;
  uint64_t batches = 0;   // mutating API calls
  uint32_t chunks = 0;    // insert chunks issued (the device-side tag)
  uint32_t sticky_err = 0;
  // workspace (sized for cfg.max_batch)
  uint64_t nmax = 0, sep_cap = 0;
  uint64_t *ka = nullptr, *kb = nullptr;
  uint32_t *ia = nullptr, *ib = nullptr, *ic = nullptr;
  uint64_t* kc = nullptr;  // tile-mode ordering scratch (insert_order)
  uint32_t* id = nullptr;
  uint64_t *uk = nullptr, *uv = nullptr, *dk = nullptr;
  uint64_t* pages = nullptr;
  uint64_t* seg_lb = nullptr;  // tagged per-tile staged-head counts (launch_segment)
  uint64_t* bsum64 = nullptr;  // tagged tile words of launch_scan_u64_total
  uint32_t scan_seq = 0;
  uint32_t* seg_start = nullptr;
  uint32_t* seg_end = nullptr;
  uint64_t* seg_page = nullptr;
  uint32_t *seg_T = nullptr, *seg_P = nullptr, *seg_np = nullptr, *seg_ver = nullptr;
  uint8_t* leaf_hw = nullptr;   // per-page occupancy bound (layout.h kLeafHwFull)
  uint8_t* sum = nullptr;       // leaf summaries, kSumBytes per page (layout.h)
  // shm_bulk_load: the lowest fences of the internal levels below the root,
  // one array per level (bulk.hip k_bulk_level); grown on demand
  uint64_t* bulk_low = nullptr;
  uint64_t bulk_low_words = 0;
  // shm_export: two unit lists (page, bound), counts, offsets and the scan's
  // tile sums, each for ex_cap pages, in one allocation; grown on demand
  uint64_t* ex_ws = nullptr;
  uint64_t ex_cap = 0;
  // the last count pass's leaf list (export_count -> export_write)
  int ex_cur = 0;
  uint64_t ex_units = 0;
  // The order index (order.hip; tree_order.cpp): the last whole-tree count
  // pass's leaf units (page, bound, off) and the sampled levels over bound and
  // off, in one allocation of its own (the next export overwrites ex_ws);
  // grown on demand, never shrunk.  It is of the tree as it was when ord_gen
  // stood at oidx.gen: every host-side issue of work that can change the
  // stored pairs or the pages bumps ord_gen (insert_finish, bulk_load_locked,
  // shm_load_image), and a call that needs the index rebuilds it first when
  // the two differ
  uint64_t ord_gen = 0;
  SHM_GROUP Oidx {
    uint64_t* ws = nullptr;
    uint64_t cap_words = 0;
    bool valid = false;
    uint64_t gen = 0;
    uint64_t units = 0, total = 0;
    uint64_t max_pages = 0;  // next_page at the build
    uint64_t builds = 0;
    double last_ms = -1.0;
  } oidx;
  // upsert staging verdicts: per op the slot it overwrites (k_locate), per
  // page the last chunk tag that brought it a new key
  uint32_t* oslot = nullptr;
  uint8_t* pnew = nullptr;  // per page: dev::new_mark(tag) of the last chunk that gave it a new key
  // k_upper state (insert.hip)
  shm::dev::UpperCtl* ctl = nullptr;
  uint64_t* leaf_rd = nullptr;
  // shm__upper_force: bit 0 = the next chunk's k_upper gives up at its first
  // hand-off, bit 1 = it propagates through the level lists (no direct path),
  // bit 2 = its upsert kernel leaves every split to k_upper (any bit does)
  uint32_t force_flags = 0;
  // shm_last_error: the last synchronising call that saw device error bits
  shm_error_t last_error{};
  uint64_t *sep_key[2] = {nullptr, nullptr}, *sep_ptr[2] = {nullptr, nullptr};
  uint64_t* ipage[2] = {nullptr, nullptr};
  uint32_t *h_end = nullptr, *h_T = nullptr, *h_P = nullptr, *h_ver = nullptr, *h_lk = nullptr;
  uint32_t *d_head = nullptr, *d_base = nullptr;
  uint64_t* int_rd = nullptr;
  uint32_t* part_hist = nullptr;  // [kMaxTiles][kCoarse] coarse tile counts
  uint32_t* part_S = nullptr;     // coarse group sums (zero between batches)
  uint32_t* part_mx = nullptr;    // [kCoarse][kMaxTiles] tile mode: each bin's run offset in a tile
  uint32_t* part_mt = nullptr;    // [kCoarse][kMaxTiles] tile mode: each bin's run length in a tile
  uint32_t* part_chunks = nullptr;  // fine-pass chunk table
  uint32_t* gcount = nullptr;       // insert ordering: survivors per 4096-op tile
  uint32_t* bins = nullptr;         // insert ordering: (start, count) per coarse bin
  bool err_pending = false;  // kernels ran since d_err was last read back
  uint64_t pub_batch = 0;          // the chunk tag the mirror last showed (mirror)
  // leaf directory (leafdir.hip): 2^bits entries of 64 B over the shard's
  // key range, rebuilt before a search once the tree grew by 1/32 since the
  // last build (stale entries only cost B-link right moves).  This group, the
  // bucket table and the top replica are read and written by tree_dir.cpp only
  SHM_GROUP Dir {
    uint32_t reads_since_write = 0;  // search calls since the last insert chunk (dir_stale)
    uint64_t pub_seen = 0;           // the tag at the last quiet-rule look (dir_chunk_begin)
    uint64_t np_seen = 0;            // the page count then
    uint32_t quiet_chunks = 0;       // published chunks in a row that left it unchanged
    uint64_t* ent = nullptr;
    uint32_t bits = 0;
    uint32_t* hint = nullptr;  // per prefix: the level-1 / level-2 page on its path
    uint64_t np = 0;
    bool valid = false;
    bool pairs = false;  // the directory is in pair form (a read phase's build)
    bool hint_ok = false;  // hint holds the last build's pages of this tree
    // the allocation: 2^cap_bits entries (a build may use fewer); never
    // shrunk, so a change of form or phase reallocates nothing
    uint32_t cap_bits = 0;
    uint32_t bits_limit = 64;  // an allocation this large failed: not asked again
    uint64_t mem_limit = 0;    // shm__dir_mem_limit (test hook): bytes, 0 = none
    // rebuild cost: timing events around each build, read once they completed
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ev_pending = false;
    uint64_t builds = 0;
    double last_ms = -1.0, total_ms = 0.0;
    bool maint = false;    // the writers keep the entries current (dir_maint_enabled)
    bool vals = true;      // a pair-form build adds the value form (SHM_DIR_VALS, layout.h kDirVals)
    // the insert chunks' repair lists (dir_upkeep.h, k_dir_repair): prefix
    // indices, and a count per chunk parity
    uint32_t* fix = nullptr;
    uint32_t* fix_n = nullptr;
    uint32_t fix_cap = 0;
    uint64_t lost_at_build = 0;  // the host word kPubDirLost at the last build
    uint64_t work_seen = 0;      // the host words kPubDirWork / kPubDirUpkeeps at the last look
    uint64_t upk_seen = 0;
    uint32_t idle_upkeeps = 0;   // finished upkeeps in a row that found nothing to do
    bool off = false;      // no directory could be allocated: walks from the root
    bool exact = false;    // built with upkeep on, and upkeep on ever since (WalkArgs.dir_exact)
    bool maint_always = false;  // shm__dir_config maint 2: every chunk keeps it (tests)
    bool last_upkept = false;   // the previous chunk kept the directory
    double debt_ps = 0.0;  // gets' estimated extra cost on shared prefixes since the build
  } dir;
  // the key-value bucket table (valtab.h): 2^bits buckets of 128 B, built
  // with a read phase's value-form directory (refresh_dir), kept by the same
  // chunks that keep the directory, trusted exactly while dir.exact holds
  SHM_GROUP Vt {
    uint64_t* tab = nullptr;
    uint64_t bytes = 0;       // the allocation
    uint32_t bits = 0;
    bool valid = false;       // built for the directory as it is, not dropped
    bool on = true;           // SHM_VALTAB
    uint64_t max_bytes = 8ull << 30;  // SHM_VALTAB_MAX_BYTES
    bool get_coop = true;        // SHM_GET_COOP
    bool get_pack = true;        // SHM_GET_PACK
    uint32_t bits_failed = 64;  // an allocation this large failed: not asked again
    uint32_t drop_bits = 0;   // the table was dropped at this size (too many keys in dead buckets)
    uint64_t* ctr = nullptr;  // device: {dead buckets, keys in dead buckets, keys} (kVtCtrWords)
    uint32_t seq = 0;         // the last build's sequence number in the host words
    bool pending = false;     // its counts were not read yet (vt_poll)
    uint64_t dead_keys = 0, keys = 0;  // at the last build
  } vt;
  // LDS replica of the top of the tree (SHM_FLAG_TOP_LDS without the
  // directory; launch_top), rebuilt with the same staleness rule
  SHM_GROUP Top {
    uint64_t* keys = nullptr;
    uint32_t* pages = nullptr;
    uint64_t* scratch = nullptr;
    uint32_t n = 0;
    uint64_t np = 0;
    bool valid = false;
  } top;
  std::mutex mu;
  enum ProfKind { kProfGet = 0, kProfInsert = 1, kProfRange = 2 };
  // get: e0 order e1 walk e2; insert chunk: e0 .. e1 upsert e2 .. e3;
  // range launch: e0 kernel e1
  struct ProfRec {
    hipEvent_t e[4];
    uint64_t n;
    int kind;
    int clk = -1;         // a get walk's clock slot in prof.clk (k_get_sum), or -1
    uint64_t blocks = 0;  // its grid
  };
  // the summary walk's device clock words while profiling (WalkArgs.clk):
  // kClkSlots launches of (blocks + 4 blocks) words, reused round robin
  static constexpr int kClkSlots = 16;
  // profiling (shm_profile_*)
  SHM_GROUP Prof {
    // index statistics of the get walk (shm_index_stats), when stats
    uint64_t* idx_stats = nullptr;
    // per-chunk insert counts while profiling (UpperArgs.prof): unique
    // upserts, deletes, staged segments
    uint64_t* ins = nullptr;
    bool stats = false;
    bool on = false;
    uint64_t* clk = nullptr;
    uint64_t clk_words = 0;  // per slot
    int clk_next = 0, clk_live = 0;
    double clk_khz = 0.0;
    std::vector<ProfRec> pending;
    std::vector<hipEvent_t> event_pool;
    shm_profile_t acc{};
  } prof;
  struct GetWs {
    uint64_t *keys1 = nullptr, *keys_out = nullptr;
    uint32_t *pos1 = nullptr, *src = nullptr, *M = nullptr, *S = nullptr, *chunks = nullptr;
  };
  // A call's completion point on its stream, recorded lazily (Order): the
  // event is recorded at the stream's tail only when a call on another
  // stream first has to follow it -- an event record between two kernels
  // leaves the device idle ≈ 4.6 µs (tools/event_gap.hip), so none is placed
  // where nobody waits.  The tail then holds everything issued there so far:
  // the first waiter may wait for a little more than it needs, never less.
  struct Mark {
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
    bool valid = false;     // a call to follow exists
    bool recorded = false;  // ev marks it (recorded at the first wait)
  };
  // chunks ordered by shm_insert_order and not yet applied, oldest first
  struct Pending {
    uint32_t tag;
    uint64_t n;
    ProfRec pr;
    hipEvent_t ev;  // the ordering done (on s)
    hipStream_t s;
  };
  // ---- cross-stream ordering (Order below) --------------------------------
  // Searches are "shared" calls: they may run concurrently on distinct
  // streams.  An ordered search uses one of two get workspaces, alternating,
  // so the partition of one batch can overlap the walk of the previous one
  // on another stream.  Every other call that touches device state (inserts,
  // deletes, range scans, routing, a directory rebuild) is "exclusive": its
  // stream waits for every earlier call on the other streams.
  SHM_GROUP Sync {
    GetWs gws[2];           // gws[0] aliases the insert workspace (ka, kb, ia, ib, part_*)
    int next_gws = 0;
    std::vector<Mark> shared_ev;  // last shared calls per stream, since the last exclusive one
    Mark ex;                      // last exclusive call
    // insert ordering pipeline.  The ordering of chunk `tag` writes the op
    // buffers of parity tag & 1 (uk / uv / dk / counts, op_keys()),
    // which the apply of chunk tag - 2 read last (app_tag / app_m); every ordering
    // reuses the ordering scratch (ka .. bins), so it follows the previous
    // ordering (ord_ev).  A later chunk's ordering may therefore run on
    // another stream beside this chunk's apply.
    // (app: the apply's chunk tag, which its k_upper publishes in the host
    // mirror once it is done with the op buffers, and a lazily recorded mark
    // of its stream; ord: a lazily recorded mark)
    uint64_t app_tag[2] = {0, 0};
    bool app_valid[2] = {false, false};
    Mark app_m[2];
    Mark ord;
    Pending pend[2];
    int n_pend = 0;
    Mark gws_m[2];  // last user of each get workspace
  } sync;
};

namespace shm {
namespace host __attribute__((visibility("hidden"))) {

constexpr uint32_t kPubWord = 768;         // superblock mirror: u64 words 384.. of h_pin

#define HIP_OK(expr)                                                         \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      fprintf(stderr, "sherman_amd: %s failed: %s (%s:%d)\n", #expr,         \
              hipGetErrorString(_e), __FILE__, __LINE__);                    \
      return SHM_EIO;                                                        \
    }                                                                        \
  } while (0)

#define DBG(s, what)                   \
  do {                                 \
    int _r = dbg((s), (what));         \
    if (_r) return _r;                 \
  } while (0)

template <class T>
int dalloc(T** p, uint64_t count) {
  if (count == 0) count = 1;
  if (hipMalloc((void**)p, sizeof(T) * count) != hipSuccess) {
    *p = nullptr;
    return SHM_ENOMEM;
  }
  return SHM_OK;
}

// stream argument of the C-ABI: NULL is the HIP null (default) stream, as for
// any HIP API; t->stream is used only for create / image transfers.
inline hipStream_t pick(void* s) { return (hipStream_t)s; }

inline bool use_leaf_dir(const shm_tree* t) { return (t->cfg.flags & SHM_FLAG_LEAF_DIR) != 0; }
inline bool use_top(const shm_tree* t) {
  return !use_leaf_dir(t) && (t->cfg.flags & SHM_FLAG_TOP_LDS) != 0;
}

// the host mirror words k_upper publishes into h_pin (kPubWord; kernels.h
// kPub*), as the host reads them and at their device address
inline volatile uint64_t* pub_words(const shm_tree* t) {
  return reinterpret_cast<volatile uint64_t*>(t->h_pin) + kPubWord / 2;
}
inline uint64_t* pub_words_dev(const shm_tree* t) {
  return reinterpret_cast<uint64_t*>(t->h_pin_dev) + kPubWord / 2;
}

// the arena fields the kernel argument structs share, under the same names
// (kernels.h); root and sum where the struct has them
template <class A>
auto set_root(A& a, const shm_tree* t, int) -> decltype((void)a.root) { a.root = t->root; }
template <class A>
void set_root(A&, const shm_tree*, long) {}
template <class A>
auto set_sum(A& a, const shm_tree* t, int) -> decltype((void)a.sum) { a.sum = t->sum; }
template <class A>
void set_sum(A&, const shm_tree*, long) {}
template <class A>
A arena_args(const shm_tree* t) {
  A a{};
  a.arena = t->arena;
  a.arena_bytes = t->arena_bytes;
  a.node = t->cfg.node_id;
  a.err = t->d_err;
  a.leaf_hw = t->leaf_hw;
  set_root(a, t, 0);
  set_sum(a, t, 0);
  return a;
}

// ---- tree.cpp ------------------------------------------------------------
// env flags: on unless the first character is '0' (dflt true), or on only
// when it is '1' (dflt false); an integer with a default.  The callers keep
// the value in a function static: read once per process, at first use
bool env_on(const char* name, bool dflt);
int env_int(const char* name, int dflt);
hipEvent_t new_event();
int follow(shm_tree::Mark& m, hipStream_t s);
void note(shm_tree::Mark& m, hipStream_t s);
void mirror(shm_tree* t);
uint32_t* lb_ctr(shm_tree* t, int which);
int dbg(hipStream_t s, const char* what);
int readback(shm_tree* t, hipStream_t s, const void* src, size_t bytes, int clear = 0);
int write_superblock(shm_tree* t, hipStream_t s);
int check_err(shm_tree* t, hipStream_t s);

// Cross-stream ordering of one API call (shm_tree: shared / exclusive calls).
// Constructed under t->mu before the call's first launch; the destructor
// notes the call's stream (no event: shm_tree::Mark).  Waits are skipped for
// marks of the same stream (stream order already covers them).
struct Order {
  shm_tree* t;
  hipStream_t s;
  bool ex;
  int ws = -1;  // get workspace used by a shared call (-1: none)
  int rc = SHM_OK;
  Order(shm_tree* tt, hipStream_t ss, bool exclusive);
  // a shared call that turns exclusive (a directory rebuild)
  void make_exclusive();
  // take the next get workspace; returns its index
  int take_ws();
  void wait(shm_tree::Mark& m);
  ~Order();
};

// ---- tree_dir.cpp --------------------------------------------------------
bool dir_trace();
// create / free_all: the env switches, the repair lists and their first
// clear; every allocation and event of the three groups
int dir_create(shm_tree* t, uint64_t n);
hipError_t dir_fix_clear(shm_tree* t, hipStream_t s);
void dir_free(shm_tree* t);
// the tree's contents were replaced (shm_load_image); table: the bucket
// table goes too (bulk load); new_range: ... and the size it was dropped at
// is forgotten (shm_tree_set_key_range)
void dir_invalidate(shm_tree* t, bool table, bool new_range);
// the chunk counter was set to tag (epoch_reset, shm__seq_jump)
void dir_tag_reset(shm_tree* t, uint64_t tag);
void dir_note_read(shm_tree* t);
void dir_note_gets(shm_tree* t, uint64_t n);
bool dir_stale(const shm_tree* t);
bool top_stale(const shm_tree* t);
int dir_poll(shm_tree* t, bool wait);
int vt_poll(shm_tree* t, bool wait);
int refresh_dir(shm_tree* t, hipStream_t s);
int refresh_top(shm_tree* t, hipStream_t s);
// the directory view of a kernel's arguments: dir, dir_lo, dir_shift, dir_n
// (null while no directory is valid) ...
void dir_view(const shm_tree* t, dev::RangeArgs& a);
void dir_view(const shm_tree* t, dev::ScanArgs& a);
// ... with its form and exactness for k_locate
void dir_view_locate(const shm_tree* t, dev::WalkArgs& a);
// ... and, for a get, its exactness, the bucket table while trusted (not
// under a.page_check, set before) and the top replica
void dir_view_get(const shm_tree* t, dev::WalkArgs& a);
// an insert chunk's part in the directory's upkeep (insert_apply), in call
// order: does this chunk keep the directory; k_upper's view of it and the
// upkeep's arguments; the two launches after k_upper
bool dir_chunk_begin(shm_tree* t, uint32_t tag);
int dir_chunk_args(shm_tree* t, hipStream_t s, bool upkeep, dev::UpperArgs& u);
int dir_chunk_upkeep(shm_tree* t, hipStream_t s, const dev::UpperArgs& u, uint64_t n,
                     uint32_t tag);

// ---- tree_insert.cpp -----------------------------------------------------
uint64_t* op_counts(shm_tree* t, uint32_t tag);
int insert_chunk(shm_tree* t, hipStream_t s, const uint64_t* keys, const uint64_t* vals,
                 uint64_t n, bool skip_pad = false);

// ---- tree_image.cpp ------------------------------------------------------
// the whole tree's count pass for the order index (export_count(0, kKeyMax)):
// on success the leaf units stand in the export workspace, *page / *bound /
// *off name their lists (units words each), *total_dev the device word that
// holds the total, and t->ex_units / *total are their counts.  Synchronising
int order_count(shm_tree* t, hipStream_t s, const uint64_t** page, const uint64_t** bound,
                const uint64_t** off, const uint64_t** total_dev, uint64_t* total);

// ---- tree_prof.cpp -------------------------------------------------------
int prof_begin(shm_tree* t, hipStream_t s, int kind, uint64_t n, int ne, shm_tree::ProfRec& r);
int drain_profile(shm_tree* t);

// one launch between the two events of a range record (kProfRange)
template <class F>
int timed_launch(shm_tree* t, hipStream_t s, uint64_t n, F&& launch) {
  shm_tree::ProfRec pr{};
  if (t->prof.on) {
    const int rc = prof_begin(t, s, shm_tree::kProfRange, n, 2, pr);
    if (rc) return rc;
  }
  launch();
  HIP_OK(hipGetLastError());
  if (t->prof.on) {
    HIP_OK(hipEventRecord(pr.e[1], s));
    t->prof.pending.push_back(pr);
  }
  return SHM_OK;
}

}  // namespace host
}  // namespace shm

using namespace shm;
using namespace shm::host;
