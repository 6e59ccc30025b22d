// tree_dir.cpp — the leaf directory, the bucket table and the LDS top replica.
//
// Everything that decides about or describes them: when a build is due and in
// which form (dir_stale, want_pairs), the allocations (dir_alloc, vt_build),
// the builds (refresh_dir, refresh_top), the drop rule of the table
// (vt_poll), the view a kernel's arguments get (dir_view*), an insert chunk's
// part in the upkeep (dir_chunk_*), what create, free and the calls that
// replace the tree's contents do to this state, and the stats, test hooks and
// dumps.  The groups shm_tree::dir, vt and top are read and written here and
// nowhere else; the other units go through the functions tree_internal.h
// declares.
#include "tree_internal.h"

namespace shm {
namespace host __attribute__((visibility("hidden"))) {

// (re)build the leaf directory when missing or the tree grew by > 1/32;
// 2^bits entries with bits = ceil(log2(pages)) (~1 entry per leaf)
// ... and in a read phase (kReadPhase searches since the last insert chunk)
// once the tree changed at all since the last build: a read-only workload
// (C2) then runs on an exact directory, with no B-link right moves left
// from the pages the last 1/32 of growth split (0.039 per get at C2 before
// this rule: each one a header and a summary read)
constexpr uint32_t kReadPhase = 4;
constexpr uint32_t kVtWord = 896;          // bucket table build counts: u64 words 448..450 of h_pin
constexpr uint32_t kVtFlagWord = 904;      // ... and their sequence word
// ... and likewise once the tree has gone quiet: the mirror showed
// kQuietChunks newer chunk tags in a row with the same page count (updates
// only, C3's mix after the load; while the directory is behind, every chunk
// publishes its tag, UpperArgs.pub_always), so a write-heavy workload that no
// longer splits also gets one rebuild instead of running on the directory of
// up to 1/32 growth ago (C3 lost 7 % to 0.01 right moves per get when the
// load's last rebuild fell early).  A mirror that merely lags (the host ahead
// of the device) shows no newer tag, so it never looks quiet
constexpr uint32_t kQuietChunks = 2;
// finished directory upkeeps in a row with no new key and no split page after
// which the chunks stop keeping the directory (insert_apply)
constexpr uint32_t kIdleUpkeeps = 2;

// Directory entries per tree page, as a power of two (SHM_DIR_EXTRA_BITS
// overrides both): eight 64 B entries per page while the tree is written
// (late round 5, with the shared candidate rounds and a quiet phase's pair
// form: same box C3 15671 / 15171 -> 15994 / 16078 Mops/s against four, C5
// unchanged; sixteen no better), and sixteen in a
// read phase, in pair form (every C2 get answered from its entry, 2 GB at
// C2's 2^26 keys): same box, C2 18200 / 18217 at four, 18941 / 18964 at
// eight, 19651 / 19685 Mops/s at sixteen (DESIGN §3 "The pair form")
uint32_t dir_extra_bits(bool read_phase) {
  static const int env = env_int("SHM_DIR_EXTRA_BITS", -1);
  const int v = env >= 0 ? env : read_phase ? 4 : 3;
  return (uint32_t)(v > 4 ? 4 : v);
}
bool read_phase(const shm_tree* t) { return t->dir.reads_since_write >= kReadPhase; }
uint32_t dir_bits_for(const shm_tree* t, bool rp) {
  uint32_t bits = 10;
  while (bits < 24 && (1ull << bits) < t->next_page) ++bits;
  bits += dir_extra_bits(rp);
  if (bits > 25) bits = 25;  // 2 GB of entries at most
  if (bits > t->cfg.key_bits) bits = t->cfg.key_bits;  // one entry per key at most
  if (bits > t->dir.bits_limit) bits = t->dir.bits_limit;  // a larger allocation failed
  return bits;
}
// The form of the next build: pairs while no page is added (a read phase,
// or a write phase whose chunks leave the page count as it is: C3's
// updates), fingerprints while the tree grows (C5: a pair build reads every
// leaf).  The form only changes at a rebuild the staleness rules call for
// anyway (and once when a read phase starts), so sporadic splits cause no
// rebuilds of their own.
bool want_pairs(const shm_tree* t) {
  return read_phase(t) || t->dir.quiet_chunks >= kQuietChunks;
}

// Directory upkeep by the writers (SHM_DIR_MAINT, default on, VERDICT r5
// #3): an insert chunk keeps the entries it affects current -- a new key in
// an empty slot adds its pair (pair form) or its fingerprint (fingerprint
// form) to its prefix's entry, and every page a split writes rewrites the
// entries of the prefixes that lie wholly inside its fences (one leaf, its
// keys' slots) and leaves the one or two prefixes it shares with a
// neighbour to the summary walk (kDirPairsBad / kDirFp cleared).  The
// directory then goes stale only by those shared prefixes, about two per
// page a split adds, and by density (the tree doubling); a rebuild is
// bought when the gets' estimated extra cost on the shared prefixes has
// reached the measured cost of one build (ski rental: at most twice the
// best offline choice).  SHM_DIR_MAINT=0: the writers leave the directory
// alone and round 5's rules rebuild it (growth by 1/32, every read phase
// after a change).
bool dir_maint_enabled() {
  static const bool on = env_on("SHM_DIR_MAINT", true);
  return on;
}
// a get that starts at a stale entry reads the leaf's summary line (and may
// turn right): about one 128 B request more than an exact entry's (2.18
// requests per get at C2, 51 ps per get at 19.5 G gets/s: DESIGN §3)
constexpr double kSharedPrefixGetPs = 25.0;
// the cost of a build before one was measured: 100 ps per entry (k_leaf_dir
// + k_dir_pairs at 2^25 entries: 3.1-3.4 ms, profiles/r05)
constexpr double kBuildPsPerEntry = 100.0;

double dir_build_ps(const shm_tree* t) {
  return t->dir.last_ms > 0 ? t->dir.last_ms * 1e9 : kBuildPsPerEntry * (double)(1ull << t->dir.bits);
}
// the host word the repair kernel adds its lost repairs to (cumulative)
uint64_t dir_lost(const shm_tree* t) {
  return pub_words(t)[dev::kPubDirLost];
}
// the fraction of entries left stale since the last build: the repairs the
// chunks could not list (k_dir_repair's count past its list)
double dir_shared_frac(const shm_tree* t) {
  if (!t->dir.valid) return 0.0;
  const uint64_t l = dir_lost(t);
  if (l <= t->dir.lost_at_build) return 0.0;
  const double f = (double)(l - t->dir.lost_at_build) / (double)(1ull << t->dir.bits);
  return f < 1.0 ? f : 1.0;
}

bool dir_stale(const shm_tree* t) {
  if (t->dir.off) return false;
  if (!t->dir.valid) return true;
  const bool rp = read_phase(t);
  if (t->dir.maint && t->dir.exact) {
    if (want_pairs(t) && !t->dir.pairs) return true;   // the form a read / quiet phase wants
    if (dir_bits_for(t, rp) > t->dir.bits) return true;  // a read phase's density, or the tree doubled
    return dir_lost(t) != t->dir.lost_at_build && t->dir.debt_ps >= dir_build_ps(t);
  }
  if (t->next_page > t->dir.np + t->dir.np / 32) return true;
  // a read phase also wants its denser directory, once
  if (rp && (t->dir.bits < dir_bits_for(t, true) || !t->dir.pairs)) return true;
  return t->next_page != t->dir.np && (rp || t->dir.quiet_chunks >= kQuietChunks);
}

// a search call: kReadPhase of them since the last insert chunk make a read phase
void dir_note_read(shm_tree* t) {
  if (t->dir.reads_since_write < kReadPhase) ++t->dir.reads_since_write;
}
// a search of n keys: its estimated extra cost on the shared prefixes
void dir_note_gets(shm_tree* t, uint64_t n) {
  if (t->dir.maint && t->dir.exact) t->dir.debt_ps += (double)n * dir_shared_frac(t) * kSharedPrefixGetPs;
}

// the last build's device time once its end event completed (wait: block
// for it)
int dir_poll(shm_tree* t, bool wait) {
  if (!t->dir.ev_pending) return SHM_OK;
  const hipError_t q = wait ? hipEventSynchronize(t->dir.ev[1]) : hipEventQuery(t->dir.ev[1]);
  if (q == hipErrorNotReady) return SHM_OK;
  HIP_OK(q);
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, t->dir.ev[0], t->dir.ev[1]));
  t->dir.last_ms = ms;
  t->dir.total_ms += ms;
  t->dir.ev_pending = false;
  return SHM_OK;
}

// The directory's allocation holds 2^bits entries (+ the level hints);
// never shrunk.  A larger one is allocated before the old one is freed, and
// when it cannot be had the tree keeps the directory it has, at its size
// (ADVICE r5): dir_bits_limit then caps every later build, so the failed
// allocation is not tried again.  No directory at all: progressively smaller
// ones, and at the last the gets walk from the root.
int dir_alloc(shm_tree* t, uint32_t bits, hipStream_t s) {
  if (t->dir.ent && bits <= t->dir.cap_bits) return SHM_OK;
  for (;;) {
    const uint64_t ent = 1ull << bits;
    const uint64_t bytes = ent * (8 * kDirWords) + ent * 8;  // entries + 2 u32 hints
    uint64_t* nd = nullptr;
    uint32_t* nh = nullptr;
    bool ok = !(t->dir.mem_limit && bytes > t->dir.mem_limit);
    if (ok && dalloc(&nd, kDirWords * ent)) ok = false;
    if (ok && dalloc(&nh, 2 * ent)) {
      (void)hipFree(nd);
      ok = false;
    }
    if (ok) {
      if (t->dir.ent) {  // the old directory's last readers are ordered before s
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipFree(t->dir.ent));
        HIP_OK(hipFree(t->dir.hint));
      }
      t->dir.ent = nd;
      t->dir.hint = nh;
      t->dir.cap_bits = bits;
      t->dir.hint_ok = false;
      return SHM_OK;
    }
    (void)hipGetLastError();  // clear the failed allocation's sticky status
    if (t->dir.ent) {
      t->dir.bits_limit = t->dir.cap_bits;
      return SHM_OK;  // keep what we have
    }
    if (bits <= 10) {
      t->dir.off = true;  // no directory: the walks start at the root
      return SHM_OK;
    }
    t->dir.bits_limit = --bits;
  }
}

// The bucket table pays only while most gets end at their bucket: with p the
// share of stored keys in live buckets and R ~ 1.7 the directory path's
// requests per get, p + (1 - p)(1 + R) < R needs p > 1 / R ~ 0.6.  Below
// kVtMinLive (clustered or dense key sets: every get would pay one more
// request for nothing) the table is dropped.
constexpr double kVtMinLive = 0.75;

// SHM_TRACE_DIR=1: the directory's and the table's builds and drops on stderr
bool dir_trace() {
  static const bool on = env_on("SHM_TRACE_DIR", false);
  return on;
}

void vt_free(shm_tree* t) {
  if (t->vt.tab) (void)hipFree(t->vt.tab);
  t->vt.tab = nullptr;
  t->vt.bytes = 0;
  t->vt.valid = false;
}

// the last table build's counts once they arrived in the host words (wait:
// block for them); applies the drop rule
int vt_poll(shm_tree* t, bool wait) {
  if (!t->vt.pending) return SHM_OK;
  const uint32_t* flag = reinterpret_cast<const uint32_t*>(t->h_pin) + kVtFlagWord;
  if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != t->vt.seq) {
    if (!wait) return SHM_OK;
    HIP_OK(hipDeviceSynchronize());
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != t->vt.seq) return SHM_EIO;
  }
  const volatile uint64_t* c = reinterpret_cast<const volatile uint64_t*>(t->h_pin) + kVtWord / 2;
  t->vt.dead_keys = c[1];
  t->vt.keys = c[2];
  t->vt.pending = false;
  if (dir_trace())
    fprintf(stderr, "sherman_amd: bucket table: 2^%u buckets, %llu of %llu stored keys in dead "
            "buckets\n", t->vt.bits, (unsigned long long)t->vt.dead_keys,
            (unsigned long long)t->vt.keys);
  if (t->vt.valid && (double)(t->vt.keys - t->vt.dead_keys) < kVtMinLive * (double)t->vt.keys) {
    // searches on other streams may still read it
    HIP_OK(hipDeviceSynchronize());
    t->vt.drop_bits = t->vt.bits;
    vt_free(t);
  }
  return SHM_OK;
}

// the table is read by the gets and kept by the chunks
bool vt_trusted(const shm_tree* t) {
  return t->vt.tab && t->vt.valid && t->dir.valid && t->dir.exact && t->dir.pairs;
}

// the table of a read phase's build (inside its timing events): half as many
// buckets as the directory has entries, all or nothing -- a smaller table's
// buckets would all overflow
int vt_build(shm_tree* t, hipStream_t s, bool want) {
  t->vt.valid = false;
  t->vt.pending = false;
  // no table for this build: the old one goes (its last readers are ordered
  // before s), so its bytes do not outlive the read phase that used them
  auto none = [&]() -> int {
    if (t->vt.tab) {
      HIP_OK(hipStreamSynchronize(s));
      vt_free(t);
    }
    return SHM_OK;
  };
  if (!want || !t->vt.on || t->dir.bits < 2) return none();
  const uint32_t bits = t->dir.bits - 1;
  if (bits == t->vt.drop_bits) return none();  // dropped at this size: not again until the tree doubled
  const uint64_t bytes = (8ull * dev::kVtBucketWords) << bits;
  const uint64_t dir_bytes = (1ull << t->dir.cap_bits) * (8 * kDirWords + 8);
  bool ok = bytes <= t->vt.max_bytes && bits < t->vt.bits_failed &&
            !(t->dir.mem_limit && dir_bytes + bytes > t->dir.mem_limit);
  if (ok && t->vt.bytes != bytes) {
    if (t->vt.tab) {  // the old table's last readers are ordered before s
      HIP_OK(hipStreamSynchronize(s));
      vt_free(t);
    }
    if (hipMalloc((void**)&t->vt.tab, bytes) != hipSuccess) {
      (void)hipGetLastError();
      t->vt.tab = nullptr;
      t->vt.bits_failed = bits;
      ok = false;
    } else {
      t->vt.bytes = bytes;
    }
  }
  if (!ok) return none();
  if (!t->vt.ctr && dalloc(&t->vt.ctr, dev::kVtCtrWords)) return SHM_ENOMEM;
  t->vt.bits = bits;
  HIP_OK(hipMemsetAsync(t->vt.tab, 0, bytes, s));
  HIP_OK(hipMemsetAsync(t->vt.ctr, 0, 8 * dev::kVtCtrWords, s));
  dev::launch_vt_build(t->arena, t->sum, t->next_page, t->cfg.key_lo, t->cfg.key_bits - bits,
                       1ull << bits, t->vt.tab, t->vt.ctr, s);
  // the counts into the host words (the drop rule reads them lazily)
  t->vt.seq = t->vt.seq + 1 ? t->vt.seq + 1 : 1;
  dev::launch_readback(t->h_pin_dev + kVtWord, reinterpret_cast<const uint32_t*>(t->vt.ctr), 6,
                       t->h_pin_dev + kVtFlagWord, t->vt.seq, 0, s);
  t->vt.valid = true;
  t->vt.pending = true;
  return SHM_OK;
}

int refresh_dir(shm_tree* t, hipStream_t s) {
  if (const int rc = dir_poll(t, false)) return rc;
  if (!dir_stale(t)) return SHM_OK;
  const bool trace = dir_trace();
  if (trace)
    fprintf(stderr, "sherman_amd: leaf directory rebuild: pages %llu (last build %llu), %u reads "
            "since the last insert, debt %.1f us\n", (unsigned long long)t->next_page,
            (unsigned long long)t->dir.np, t->dir.reads_since_write, t->dir.debt_ps * 1e-6);
  uint32_t bits = dir_bits_for(t, read_phase(t));
  if (const int rc = dir_alloc(t, bits, s)) return rc;
  if (t->dir.off) {
    t->dir.valid = false;
    t->vt.valid = false;
    return SHM_OK;
  }
  if (bits > t->dir.cap_bits) bits = t->dir.cap_bits;
  if (bits != t->dir.bits) t->dir.hint_ok = false;  // the hints are laid out by entry count
  t->dir.bits = bits;
  // the previous build's time first (its events are reused)
  if (const int rc = dir_poll(t, true)) return rc;
  for (hipEvent_t& e : t->dir.ev)
    if (!e) HIP_OK(hipEventCreate(&e));  // timing events (a rebuild is rare)
  HIP_OK(hipEventRecord(t->dir.ev[0], s));
  // a read phase builds the pair form (layout.h kDirPairs): each prefix's
  // own keys, a get reads fewer false candidates and prefixes that span
  // several leaves are answered from the entry as well
  const bool pairs = want_pairs(t);
  dev::launch_leaf_dir(t->arena, t->arena_bytes, t->cfg.node_id, t->root, t->cfg.key_lo,
                       t->cfg.key_bits - bits, 1ull << bits, t->dir.ent, t->dir.hint,
                       t->dir.hint_ok ? 1 : 0, t->sum, t->d_err, s, pairs ? 1 : 0);
  if (pairs)
    dev::launch_dir_pairs(t->arena, t->sum, t->next_page, t->cfg.node_id, t->cfg.key_lo,
                          t->cfg.key_bits - bits, 1ull << bits, t->dir.ent, s);
  // the value form is only ever read from an exact directory
  if (pairs && t->dir.vals && t->dir.maint)
    dev::launch_dir_vals(t->arena, t->next_page, 1ull << bits, t->dir.ent, s);
  // ... and so is the bucket table, built with it
  // (a read phase's build only: a write phase that went quiet builds pairs
  // too, but its gets share the device with chunks that would each pay the
  // table's upkeep)
  if (const int rc = vt_build(t, s, pairs && t->dir.vals && t->dir.maint && read_phase(t)))
    return rc;
  HIP_OK(hipEventRecord(t->dir.ev[1], s));
  t->dir.ev_pending = true;
  ++t->dir.builds;
  t->dir.pairs = pairs;
  t->dir.np = t->next_page;
  t->dir.valid = true;
  t->dir.hint_ok = true;
  t->dir.debt_ps = 0.0;
  t->dir.lost_at_build = dir_lost(t);
  t->dir.idle_upkeeps = 0;
  t->dir.exact = t->dir.maint;
  return SHM_OK;
}

// the LDS replica's table (rebuilt like the directory, once the tree grew
// by 1/32); one read-back of its size per rebuild
bool top_stale(const shm_tree* t) {
  return !(t->top.valid && t->next_page <= t->top.np + t->top.np / 32);
}
int refresh_top(shm_tree* t, hipStream_t s) {
  if (!use_top(t) || !top_stale(t)) return SHM_OK;
  if (!t->top.keys) {
    if (dalloc(&t->top.keys, dev::kTopMax) || dalloc(&t->top.pages, dev::kTopMax) ||
        dalloc(&t->top.scratch, 4ull * dev::kTopMax))
      return SHM_ENOMEM;
  }
  dev::launch_top(t->arena, t->arena_bytes, t->cfg.node_id, t->root, dev::kTopMax, t->top.keys,
                  t->top.pages, t->top.scratch, reinterpret_cast<uint32_t*>(t->d_counts + 14),
                  t->d_err, s);
  HIP_OK(hipGetLastError());
  const int rc = readback(t, s, t->d_counts + 14, sizeof(uint32_t));
  if (rc) return rc;
  t->top.n = (uint32_t)t->h_pin[0];
  t->top.np = t->next_page;
  t->top.valid = t->top.n > 0;
  return SHM_OK;
}

// ---- the view a kernel's arguments get ------------------------------------
// (the argument structs of kernels.h name these fields alike)
template <class A>
static void set_dir(const shm_tree* t, A& a) {
  if (!use_leaf_dir(t) || !t->dir.valid) return;
  a.dir = t->dir.ent;
  a.dir_lo = t->cfg.key_lo;
  a.dir_shift = t->cfg.key_bits - t->dir.bits;
  a.dir_n = 1ull << t->dir.bits;
}
template <class A>
static void set_vt(const shm_tree* t, A& a) {
  a.vt = t->vt.tab;
  a.vt_lo = t->cfg.key_lo;
  a.vt_shift = t->cfg.key_bits - t->vt.bits;
  a.vt_n = 1ull << t->vt.bits;
}
void dir_view(const shm_tree* t, dev::RangeArgs& a) { set_dir(t, a); }
void dir_view(const shm_tree* t, dev::ScanArgs& a) { set_dir(t, a); }
void dir_view_locate(const shm_tree* t, dev::WalkArgs& a) {
  set_dir(t, a);
  a.dir_pairs = a.dir && t->dir.pairs ? 1 : 0;
  a.dir_exact = a.dir && t->dir.exact ? 1 : 0;
}
void dir_view_get(const shm_tree* t, dev::WalkArgs& a) {
  set_dir(t, a);
  a.dir_exact = a.dir && t->dir.exact ? 1 : 0;
  if (a.dir && !a.page_check && vt_trusted(t)) {
    set_vt(t, a);
    a.get_coop = t->vt.get_coop ? 1 : 0;
    a.get_pack = t->vt.get_pack ? 1 : 0;
  }
  if (use_top(t) && t->top.valid) {
    a.top_keys = t->top.keys;
    a.top_pages = t->top.pages;
    a.top_n = t->top.n;
  }
}

// ---- an insert chunk's part (insert_apply) ---------------------------------
// The quiet rule's and the upkeep rule's bookkeeping at the start of a chunk;
// returns whether the chunk keeps the directory
bool dir_chunk_begin(shm_tree* t, uint32_t tag) {
  const bool searched = t->dir.reads_since_write > 0;
  t->dir.reads_since_write = 0;
  if (t->pub_batch != t->dir.pub_seen) {  // a newer chunk published since the last look
    if (t->next_page == t->dir.np_seen) {
      if (t->dir.quiet_chunks < kQuietChunks) ++t->dir.quiet_chunks;
    } else {
      t->dir.quiet_chunks = 0;
      t->dir.np_seen = t->next_page;
    }
    t->dir.pub_seen = t->pub_batch;
  }
  // the chunk keeps the directory exact (dir_upkeep.h: two launches after
  // its k_upper) only where gets read it between chunks and the chunks
  // still add keys: a write-only stream (C5) or one whose upkeeps found
  // nothing to do kIdleUpkeeps times in a row (C3's updates) runs round 5's
  // rules instead -- its directory stops being exact until the next build --
  // rather than pay the launches for nothing
  {  // the upkeeps finished since the last look: did any find work?
    const volatile uint64_t* p = pub_words(t);
    const uint64_t done = p[dev::kPubDirUpkeeps];  // first: the work word is at least this new
    const uint64_t work = p[dev::kPubDirWork];
    if (done != t->dir.upk_seen) {
      t->dir.idle_upkeeps = work == t->dir.work_seen ? t->dir.idle_upkeeps + (uint32_t)(done - t->dir.upk_seen) : 0;
      t->dir.upk_seen = done;
      t->dir.work_seen = work;
    }
  }
  const bool upkeep = t->dir.maint && t->dir.exact && t->dir.valid &&
                      ((searched && t->dir.idle_upkeeps < kIdleUpkeeps) || t->dir.maint_always);
  if (!upkeep && t->dir.exact && dir_trace())
    fprintf(stderr, "sherman_amd: chunk %u not kept: the directory is no longer exact (searched %d, "
            "idle upkeeps %u)\n", tag, (int)searched, t->dir.idle_upkeeps);
  if (!upkeep) t->dir.exact = false;
  return upkeep;
}

// k_upper's view of the directory (u.par is set) and, for a chunk that keeps
// it, the upkeep's arguments
int dir_chunk_args(shm_tree* t, hipStream_t s, bool upkeep, dev::UpperArgs& u) {
  set_dir(t, u);
  if (u.dir) u.dir_hint = t->dir.hint;
  if (u.dir && upkeep) {  // the chunk's directory upkeep after its k_upper (dir_upkeep.h)
    // the first kept chunk after chunks that were not: its parity's list
    // count may still hold the count of the last kept chunk of that parity
    // (each repair zeroes only the other parity's, for the chunk after it)
    if (!t->dir.last_upkept) HIP_OK(hipMemsetAsync(t->dir.fix_n + u.par, 0, sizeof(uint32_t), s));
    u.dir_w = t->dir.ent;
    u.dir_form = t->dir.pairs ? dev::kDirFormPairs : dev::kDirFormFp;
    u.dir_vals = t->dir.pairs && t->dir.vals ? 1u : 0u;
    // the upkeep reads this chunk's op buffers after k_upper: they are
    // published free by k_dir_repair
    u.pub_later = 1u;
    u.dir_fix = t->dir.fix;
    u.dir_fix_n = t->dir.fix_n;
    u.dir_fix_cap = t->dir.fix_cap;
    if (vt_trusted(t)) {  // the same launch keeps the bucket table
      set_vt(t, u);
      u.vt_ctr = t->vt.ctr;
    }
  }
  u.pub_always = t->next_page != t->dir.np ? 1u : 0u;
  return SHM_OK;
}

// after the chunk's k_upper: its two upkeep launches, if it keeps the directory
int dir_chunk_upkeep(shm_tree* t, hipStream_t s, const dev::UpperArgs& u, uint64_t n,
                     uint32_t tag) {
  t->dir.last_upkept = u.dir_w != nullptr;
  if (u.dir_w) {
    // the chunk's directory upkeep (new keys' pairs / fingerprints, split
    // pages' prefixes), then the entries it listed rebuilt from the tree
    dev::launch_dir_upkeep(u, t->oslot, t->pages, op_counts(t, tag) + 0, n, s);
    DBG(s, "dir_upkeep");
    dev::launch_dir_repair(t->arena, t->arena_bytes, t->cfg.node_id, t->root, u.dir_lo,
                           u.dir_shift, u.dir_n, t->dir.ent, t->dir.hint, (int)u.dir_form, t->dir.fix,
                           t->dir.fix_n, u.par, t->dir.fix_cap, u.pub + dev::kPubDirLost,
                           t->d_err, s, (int)u.dir_vals, (uint64_t)tag);
    DBG(s, "dir_repair");
  }
  return SHM_OK;
}

// ---- create, free, and the calls that replace the tree's contents ----------
int dir_create(shm_tree* t, uint64_t n) {
  t->dir.maint = dir_maint_enabled();
  // SHM_DIR_VALS=0: builds and upkeep leave the entries in plain pair form
  // (read per tree, so one process can run both)
  t->dir.vals = env_on("SHM_DIR_VALS", true);
  // SHM_VALTAB=0: no bucket table (A/B); SHM_VALTAB_MAX_BYTES: its byte limit
  t->vt.on = env_on("SHM_VALTAB", true);
  if (const char* m = getenv("SHM_VALTAB_MAX_BYTES")) t->vt.max_bytes = strtoull(m, nullptr, 0);
  // SHM_GET_COOP=0 / SHM_GET_PACK=0: the get's probe and fall-through in
  // the form before each (A/B; kernels.h WalkArgs)
  t->vt.get_coop = env_on("SHM_GET_COOP", true);
  t->vt.get_pack = env_on("SHM_GET_PACK", true);
  t->dir.fix_cap = (uint32_t)std::max<uint64_t>(n, 1u << 16);
  return dalloc(&t->dir.fix, t->dir.fix_cap) | dalloc(&t->dir.fix_n, 32);
}
hipError_t dir_fix_clear(shm_tree* t, hipStream_t s) {
  return hipMemsetAsync(t->dir.fix_n, 0, sizeof(uint32_t) * 32, s);
}
void dir_free(shm_tree* t) {
  auto F = [](void* p) {
    if (p) (void)hipFree(p);
  };
  F(t->dir.fix); F(t->dir.fix_n); F(t->vt.tab); F(t->vt.ctr); F(t->dir.ent); F(t->dir.hint);
  F(t->top.keys); F(t->top.pages); F(t->top.scratch);
  for (hipEvent_t e : t->dir.ev)
    if (e) (void)hipEventDestroy(e);
}
void dir_invalidate(shm_tree* t, bool table, bool new_range) {
  t->dir.valid = false;  // contents changed: rebuild the leaf directory
  t->dir.hint_ok = false;    // ... from the root
  t->top.valid = false;
  // the bucket table is trusted only beside a valid directory (vt_trusted) and
  // the directory's next build replaces it (vt_build); dropped here as well
  if (table) t->vt.valid = false;
  // the table was dropped at this size because of the old range's dead buckets
  if (new_range) t->vt.drop_bits = 0;
}
void dir_tag_reset(shm_tree* t, uint64_t tag) {
  t->dir.pub_seen = tag;  // with pub_batch: no quiet-rule look is pending
  t->dir.last_upkept = false;  // both parities' repair list counts are unknown again
}
}  // namespace host
}  // namespace shm

extern "C" {

int shm_dir_stats(shm_tree* t, shm_dir_stats_t* out) {
  if (!t || !out) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  memset(out, 0, sizeof(*out));
  if (const int rc = dir_poll(t, true)) return rc;
  mirror(t);
  out->form = !t->dir.valid ? 0u : t->dir.pairs ? 2u : 1u;
  out->bits = t->dir.valid ? t->dir.bits : 0u;
  out->entries = t->dir.valid ? 1ull << t->dir.bits : 0ull;
  out->bytes = t->dir.ent ? (1ull << t->dir.cap_bits) * (8 * kDirWords + 8) : 0ull;
  out->builds = t->dir.builds;
  out->pages_at_build = t->dir.np;
  out->pages_since_build = t->next_page > t->dir.np ? t->next_page - t->dir.np : 0ull;
  out->last_build_ms = t->dir.last_ms;
  out->total_build_ms = t->dir.total_ms;
  out->maintained = t->dir.maint ? 1u : 0u;
  out->exact = t->dir.valid && t->dir.exact ? 1u : 0u;
  return SHM_OK;
}

// test hook: directory upkeep on / off for this tree (maint < 0: as is; 2:
// on for every chunk, also those with no search before them) and
// a cap on the bytes a directory allocation may take (0: none), as a device
// short of memory would impose
int shm__dir_config(shm_tree* t, int maint, uint64_t mem_limit) {
  if (!t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  if (maint >= 0) t->dir.maint = maint != 0;
  if (maint >= 0) t->dir.maint_always = maint == 2;
  if (!t->dir.maint) t->dir.exact = false;  // until the next build
  t->dir.mem_limit = mem_limit;
  return SHM_OK;
}

// test hook: the get's forms for this tree's later launches (as SHM_GET_COOP /
// SHM_GET_PACK set them at its creation; < 0: as is), so one tree's state can
// be read in every form
int shm__get_forms(shm_tree* t, int coop, int pack) {
  if (!t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  if (coop >= 0) t->vt.get_coop = coop != 0;
  if (pack >= 0) t->vt.get_pack = pack != 0;
  return SHM_OK;
}

// diagnostics: every entry the walks trust against the tree as it is now
// (k_dir_verify): out[0] checked, out[1..3] bad leaf lists / pair sets /
// fingerprint copies, out[4..7] first bad prefixes + 1, out[8..9] value-form
// entries checked / wrong (kDirVerifyWords words)
int shm__dir_verify(shm_tree* t, uint64_t* out) {
  if (!t || !out) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  constexpr size_t kBytes = dev::kDirVerifyWords * sizeof(uint64_t);
  memset(out, 0, kBytes);
  HIP_OK(hipDeviceSynchronize());
  if (!t->dir.valid) return SHM_OK;
  unsigned long long* d = nullptr;
  if (dalloc(&d, dev::kDirVerifyWords)) return SHM_ENOMEM;
  int rc = SHM_OK;
  if (hipMemset(d, 0, kBytes) != hipSuccess) rc = SHM_EIO;
  if (!rc) {
    dev::launch_dir_verify(t->arena, t->arena_bytes, t->cfg.node_id, t->root, t->cfg.key_lo,
                           t->cfg.key_bits - t->dir.bits, 1ull << t->dir.bits, t->dir.ent, t->dir.hint,
                           d, t->stream);
    if (hipStreamSynchronize(t->stream) != hipSuccess ||
        hipMemcpy(out, d, kBytes, hipMemcpyDeviceToHost) != hipSuccess)
      rc = SHM_EIO;
  }
  (void)hipFree(d);
  return rc;
}

// test hook: the raw directory, for a host-side check that shares no code
// with the kernels (tests/dir_model.py).  Copies up to cap_entries 64 B
// entries into buf (nullable: sizes only); info = {entries, dir_lo, shift,
// form (shm_dir_stats' coding)}, entries 0 while no directory is valid.
int shm__dir_dump(shm_tree* t, void* buf, uint64_t cap_entries, uint64_t* info) {
  if (!t || !info) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  memset(info, 0, 4 * sizeof(uint64_t));
  HIP_OK(hipDeviceSynchronize());
  if (!t->dir.valid || !t->dir.ent) return SHM_OK;
  const uint64_t n = 1ull << t->dir.bits;
  info[0] = n;
  info[1] = t->cfg.key_lo;
  info[2] = t->cfg.key_bits - t->dir.bits;
  info[3] = t->dir.pairs ? 2u : 1u;
  if (!buf) return SHM_OK;
  if (cap_entries < n) return SHM_EINVAL;
  HIP_OK(hipMemcpy(buf, t->dir.ent, n * 8 * kDirWords, hipMemcpyDeviceToHost));
  return SHM_OK;
}

// test hook: the bucket table (valtab.h): out = {buckets, bytes, dead
// buckets now, stored keys in dead buckets at the last build, stored keys
// then, trusted}; all 0 without a table
int shm__vt_stats(shm_tree* t, uint64_t* out) {
  if (!t || !out) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  memset(out, 0, 6 * sizeof(uint64_t));
  if (const int rc = vt_poll(t, true)) return rc;
  HIP_OK(hipDeviceSynchronize());
  if (!t->vt.tab || !t->vt.valid) return SHM_OK;
  out[0] = 1ull << t->vt.bits;
  out[1] = t->vt.bytes;
  HIP_OK(hipMemcpy(out + 2, t->vt.ctr, sizeof(uint64_t), hipMemcpyDeviceToHost));
  out[3] = t->vt.dead_keys;
  out[4] = t->vt.keys;
  out[5] = vt_trusted(t) ? 1u : 0u;
  return SHM_OK;
}

// test hook: the raw buckets (16 u64 each) for a host-side check
// (tests/valtab_model.py), in the style of shm__dir_dump; info = {buckets,
// lo, shift, trusted}, buckets 0 without a table
int shm__vt_dump(shm_tree* t, void* buf, uint64_t cap_buckets, uint64_t* info) {
  if (!t || !info) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  memset(info, 0, 4 * sizeof(uint64_t));
  if (const int rc = vt_poll(t, true)) return rc;
  HIP_OK(hipDeviceSynchronize());
  if (!t->vt.tab || !t->vt.valid) return SHM_OK;
  const uint64_t n = 1ull << t->vt.bits;
  info[0] = n;
  info[1] = t->cfg.key_lo;
  info[2] = t->cfg.key_bits - t->vt.bits;
  info[3] = vt_trusted(t) ? 1u : 0u;
  if (!buf) return SHM_OK;
  if (cap_buckets < n) return SHM_EINVAL;
  HIP_OK(hipMemcpy(buf, t->vt.tab, n * 8 * dev::kVtBucketWords, hipMemcpyDeviceToHost));
  return SHM_OK;
}
}  // extern "C"
