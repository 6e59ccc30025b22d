// tree.cpp — host runtime behind the C-ABI (include/sherman_amd.h).
//
// Owns one shard's HBM page arena, lock table and batch workspace, and issues
// the kernels of get.hip / get_sum.hip / get_side.hip / isort.hip /
// upsert.hip / insert.hip / range.hip / tile_scan.hip / service.hip.  The roles of the reference's DSM (include/DSM.h:33-176: remote
// read/write/CAS, alloc), the Directory's root publication
// (src/Directory.cpp:72-83) and the Local/GlobalAllocator
// (include/LocalAllocator.h, GlobalAllocator.h) are taken by: plain HBM
// pointers, a device bump allocator (the superblock's next_page in page 0,
// advanced by k_upper) and a root page that never moves.  An insert batch is
// issued without any host wait: the host keeps a lagging mirror of the
// superblock (published by k_upper into mapped host memory) for heuristics
// only (directory staleness, get ordering) and reads exact values at
// synchronising calls.
//
// This unit: the handle's lifecycle (config, create, destroy) and the plumbing
// every other unit uses -- the cross-stream ordering (follow / note / Order),
// the superblock mirror, the zero-copy read-back, the error word, the env
// flags, SHM_DEBUG -- with the calls that only report (stats, last error,
// synchronize).  The directory is in tree_dir.cpp, inserts in
// tree_insert.cpp, gets / ranges / scans in tree_read.cpp, images, bulk load
// and export in tree_image.cpp, profiling in tree_prof.cpp, routing in
// tree_route.cpp; tree_internal.h is what they share.
#include "tree_internal.h"

namespace shm {
namespace host __attribute__((visibility("hidden"))) {

constexpr uint32_t kDefaultSortBits = 16; // top key bits that order gets (8 + 8)
constexpr uint32_t kFlagWord = 512;        // read-back sequence word: byte 2048 of h_pin

// Cross-stream ordering events of one device: recording one needs no
// system-scope release and waiting on one no system-scope acquire (the
// streams share the device's memory; the host reads device results through
// copies or the read-back kernel's own system-scope fence, never through
// these events).  Default HIP events fence at system scope: a write-back of
// the L2s at every record, measured as 12-22 us gaps around each C5 step's
// cross-stream wait (round 4 A/B, tools/ab_events.sh: C2 +0.7 %, C3 +4.7 %,
// C5 +3.1 % with device scope; the system-fence switch is gone).
unsigned event_flags() { return (unsigned)(hipEventDisableTiming | hipEventDisableSystemFence); }

// INVARIANT: events from new_event() order streams of this device and
// nothing else.  They are only ever passed to hipEventRecord and
// hipStreamWaitEvent; never host-queried (hipEventSynchronize /
// hipEventQuery) and never relied on to make device writes visible to the
// host or to another device: with hipEventDisableSystemFence their record
// does not write back the L2s.  Host-facing completion goes through
// take_event() (HIP's default events: the profiler's timing) or the
// read-back kernel's system-scope release (readback below).
hipEvent_t new_event() {
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, event_flags()) != hipSuccess) return nullptr;
  return e;
}

// stream s follows the call mark m notes (its stream's tail, recorded at the
// first wait: shm_tree::Mark)
int follow(shm_tree::Mark& m, hipStream_t s) {
  if (!m.valid || m.s == s) return SHM_OK;
  if (!m.recorded) {
    if (!m.ev) m.ev = new_event();
    if (!m.ev || hipEventRecord(m.ev, m.s) != hipSuccess) return SHM_EIO;
    m.recorded = true;
  }
  return hipStreamWaitEvent(s, m.ev, 0) == hipSuccess ? SHM_OK : SHM_EIO;
}
void note(shm_tree::Mark& m, hipStream_t s) {
  m.s = s;
  m.valid = true;
  m.recorded = false;
}

// Order (tree_internal.h): the waits of a call's start ...
Order::Order(shm_tree* tt, hipStream_t ss, bool exclusive) : t(tt), s(ss), ex(exclusive) {
  wait(t->sync.ex);
  if (ex) {
    for (auto& m : t->sync.shared_ev) wait(m);
    for (int j = 0; j < 2; ++j) wait(t->sync.gws_m[j]);
  }
}
void Order::make_exclusive() {
  if (ex) return;
  ex = true;
  for (auto& m : t->sync.shared_ev) wait(m);
  for (int j = 0; j < 2; ++j) wait(t->sync.gws_m[j]);
}
int Order::take_ws() {
  ws = t->sync.next_gws;
  t->sync.next_gws ^= 1;
  if (!ex) wait(t->sync.gws_m[ws]);
  return ws;
}
void Order::wait(shm_tree::Mark& m) {
  if (follow(m, s) != SHM_OK) rc = SHM_EIO;
}
// ... and the notes of its end
Order::~Order() {
  if (ex) {
    // the waits above ordered this call after every earlier one
    note(t->sync.ex, s);
    for (auto& m : t->sync.shared_ev) m.valid = false;
    t->sync.gws_m[0].valid = t->sync.gws_m[1].valid = false;
    return;
  }
  shm_tree::Mark* r = nullptr;
  for (auto& m : t->sync.shared_ev)
    if (m.s == s) r = &m;
  if (!r) {
    for (auto& m : t->sync.shared_ev)
      if (!m.valid) r = &m;  // a slot of a stream no call waits for any more
    if (!r) {
      t->sync.shared_ev.push_back(shm_tree::Mark{});
      r = &t->sync.shared_ev.back();
    }
  }
  note(*r, s);
  if (ws >= 0) note(t->sync.gws_m[ws], s);
}

// the superblock mirror k_upper publishes into h_pin (kPubWord): {chunk tag,
// next_page, root_level, splits}; exact once the device is idle
void mirror(shm_tree* t) {
  const volatile uint64_t* p = pub_words(t);
  t->pub_batch = p[0];  // first: the words below are at least this chunk's
  t->next_page = p[1];
  t->root_level = (uint32_t)p[2];
  t->splits = p[3];
}

void publish_host(shm_tree* t) {
  volatile uint64_t* p = pub_words(t);
  p[1] = t->next_page;
  p[2] = t->root_level;
  p[3] = t->splits;
  p[0] = t->chunks;
}

// The look-back kernels' block-index counters (lookback_index): the
// ordering's bin prefix (k_bin_unique: 256 blocks, one per CU; two ranks on
// one GPU spun on each other with blockIdx, kErrBinSpin) and the scans take a
// ticket, which costs nothing measurable there.  k_seg_fill keeps blockIdx:
// its 1024 blocks per C5 chunk serialised on a counter (C5 5.19-5.23 K
// against 5.33-5.38 K Mops/s, round-4 A/B), and it needs none for forward
// progress: a tile that waits too long for an earlier tile counts that
// tile's staged heads itself (seg_tile.h).
uint32_t* lb_ctr(shm_tree* t, int which) {
  return which == dev::kLbSeg ? nullptr : t->ctl->lb_ids[which];
}

// the first character of an env variable (0: unset or empty)
static char env_char(const char* name) {
  const char* e = getenv(name);
  return e ? e[0] : 0;
}
bool env_on(const char* name, bool dflt) {
  const char c = env_char(name);
  return dflt ? c != '0' : c == '1';
}
int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// SHM_DEBUG=1: synchronise after every launch and name the failing step
// (diagnostics only; the launch sequence is the same)
// SHM_DEBUG=2: also name every step as it completes (a hang's last line)
int dbg(hipStream_t s, const char* what) {
  static const char level = env_char("SHM_DEBUG");
  if (level != '1' && level != '2') return SHM_OK;
  hipError_t e = hipStreamSynchronize(s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "sherman_amd[debug]: %s failed: %s\n", what, hipGetErrorString(e));
    return SHM_EIO;
  }
  if (level == '2') fprintf(stderr, "sherman_amd[debug]: %s done\n", what);
  return SHM_OK;
}

// Read `bytes` (<= 256) of device words into pinned host scratch and wait.
// A one-wave kernel stores the words straight into the mapped, coherent host
// page, then a sequence number after a system-scope fence; the host spins on
// that word instead of a D2H copy (an SDMA/blit round trip) and a stream
// synchronisation.  While spinning it polls the stream, so a fault in an
// earlier kernel (which would keep the word from ever arriving) still returns
// SHM_EIO.
int readback(shm_tree* t, hipStream_t s, const void* src, size_t bytes, int clear) {
  const uint32_t seq = ++t->rb_seq;
  dev::launch_readback(t->h_pin_dev, static_cast<const uint32_t*>(src),
                       (uint32_t)((bytes + 3) / 4), t->h_pin_dev + kFlagWord, seq, clear, s);
  HIP_OK(hipGetLastError());
  const uint32_t* flag = reinterpret_cast<const uint32_t*>(t->h_pin) + kFlagWord;
  for (uint32_t spin = 1;; ++spin) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return SHM_OK;
    if ((spin & 1023) == 0) {
      const hipError_t e = hipStreamQuery(s);
      if (e != hipSuccess && e != hipErrorNotReady) return SHM_EIO;
      if (e == hipSuccess && __atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) return SHM_EIO;
    }
    __builtin_ia32_pause();
  }
}

// the host's superblock written by a one-wave kernel (create / load_image);
// afterwards k_upper owns next_page, root_level, splits and batches
int write_superblock(shm_tree* t, hipStream_t s) {
  Superblock sb{};
  sb.magic = kSuperMagic;
  sb.root_ptr = t->root;
  sb.root_level = t->root_level;
  sb.next_page = t->next_page;
  sb.capacity_pages = t->cap_pages;
  sb.node_id = t->cfg.node_id;
  sb.batches = t->chunks;
  sb.splits = t->splits;
  dev::launch_write_superblock(t->arena, sb, s);
  HIP_OK(hipGetLastError());
  publish_host(t);
  return SHM_OK;
}

// device error block -> status.  Word 0 holds the bits (kErrKeyMax: a chunk
// with kKeyMax was rejected whole; kErrNoMem: the arena ran out, splits left
// unapplied; kErrHandoff: a chunk's k_upper gave up at a hand-off and its
// last block completed the chunk alone -- word 2 counts those chunks; the
// rest: a tree inconsistency or a kernel bound, SHM_EIO), word 1 the first
// insert chunk that saw a bit (0: none did).  The words are taken by atomic
// exchange (readback clear), so a bit set by another stream after the read
// stays for the next call.  shm_last_error reports what was read.
int check_err(shm_tree* t, hipStream_t s) {
  t->err_pending = false;
  int rc = readback(t, s, t->d_err, 3 * sizeof(uint32_t), 1);
  if (rc) return rc;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(t->h_pin);
  const uint32_t e = w[0], chunk = w[1], resumed = w[2];
  mirror(t);  // the stream is idle up to here: the mirror is exact
  t->last_error.resumed += resumed;
  if (!e) return SHM_OK;
  t->sticky_err |= e;
  const uint32_t other = e & ~(dev::kErrKeyMax | kErrNoMem | kErrHandoff);
  rc = other ? SHM_EIO : (e & kErrNoMem) ? SHM_ENOMEM : (e & dev::kErrKeyMax) ? SHM_EINVAL : SHM_OK;
  t->last_error.bits = e;
  t->last_error.chunk = chunk;
  t->last_error.status = rc;
  if (other) fprintf(stderr, "sherman_amd: device error bits 0x%x (first seen by chunk %u)\n", e, chunk);
  return rc;
}

void free_all(shm_tree* t) {
  auto F = [](void* p) {
    if (p) (void)hipFree(p);
  };
  F(t->arena); F(t->locks); F(t->stamps); F(t->d_err); F(t->d_counts); F(t->route_scratch);
  for (auto& r : t->route_ws)
    if (r.second != t->route_scratch) F(r.second);
  F(t->ka); F(t->kb); F(t->ia); F(t->ib); F(t->ic); F(t->kc); F(t->id); F(t->part_mx); F(t->part_mt);
  F(t->uk); F(t->uv); F(t->dk); F(t->pages); F(t->seg_lb); F(t->bsum64);
  F(t->seg_start); F(t->seg_end); F(t->seg_page); F(t->seg_T); F(t->seg_P); F(t->seg_np);
  F(t->seg_ver); F(t->leaf_hw); F(t->sum); F(t->bulk_low); F(t->ex_ws); F(t->oidx.ws); F(t->oslot); F(t->pnew);
  F(t->ctl); F(t->leaf_rd);
  for (int i = 0; i < 2; ++i) { F(t->sep_key[i]); F(t->sep_ptr[i]); F(t->ipage[i]); }
  F(t->h_end); F(t->h_T); F(t->h_P); F(t->h_ver); F(t->h_lk);
  F(t->d_head); F(t->d_base); F(t->int_rd);
  F(t->part_hist); F(t->part_S); F(t->part_chunks); F(t->gcount); F(t->bins);
  dir_free(t);
  F(t->prof.idx_stats); F(t->prof.ins); F(t->prof.clk);
  for (auto& r : t->prof.pending)
    for (hipEvent_t e : r.e)
      if (e) t->prof.event_pool.push_back(e);
  for (hipEvent_t e : t->prof.event_pool) (void)hipEventDestroy(e);
  if (t->rstage) (void)hipFree(t->rstage);
  {
    shm_tree::GetWs& w = t->sync.gws[1];
    F(w.keys1); F(w.keys_out); F(w.pos1); F(w.src); F(w.M); F(w.S); F(w.chunks);
  }
  for (auto& r : t->sync.shared_ev)
    if (r.ev) (void)hipEventDestroy(r.ev);
  if (t->sync.ex.ev) (void)hipEventDestroy(t->sync.ex.ev);
  if (t->sync.ord.ev) (void)hipEventDestroy(t->sync.ord.ev);
  for (auto& m : t->sync.app_m)
    if (m.ev) (void)hipEventDestroy(m.ev);
  for (auto& pd : t->sync.pend)
    if (pd.ev) (void)hipEventDestroy(pd.ev);
  for (auto& m : t->sync.gws_m)
    if (m.ev) (void)hipEventDestroy(m.ev);
  if (t->h_pin) (void)hipHostFree(t->h_pin);
  if (t->stream) (void)hipStreamDestroy(t->stream);
}
}  // namespace host
}  // namespace shm

extern "C" {

int shm_abi_version(void) { return SHM_ABI_VERSION; }

const char* shm_strerror(int s) {
  switch (s) {
    case SHM_OK: return "ok";
    case SHM_EINVAL: return "invalid argument (key == kKeyMax or bad config)";
    case SHM_ENOMEM: return "page arena or workspace exhausted";
    case SHM_EIO: return "HIP failure or tree inconsistency";
    case SHM_EAGAIN: return "optimistic check failed";
    case SHM_E2BIG: return "batch larger than max_batch";
    case SHM_ENOSPC: return "output buffer too small";
    default: return "unknown status";
  }
}

int shm_config_init(shm_config* c) {
  if (!c) return SHM_EINVAL;
  memset(c, 0, sizeof(*c));
  c->struct_size = sizeof(shm_config);
  c->device = 0;
  c->node_id = 0;
  c->flags = SHM_FLAG_LEAF_DIR | SHM_FLAG_AUTO_SORT_GETS;
  c->arena_bytes = 1ull << 30;
  c->max_batch = 1ull << 20;
  // the reference's kNumOfLock (Common.h:87-93): 128 KB of lock words stay
  // cached at the memory side, where the atomics run (C5 locate 76 -> 69 us
  // against 4 Mi words; 2^17 measured the same as 2^14)
  c->num_locks = 16384;
  c->sort_bits = kDefaultSortBits;
  c->key_lo = 0;
  c->key_bits = 64;
  return SHM_OK;
}

int shm_tree_create(const shm_config* cfg, shm_tree** out) {
  if (!cfg || !out || cfg->struct_size != sizeof(shm_config)) return SHM_EINVAL;
  // arena < 4 TB: the leaf directory holds 32-bit page indices
  if (cfg->arena_bytes < 4 * kPageSize || cfg->arena_bytes > (1ull << 42) ||
      cfg->max_batch == 0 ||
      cfg->max_batch >= (1ull << 24) || cfg->num_locks == 0 ||
      (cfg->sort_bits != 0 && cfg->sort_bits != kDefaultSortBits) || cfg->key_bits > 64)
    return SHM_EINVAL;
  shm_tree* t = new shm_tree();
  t->cfg = *cfg;
  if (!t->cfg.sort_bits || t->cfg.sort_bits > 64) t->cfg.sort_bits = kDefaultSortBits;
  if (t->cfg.key_bits == 0) t->cfg.key_bits = 64;
  if (t->cfg.key_bits == 64) t->cfg.key_lo = 0;
  auto fail = [&](int rc) {
    free_all(t);
    delete t;
    return rc;
  };
  if (hipSetDevice(cfg->device) != hipSuccess) return fail(SHM_EIO);
  // k_upper's grid barriers need one resident 512-thread block per CU
  if (!dev::upper_resident()) {
    fprintf(stderr, "sherman_amd: k_upper blocks do not fit a CU\n");
    return fail(SHM_EIO);
  }
  if (hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking) != hipSuccess)
    return fail(SHM_EIO);
  t->cap_pages = cfg->arena_bytes / kPageSize;
  t->arena_bytes = t->cap_pages * kPageSize;
  const uint64_t n = cfg->max_batch;
  t->nmax = n;
  t->sep_cap = 2 * n + 1024;
  const uint64_t segcap = t->sep_cap;
  int rc = SHM_OK;
  rc |= dalloc(&t->arena, t->arena_bytes);
  rc |= dalloc(&t->locks, cfg->num_locks);
  rc |= dalloc(&t->d_err, 4);
  rc |= dalloc(&t->d_counts, 32);
  rc |= dalloc(&t->route_scratch, dev::route_scratch_words(n));
  rc |= dalloc(&t->ka, n);
  rc |= dalloc(&t->kb, n);
  rc |= dalloc(&t->ia, n);
  rc |= dalloc(&t->ib, n);
  rc |= dalloc(&t->ic, n);
  rc |= dalloc(&t->kc, n);
  rc |= dalloc(&t->id, n);
  rc |= dalloc(&t->uk, 2 * n);  // two parities (op_keys)
  rc |= dalloc(&t->uv, 2 * n);
  rc |= dalloc(&t->dk, 2 * n);
  rc |= dalloc(&t->pages, segcap);
  rc |= dalloc(&t->seg_lb, dev::seg_tiles(segcap) + 1);
  rc |= dalloc(&t->bsum64, dev::seg_tiles(n) + 1);
  rc |= dalloc(&t->seg_start, segcap + 1);
  rc |= dalloc(&t->seg_end, segcap);
  rc |= dalloc(&t->seg_page, segcap);
  rc |= dalloc(&t->seg_T, segcap);
  rc |= dalloc(&t->seg_P, segcap);
  rc |= dalloc(&t->seg_np, segcap);
  rc |= dalloc(&t->seg_ver, segcap);
  rc |= dalloc(&t->leaf_hw, t->cap_pages);
  rc |= dalloc(&t->sum, t->cap_pages * kSumBytes);
  rc |= dalloc(&t->oslot, n);
  rc |= dalloc(&t->pnew, t->cap_pages);
  rc |= dalloc(&t->ctl, 1);
  rc |= dir_create(t, n);
  rc |= dalloc(&t->leaf_rd, segcap);
  for (int i = 0; i < 2; ++i) {
    rc |= dalloc(&t->sep_key[i], t->sep_cap);
    rc |= dalloc(&t->sep_ptr[i], t->sep_cap);
    rc |= dalloc(&t->ipage[i], t->sep_cap);
  }
  rc |= dalloc(&t->h_end, t->sep_cap);
  rc |= dalloc(&t->h_T, t->sep_cap);
  rc |= dalloc(&t->h_P, t->sep_cap);
  rc |= dalloc(&t->h_ver, t->sep_cap);
  rc |= dalloc(&t->h_lk, t->sep_cap);
  rc |= dalloc(&t->d_head, t->sep_cap);
  rc |= dalloc(&t->d_base, t->sep_cap);
  rc |= dalloc(&t->int_rd, t->sep_cap);
  rc |= dalloc(&t->part_hist, dev::kPartHistWords);
  rc |= dalloc(&t->part_S, dev::kPartGroupWords);
  rc |= dalloc(&t->part_mx, dev::kPartHistWords);
  rc |= dalloc(&t->part_mt, dev::kPartHistWords);
  rc |= dalloc(&t->part_chunks, 2 * (uint64_t)dev::partition_chunk_slots(n));
  rc |= dalloc(&t->gcount, n / dev::kIsortTile + 1);
  rc |= dalloc(&t->bins, 4 * dev::kCoarse);  // (start, count) per bin, then the bins' tagged counts
  // get workspaces: 0 shares the insert arrays, 1 is its own
  t->sync.gws[0] = {t->kb, t->ka, t->ia, t->ib, t->part_hist, t->part_S, t->part_chunks};
  {
    shm_tree::GetWs& w = t->sync.gws[1];
    rc |= dalloc(&w.keys1, n);
    rc |= dalloc(&w.keys_out, n);
    rc |= dalloc(&w.pos1, n);
    rc |= dalloc(&w.src, n);
    rc |= dalloc(&w.M, dev::kPartHistWords);
    rc |= dalloc(&w.S, dev::kPartGroupWords);
    rc |= dalloc(&w.chunks, 2 * (uint64_t)dev::partition_chunk_slots(n));
  }
  if (rc) return fail(SHM_ENOMEM);
  if (hipHostMalloc((void**)&t->h_pin, 4096, hipHostMallocMapped | hipHostMallocCoherent) !=
          hipSuccess ||
      hipHostGetDevicePointer((void**)&t->h_pin_dev, t->h_pin, 0) != hipSuccess)
    return fail(SHM_ENOMEM);
  memset(t->h_pin, 0, 4096);
  hipStream_t s = t->stream;
  if (hipMemsetAsync(t->locks, 0, sizeof(uint64_t) * cfg->num_locks, s) ||
      hipMemsetAsync(t->d_err, 0, 16, s) ||
      hipMemsetAsync(t->seg_lb, 0, sizeof(uint64_t) * (dev::seg_tiles(segcap) + 1), s) ||
      hipMemsetAsync(t->bsum64, 0, sizeof(uint64_t) * (dev::seg_tiles(n) + 1), s) ||
      hipMemsetAsync(t->ctl, 0, sizeof(dev::UpperCtl), s) ||
      dir_fix_clear(t, s) ||
      hipMemsetAsync(t->bins, 0, sizeof(uint32_t) * 4 * dev::kCoarse, s) ||
      hipMemsetAsync(t->leaf_rd, 0, sizeof(uint64_t) * segcap, s) ||
      hipMemsetAsync(t->int_rd, 0, sizeof(uint64_t) * t->sep_cap, s) ||
      hipMemsetAsync(t->part_S, 0, sizeof(uint32_t) * dev::kPartGroupWords, s) ||
      hipMemsetAsync(t->sync.gws[1].S, 0, sizeof(uint32_t) * dev::kPartGroupWords, s) ||
      hipMemsetAsync(t->arena, 0, kPageSize, s) ||
      hipMemsetAsync(t->leaf_hw, kLeafHwFull, t->cap_pages, s) ||
      hipMemsetAsync(t->sum, 0, t->cap_pages * kSumBytes, s) ||
      hipMemsetAsync(t->pnew, 0, t->cap_pages, s))
    return fail(SHM_EIO);
  // Tree::Tree (Tree.cpp:44-60): empty leaf root
  t->next_page = 1;
  const uint64_t root_off = t->next_page * kPageSize;
  dev::launch_empty_leaf(t->arena, root_off, t->sum, s);
  t->next_page += 1;
  t->root = ga_make(cfg->node_id, root_off);
  t->root_level = 0;
  if (write_superblock(t, s)) return fail(SHM_EIO);
  if (hipStreamSynchronize(s) != hipSuccess) return fail(SHM_EIO);
  *out = t;
  return SHM_OK;
}

uint64_t shm_tree_max_batch(const shm_tree* t) { return t ? t->nmax : 0; }

int shm_tree_destroy(shm_tree* t) {
  if (!t) return SHM_EINVAL;
  (void)hipSetDevice(t->cfg.device);
  (void)hipDeviceSynchronize();
  free_all(t);
  delete t;
  return SHM_OK;
}

// Library-internal, not part of include/sherman_amd.h: the tree's sticky
// device error word (shard.cpp's kernels report into it, so the next
// synchronising call on the tree returns their errors)
uint32_t* shm__error_word(shm_tree* t) { return t ? t->d_err : nullptr; }

int shm_stats(shm_tree* t, shm_stats_t* o) {
  if (!t || !o) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  HIP_OK(hipDeviceSynchronize());
  mirror(t);  // exact: the device is idle
  memset(o, 0, sizeof(*o));
  o->root_ptr = t->root;
  o->root_level = t->root_level;
  o->height = t->root_level + 1;
  o->pages_used = t->next_page - 1;
  o->pages_capacity = t->cap_pages - 1;
  o->arena_bytes = t->arena_bytes;
  o->batches = t->batches;
  o->splits = t->splits;
  o->last_error = t->sticky_err;
  return SHM_OK;
}

int shm_read_words(shm_tree* t, const void* src, uint64_t bytes, void* host_out,
                   void* stream) {
  if (!t || !src || !host_out || bytes == 0 || bytes > 1024 || (bytes & 3)) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  const int rc = readback(t, pick(stream), src, bytes);
  if (rc) return rc;
  memcpy(host_out, t->h_pin, bytes);
  return SHM_OK;
}

int shm_last_error(shm_tree* t, shm_error_t* out, int reset) {
  if (!t || !out) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  *out = t->last_error;
  if (reset) {
    const uint32_t resumed = t->last_error.resumed;
    t->last_error = shm_error_t{};
    t->last_error.resumed = resumed;
  }
  return SHM_OK;
}

uint32_t shm_last_chunk(shm_tree* t) {
  if (!t) return 0;
  std::lock_guard<std::mutex> g(t->mu);
  return t->chunks;
}

int shm_synchronize(shm_tree* t) {
  if (!t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  HIP_OK(hipDeviceSynchronize());
  return check_err(t, t->stream);
}
}  // extern "C"
