// tree_insert.cpp — the insert pipeline.
//
// One insert chunk is an ordering (insert_order: the batch sorted, deduplicated
// and split into upserts and deletes, in the op buffers of the chunk tag's
// parity) and an apply (insert_apply: locate, segmentation, leaf upsert,
// k_upper, and the directory's upkeep where tree_dir.cpp says so), queued
// without a host wait.  Around them: the flow control between orderings and
// applies on different streams, the chunk counter's epoch (epoch_reset), the
// insert and delete calls of the C-ABI, and the hooks that force a path of
// k_upper, move the counters or read an ordered chunk.
#include "tree_internal.h"

namespace shm {
namespace host __attribute__((visibility("hidden"))) {

constexpr int kAppWaitMs = 5;             // insert_order's host wait before an event fallback
// polls of an earlier segmentation tile's word before a tile counts that
// tile's staged heads itself (seg_tile.h; ~1 ms, far past a placed tile's
// few microseconds)
constexpr uint32_t kSegSelfAfter = 1024;

// the op buffers of chunk tag's parity (the ordering's outputs)
uint64_t* op_keys(shm_tree* t, uint32_t tag) { return t->uk + (uint64_t)(tag & 1u) * t->nmax; }
uint64_t* op_vals(shm_tree* t, uint32_t tag) { return t->uv + (uint64_t)(tag & 1u) * t->nmax; }
uint64_t* op_dels(shm_tree* t, uint32_t tag) { return t->dk + (uint64_t)(tag & 1u) * t->nmax; }
// {upserts, deletes} of the chunk (k_bin_unique)
uint64_t* op_counts(shm_tree* t, uint32_t tag) { return t->d_counts + 16 * (tag & 1u); }

// One insert chunk (n <= nmax ops), issued without a host wait:
//   1. ordering: k_tile_dedup, coarse partition, k_bin_unique
//      -> uk / uv (upserts, key order, last writer) and dk (deletes); counts
//      stay on the device (d_counts[0..1]);
//   2. k_locate: each upsert's leaf from the leaf directory (summary or
//      header walk); an op whose key its leaf holds is applied right there
//      (lock word, one entry write);
//   3. segmentation (k_seg_count, k_seg_fill_scan): only the runs of ops
//      on a page that gets a new key are listed (the upsert stages them);
//   4. k_leaf_upsert_pipe: lock words with the page DMAs, in-place upserts,
//      splits flagged and counted;
//   5. k_upper: leaf splits, parent levels, root growth, unlocks, the
//      chunk's deletes, superblock.
// step 1: it reads only the batch and writes the insert workspace
int insert_order(shm_tree* t, hipStream_t s, const uint64_t* keys, const uint64_t* vals,
                 uint64_t n, uint32_t tag, bool skip_pad) {
  // the scratch's last user (the previous ordering) and the op buffers'
  // (the apply of tag - 2), when they ran on another stream
  if (const int rc = follow(t->sync.ord, s)) return rc;
  const uint32_t p = tag & 1u;
  // The apply of tag - 2 (another stream) last read these op buffers.  Flow
  // control on the host: its k_upper publishes its tag in the host mirror
  // once it is done with them, and this call waits for that (in a pipeline
  // the host then runs at most about two chunks ahead of the device).  The
  // apply's stream gets no event record (≈ 4.6 µs of idle device between
  // kernels, tools/event_gap.hip), and the device no polling wait (a
  // wait-value kernel: a profiler that serialises kernels deadlocks on it).
  // A wait past kAppWaitMs (5 ms: the apply's stream held up by the caller,
  // or the card shared) falls back to an event at that stream's tail, so a
  // stalled apply costs this call (which holds the tree's mutex) at most
  // that long on the host.
  if (t->sync.app_valid[p] && t->sync.app_m[p].s != s) {
    const volatile uint64_t* ap = pub_words(t) + dev::kPubApplied;
    if (*ap < t->sync.app_tag[p]) {
      const auto t0 = std::chrono::steady_clock::now();
      while (*ap < t->sync.app_tag[p] &&
             std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(kAppWaitMs))
        std::this_thread::yield();
      if (*ap < t->sync.app_tag[p])
        if (const int rc = follow(t->sync.app_m[p], s)) return rc;
    }
  }
  // Tile mode (chunks of <= kMaxTiles tiles, i.e. <= 1 Mi ops): the tiles
  // write their survivors sorted by coarse bin and k_bin_unique gathers its
  // bin's runs from every tile, so there is no coarse scatter pass (round 4:
  // C3 9612 -> 10231, C5 4425 -> 4703 Mops/s); a larger chunk takes the
  // coarse pass.  The tiles' output
  // (kb / ia) stays live through k_bin_unique, so a bin over kUniqCap ops
  // sorts in ka / ib with kc / id as scratch and ic for its ranks.
  const uint64_t tiles = (n + dev::kIsortTile - 1) / dev::kIsortTile;
  const bool tile_mode = tiles <= (uint64_t)dev::kMaxTiles;
  // tile mode: M and Mx bin-major in part_mt / part_mx (part_hist keeps the
  // coarse pass's tile-major layout for the other path and ordered gets)
  dev::launch_tile_dedup(keys, n, t->kb, t->ia, t->gcount, t->d_err, &t->ctl->gate, tag,
                         t->cfg.key_lo, t->cfg.key_bits, tile_mode ? t->part_mt : t->part_hist,
                         t->part_S, tile_mode ? t->part_mx : nullptr, skip_pad ? 1 : 0, s);
  dev::TileRuns tr{t->kb, t->ia, t->part_mt, t->part_mx, tile_mode ? (uint32_t)tiles : 0u};
  if (!tile_mode)
    dev::launch_partition_coarse(t->kb, n, t->gcount, t->ia, t->cfg.key_lo, t->cfg.key_bits,
                                 t->part_hist, t->part_S, t->ka, t->ib, t->bins, s);
  dev::launch_bin_unique(t->ka, t->ib, t->bins, t->cfg.key_lo, t->cfg.key_bits, vals,
                         tile_mode ? t->ic : t->ia,
                         reinterpret_cast<uint64_t*>(t->bins + 2 * dev::kCoarse),
                         tile_mode ? t->kc : t->kb, tile_mode ? t->id : t->ic,
                         op_keys(t, tag), op_vals(t, tag), op_dels(t, tag), op_counts(t, tag),
                         t->d_err, t->part_S, &t->ctl->gate,
                         tag, t->stamps ? t->stamps + dev::kUpperStamps : nullptr, tr,
                         lb_ctr(t, dev::kLbBin), s);
  DBG(s, "ordering");
  note(t->sync.ord, s);
  return SHM_OK;
}

// steps 2-5 on the ordered chunk of tag (the leaf directory is current)
int insert_apply(shm_tree* t, hipStream_t s, uint64_t n, uint32_t tag,
                 shm_tree::ProfRec& pr) {
  const uint64_t lock_tag = (uint64_t)tag << 32;
  const bool upkeep = dir_chunk_begin(t, tag);
  // the byte marks repeat every 255 chunks: clear them when they wrap, so
  // no page still carries this chunk's mark from 255 chunks ago
  if (dev::new_mark(tag) == 1)
    HIP_OK(hipMemsetAsync(t->pnew, 0, t->cap_pages, s));
  // the fan-in words' 32-bit tag (split_wave.h fan_tag: the chunk tag's low
  // 29 bits and the level) repeats every 2^29 chunks: clear the words when it
  // wraps, so a large split never finds the count its segment's word was
  // left with 2^29 chunks ago under the same tag (fan_arrive would count on
  // from it and fan_in pass early or never).  A zero word reads as tag 0
  // with no arrival, which is what the chunk with tag bits 0 starts from
  if ((tag & (seq::kFanPeriod - 1u)) == 0) {
    HIP_OK(hipMemsetAsync(t->leaf_rd, 0, sizeof(uint64_t) * t->sep_cap, s));
    HIP_OK(hipMemsetAsync(t->int_rd, 0, sizeof(uint64_t) * t->sep_cap, s));
  }
  dev::WalkArgs w = arena_args<dev::WalkArgs>(t);
  uint64_t* const cnt = op_counts(t, tag);
  w.keys = op_keys(t, tag);
  w.n = n;
  w.n_dev = cnt + 0;
  w.out_page = t->pages;
  w.target_level = 0;
  w.out_slot = t->oslot;
  w.out_new = t->pnew;  // the page marks the segmentation reads
  w.out_new_tag = tag;
  w.any_new = reinterpret_cast<uint32_t*>(t->d_counts + 10);
  w.vals = op_vals(t, tag);
  w.locks = t->locks;
  w.num_locks = t->cfg.num_locks;
  w.lock_tag = lock_tag;
  dir_view_locate(t, w);
  dev::launch_locate(w, n, s);
  DBG(s, "locate");
  uint32_t* d_ns = reinterpret_cast<uint32_t*>(t->d_counts + 8);
  dev::UpperArgs u = arena_args<dev::UpperArgs>(t);
  u.locks = t->locks;
  u.num_locks = t->cfg.num_locks;
  u.tag = lock_tag;
  u.batch = tag;
  u.par = tag & 1u;
  u.ctl = t->ctl;
  u.op_key = op_keys(t, tag);
  u.op_val = op_vals(t, tag);
  u.seg_start = t->seg_start;
  u.seg_end = t->seg_end;
  u.seg_page = t->seg_page;
  u.seg_T = t->seg_T;
  u.seg_P = t->seg_P;
  u.seg_np = t->seg_np;
  u.seg_ver = t->seg_ver;
  u.ns_dev = d_ns;
  u.leaf_rd = t->leaf_rd;
  u.sep_cap = t->sep_cap;
  for (int i = 0; i < 2; ++i) {
    u.sep_key[i] = t->sep_key[i];
    u.sep_ptr[i] = t->sep_ptr[i];
    u.ipage[i] = t->ipage[i];
  }
  u.h_end = t->h_end;
  u.h_T = t->h_T;
  u.h_P = t->h_P;
  u.h_ver = t->h_ver;
  u.h_lk = t->h_lk;
  u.d_head = t->d_head;
  u.d_base = t->d_base;
  u.int_rd = t->int_rd;
  u.pub = pub_words_dev(t);
  u.dk = op_dels(t, tag);
  u.n_del = cnt + 1;
  if (const int rc = dir_chunk_args(t, s, upkeep, u)) return rc;
  u.stamps = t->stamps;
  u.force_abort = (t->force_flags & 1u) ? 1u : 0u;
  u.no_direct = (t->force_flags & 2u) ? 1u : 0u;
  u.prof = t->prof.on ? t->prof.ins : nullptr;
  // small splits built by the upsert kernel itself; the forced k_upper paths
  // (force flags 1, 2, 4) leave them all to k_upper
  dev::UpperArgs ue = u;
  ue.early = (t->force_flags & 7u) ? 0u : 1u;
  // a chunk with no new key and no delete is completed by the segmentation
  // kernel's block 0 (u: k_upper's quick path; k_upper then returns at once).
  const bool quick_ok = !u.force_abort;
  // force flag bit 3: every tile counts its predecessors itself (the
  // look-back's fallback, exercised by a test)
  dev::launch_segment(t->pages, n, cnt + 0, t->seg_lb, t->seg_start, t->seg_end,
                      t->seg_page, d_ns, t->pnew, tag, w.any_new, t->d_err, s,
                      quick_ok ? &u : nullptr, lb_ctr(t, dev::kLbSeg),
                      (t->force_flags & 8u) ? 0u : kSegSelfAfter, cnt + 1,
                      &t->ctl->ndel[tag & 1u][0]);
  DBG(s, "segment");
  if (t->prof.on) HIP_OK(hipEventRecord(pr.e[1], s));
  dev::SegArgs a = arena_args<dev::SegArgs>(t);
  a.op_key = op_keys(t, tag);
  a.op_val = op_vals(t, tag);
  a.seg_start = t->seg_start;
  a.seg_end = t->seg_end;
  a.seg_page = t->seg_page;
  a.num_seg = (uint32_t)n;
  a.num_seg_dev = d_ns;
  a.seg_T = t->seg_T;
  a.seg_P = t->seg_P;
  a.seg_newpages = t->seg_np;
  a.seg_ver = t->seg_ver;
  a.oslot = t->oslot;
  a.placed = u.dir_w ? t->oslot : nullptr;  // new keys' slots for k_dir_upkeep
  a.locks = t->locks;
  a.num_locks = t->cfg.num_locks;
  a.tag = lock_tag;
  a.ctl = t->ctl;
  a.par = tag & 1u;
  a.up_nb = dev::upper_blocks();
  dev::launch_leaf_upsert(a, ue, s);
  DBG(s, "leaf_upsert");
  if (t->prof.on) HIP_OK(hipEventRecord(pr.e[2], s));
  t->force_flags = 0;
  dev::launch_upper(u, s);
  DBG(s, "upper");
  if (const int rc = dir_chunk_upkeep(t, s, u, n, tag)) return rc;
  HIP_OK(hipGetLastError());
  t->err_pending = true;
  if (t->prof.on) {
    HIP_OK(hipEventRecord(pr.e[3], s));
    t->prof.pending.push_back(pr);
  }
  return SHM_OK;
}

// The end of the chunk counter's epoch (seq_epoch.h kLastTag = 2^32 - 1): the
// next chunk is tag 1 of a new epoch.  Every device word that is compared
// with a chunk tag would otherwise meet values of the old epoch: lock words
// stay above every small tag (never free: kErrLock after kMaxLockSpins), and
// gate, skip, the segmentation's tile words, the ordering's look-back words
// and the fan-in words could equal a new tag again.  So the handle is drained
// and all of them are zeroed, as shm_tree_create leaves them, the page marks
// with them; the counter restarts at 0 (the caller increments it to 1: tag 0
// is never issued) and the mirrors follow: the superblock's batch count, the
// host words (published tag, applied tag) and the flow control of
// insert_order (app_valid), whose `<` wait would otherwise hold a small tag
// against a large applied word of the old epoch and let it pass early.
int epoch_reset(shm_tree* t) {
  HIP_OK(hipDeviceSynchronize());
  mirror(t);  // exact: the device is idle
  hipStream_t s = t->stream;
  HIP_OK(hipMemsetAsync(t->locks, 0, sizeof(uint64_t) * t->cfg.num_locks, s));
  HIP_OK(hipMemsetAsync(t->ctl, 0, sizeof(dev::UpperCtl), s));
  HIP_OK(hipMemsetAsync(t->seg_lb, 0, sizeof(uint64_t) * (dev::seg_tiles(t->sep_cap) + 1), s));
  HIP_OK(hipMemsetAsync(t->bins, 0, sizeof(uint32_t) * 4 * dev::kCoarse, s));
  HIP_OK(hipMemsetAsync(t->leaf_rd, 0, sizeof(uint64_t) * t->sep_cap, s));
  HIP_OK(hipMemsetAsync(t->int_rd, 0, sizeof(uint64_t) * t->sep_cap, s));
  HIP_OK(hipMemsetAsync(t->pnew, 0, t->cap_pages, s));
  // k_locate's "a page was marked" word (d_counts + 10) holds a chunk tag too
  HIP_OK(hipMemsetAsync(t->d_counts, 0, sizeof(uint64_t) * 32, s));
  t->chunks = 0;
  for (int p = 0; p < 2; ++p) {
    t->sync.app_valid[p] = false;
    t->sync.app_tag[p] = 0;
  }
  pub_words(t)[dev::kPubApplied] = 0;
  if (write_superblock(t, s)) return SHM_EIO;  // batches = 0, and the host words (publish_host)
  t->pub_batch = 0;
  dir_tag_reset(t, 0);
  HIP_OK(hipStreamSynchronize(s));
  return SHM_OK;
}

// the chunk's ordering (step 1): its tag, profile record started
int insert_begin(shm_tree* t, hipStream_t s, const uint64_t* keys, const uint64_t* vals,
                 uint64_t n, bool skip_pad, uint32_t* tag, shm_tree::ProfRec& pr) {
  if (seq::epoch_ends(t->chunks)) {
    // a chunk ordered in the old epoch is applied under its old tag first
    if (t->sync.n_pend) return SHM_EAGAIN;
    if (const int rc = epoch_reset(t)) return rc;
  }
  *tag = ++t->chunks;
  if (t->prof.on) {
    const int rc = prof_begin(t, s, shm_tree::kProfInsert, n, 4, pr);
    if (rc) return rc;
  }
  return insert_order(t, s, keys, vals, n, *tag, skip_pad);
}

// steps 2-5 once the device state may change (the leaf directory current)
int insert_finish(shm_tree* t, hipStream_t s, uint64_t n, uint32_t tag, shm_tree::ProfRec& pr) {
  // every insert chunk passes here (shm_insert_batch and _async, shm_del_batch
  // through them, shm_insert_apply, shm_mixed_batch, the padded hook): the
  // order index is of the tree before it, whatever the chunk's status
  ++t->ord_gen;
  if (use_leaf_dir(t)) {
    const int rc = refresh_dir(t, s);
    if (rc) return rc;
  }
  const int rc = insert_apply(t, s, n, tag, pr);
  if (rc != SHM_OK) return rc;
  // k_upper was queued: it publishes the tag once done with the op buffers
  const uint32_t p = tag & 1u;
  t->sync.app_tag[p] = tag;
  t->sync.app_valid[p] = true;
  note(t->sync.app_m[p], s);
  return SHM_OK;
}

int insert_chunk(shm_tree* t, hipStream_t s, const uint64_t* keys, const uint64_t* vals,
                 uint64_t n, bool skip_pad) {
  uint32_t tag = 0;
  shm_tree::ProfRec pr{};
  if (const int rc = insert_begin(t, s, keys, vals, n, skip_pad, &tag, pr)) return rc;
  return insert_finish(t, s, n, tag, pr);
}

// every chunk of one insert call, in order.  A chunk holding kKeyMax is
// rejected whole on the device (SHM_EINVAL at the next synchronising call);
// the call's other chunks, before and after it, are applied (the host does
// not wait between chunks).  skip_pad: kKeyMax keys are a routed insert's
// slot padding and are skipped (shm__insert_batch_padded).
int insert_all(shm_tree* t, const uint64_t* keys, const uint64_t* vals, uint64_t n, void* stream,
               bool sync, bool skip_pad = false) {
  if (!t || (n && (!keys || !vals))) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  if (t->sync.n_pend) return SHM_EINVAL;  // chunks ordered by shm_insert_order come first
  hipStream_t s = pick(stream);
  // The first chunk's ordering reads only the batch and writes the insert
  // workspace, so it is queued before this call's cross-stream wait: it
  // waits for the workspace's last users (insert_order) but not for, e.g.,
  // the range scans just issued on another stream, and runs beside them.
  // (An ordered search's workspace aliases the insert workspace: not with
  // SHM_FLAG_SORT_GETS.)
  const bool early = n > 0 && !(t->cfg.flags & SHM_FLAG_SORT_GETS);
  uint32_t tag0 = 0;
  shm_tree::ProfRec pr0{};
  const uint64_t m0 = std::min(t->nmax, n);
  if (early) {
    if (const int rc = insert_begin(t, s, keys, vals, m0, skip_pad, &tag0, pr0)) return rc;
  }
  Order ord(t, s, true);
  if (ord.rc) return ord.rc;
  mirror(t);
  int rc = SHM_OK;
  for (uint64_t off = 0; off < n && rc == SHM_OK; off += t->nmax) {
    const uint64_t m = std::min(t->nmax, n - off);
    rc = off == 0 && early ? insert_finish(t, s, m0, tag0, pr0)
                           : insert_chunk(t, s, keys + off, vals + off, m, skip_pad);
  }
  if (rc == SHM_OK) {
    t->batches += 1;
    if (sync) rc = check_err(t, s);
  }
  return rc;
}
}  // namespace host
}  // namespace shm

extern "C" {

int shm_insert_batch(shm_tree* t, const uint64_t* keys, const uint64_t* vals,
                     uint64_t n, void* stream) {
  return insert_all(t, keys, vals, n, stream, true);
}

int shm_insert_batch_async(shm_tree* t, const uint64_t* keys, const uint64_t* vals,
                           uint64_t n, void* stream) {
  return insert_all(t, keys, vals, n, stream, false);
}

// Split insert (one chunk): the ordering on one stream, the tree phase
// later on another, so a caller can order chunk i + 1 while chunk i applies.
int shm_insert_order(shm_tree* t, const uint64_t* keys, const uint64_t* vals, uint64_t n,
                     void* stream, uint32_t* ticket) {
  if (!t || !ticket || (n && (!keys || !vals))) return SHM_EINVAL;
  if (n > t->nmax) return SHM_E2BIG;
  if (n == 0) {
    // An empty chunk takes no chunk id and queues nothing: ticket 0 (never a
    // chunk id), which shm_insert_apply accepts as done.  The ordering of 0
    // ops has no tile and no coarse pass, so k_bin_unique would read the bin
    // table the last coarse pass left, with no values behind it.
    *ticket = 0;
    return SHM_OK;
  }
  std::lock_guard<std::mutex> g(t->mu);
  if (t->sync.n_pend >= 2) return SHM_EAGAIN;  // two op-buffer parities
  hipStream_t s = pick(stream);
  // The ordering reads only the batch and writes the insert workspace, whose
  // users it waits for itself (insert_order: ord_ev, app_ev), so it takes no
  // part in the tree's call ordering: it neither waits for the calls before
  // it nor makes the next tree change wait for it (the apply waits for its
  // own ticket only) -- chunk i + 1 is ordered beside chunk i's tree phase.
  // With SHM_FLAG_SORT_GETS an ordered search shares the ordering scratch:
  // the ordering is then ordered like an exclusive call.
  const bool sorted = (t->cfg.flags & SHM_FLAG_SORT_GETS) != 0;
  std::optional<Order> ord;
  if (sorted) {
    ord.emplace(t, s, true);
    if (ord->rc) return ord->rc;
  }
  shm_tree::Pending& pd = t->sync.pend[t->sync.n_pend];
  pd.pr = shm_tree::ProfRec{};
  if (const int rc = insert_begin(t, s, keys, vals, n, false, &pd.tag, pd.pr)) return rc;
  pd.n = n;
  pd.s = s;
  if (!pd.ev) pd.ev = new_event();
  if (!pd.ev) return SHM_EIO;
  HIP_OK(hipEventRecord(pd.ev, s));
  ++t->sync.n_pend;
  *ticket = pd.tag;
  return SHM_OK;
}

int shm_insert_apply(shm_tree* t, uint32_t ticket, void* stream) {
  if (!t) return SHM_EINVAL;
  if (ticket == 0) return SHM_OK;  // an empty chunk (shm_insert_order, n == 0)
  std::lock_guard<std::mutex> g(t->mu);
  if (!t->sync.n_pend || t->sync.pend[0].tag != ticket) return SHM_EINVAL;  // oldest first
  const shm_tree::Pending pd = t->sync.pend[0];
  hipStream_t s = pick(stream);
  Order ord(t, s, true);
  if (ord.rc) return ord.rc;
  if (pd.s != s) HIP_OK(hipStreamWaitEvent(s, pd.ev, 0));
  // the slot is free once its apply is queued (the buffers' reuse waits on
  // the host for this chunk's kPubApplied tag in the mirror, with an event
  // at the apply stream's tail as the fallback: insert_order)
  std::swap(t->sync.pend[0], t->sync.pend[1]);
  --t->sync.n_pend;
  mirror(t);
  shm_tree::ProfRec pr = pd.pr;
  if (t->prof.on) {
    // the profile times the apply alone (the ordering ran earlier, elsewhere)
    if (!pr.e[0]) {
      if (const int rc = prof_begin(t, s, shm_tree::kProfInsert, pd.n, 4, pr)) return rc;
    } else {
      HIP_OK(hipEventRecord(pr.e[0], s));
    }
  }
  const int rc = insert_finish(t, s, pd.n, pd.tag, pr);
  if (rc == SHM_OK) t->batches += 1;
  return rc;
}

int shm_del_batch(shm_tree* t, const uint64_t* keys, uint64_t n, void* stream) {
  if (!t || (n && !keys)) return SHM_EINVAL;
  if (n == 0) return SHM_OK;
  // deletes are upserts of kValueNull (Tree.cpp:1040-1043)
  uint64_t* zeros = nullptr;
  const uint64_t m = std::min<uint64_t>(n, t->nmax);
  if (hipMalloc((void**)&zeros, m * sizeof(uint64_t)) != hipSuccess) return SHM_ENOMEM;
  hipStream_t s = pick(stream);
  int rc = SHM_OK;
  if (hipMemsetAsync(zeros, 0, m * sizeof(uint64_t), s) != hipSuccess) rc = SHM_EIO;
  for (uint64_t off = 0; off < n && rc == SHM_OK; off += m) {
    rc = shm_insert_batch(t, keys + off, zeros, std::min(m, n - off), stream);
  }
  (void)hipStreamSynchronize(s);
  (void)hipFree(zeros);
  return rc;
}

// Library-internal, not part of include/sherman_amd.h (shard.cpp): a routed
// insert's received slots, kKeyMax padding skipped, queued as
// shm_insert_batch_async (n <= max_batch: one chunk)
int shm__insert_batch_padded(shm_tree* t, const uint64_t* keys, const uint64_t* vals, uint64_t n,
                             void* stream) {
  if (t && n > t->nmax) return SHM_E2BIG;
  return insert_all(t, keys, vals, n, stream, false, true);
}

// Diagnostics, not part of include/sherman_amd.h: flags for the next insert
// chunk's k_upper.  Bit 0: every block gives up at its first phase hand-off
// (as a timed-out wait would; the launch's last block then completes the
// chunk alone); bit 1: the chunk propagates its splits through the level
// lists instead of the direct path; bit 2 (or any bit): the chunk's upsert
// kernel leaves every split to k_upper (no early splits).
int shm__upper_force(shm_tree* t, uint32_t flags) {
  if (!t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  t->force_flags = flags;
  return SHM_OK;
}
int shm__upper_force_abort(shm_tree* t) { return shm__upper_force(t, 1u); }

// Test hook, not part of include/sherman_amd.h: move a counter forward as if
// value - current chunks (which = 0) or scans (which = 1) without effect had
// run -- chunks that only overwrite stored keys with the values they hold (no
// new key, no delete, none rejected, directory not kept), scans of one tile.
// Waits for the tree first.  SHM_EINVAL while ordered chunks are pending or
// when value is below the counter; value == counter changes nothing.
//
// which = 0, the chunk counter (C = the counter, V = value).  Set on the host:
//   t->chunks = V                   the counter (shm_last_chunk)
//   host word 0 (publish_host)      the published tag; pub_batch, pub_seen = V
//                                   (only compared with each other: no quiet-
//                                   rule look is pending)
//   host word kPubApplied = V       the last skipped chunk is done with its op
//                                   buffers; app_valid = false says the same
//                                   to insert_order (nothing to wait for)
//   dir_last_upkept = false         no skipped chunk kept the directory: the
//                                   next kept chunk zeroes its parity's
//                                   repair list count itself
// The host clears the skipped chunks' insert_apply would have made:
//   pnew            when a multiple of 255 lies in (C, V] (the marks' period);
//                   the chunks after it bring no new key and mark nothing
//   leaf_rd, int_rd when a multiple of 2^29 lies in (C, V] (the fan tags')
// Device words the skipped chunks would have rewritten, written here:
//   superblock.batches = V          every chunk's completion stores it (the
//                                   whole superblock is rewritten from the
//                                   exact mirror: no other field changes)
//   UpperCtl tk, dn, abort, leaf_np, leaf_ns, leaf_nb, alloc, made, root_new,
//   lvl_sep, done, ualloc, late     both parities zero: chunk C + 1 zeroes
//                                   parity C & 1 (upper_zero_next) and no
//                                   skipped chunk counts a split, so the next
//                                   chunk finds its parity clean whether
//                                   V - C is odd or even
//   UpperCtl skip[V & 1] = V, skip[(V - 1) & 1] = V - 1 (if V - C >= 2), and
//   ndel of those parities = 0      the segmentation completes such chunks
//                                   (seg_complete_unchanged)
//   the ordering's 256 look-back words = (V & 0xFFFF) << 48
//                                   every k_bin_unique launch that is not
//                                   rejected publishes all of them (isort.hip
//                                   bin_prefix, called on both paths of every
//                                   block); only the tag is compared later,
//                                   so the counts are written as 0
// Left as they are: gate (no skipped chunk is rejected), the lock words (a
// skipped chunk would leave the words it took at its tag << 32, which is
// free for every later tag exactly as the older value is), the
// segmentation's tile words (a skipped chunk writes (tag << 32 | 0) into the
// words of its own tiles only; an older tag matches a later chunk no more
// than a skipped one would), the op buffers and the ordering's scratch
// (rewritten by every ordering before they are read).
//
// which = 1, scan_seq: set to V, or V + 1 when V is a multiple of 2^16
// (scan_tag steps over those); bsum64 is cleared when a multiple of 2^16
// lies in (C, V], as scan_tag clears it.  A skipped scan of one tile reads
// no tile word and leaves its own word 0 tagged: not written here, its tag
// is older than any the next 65534 scans use.
int shm__seq_jump(shm_tree* t, int which, uint32_t value) {
  if (!t || (which != 0 && which != 1)) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  HIP_OK(hipDeviceSynchronize());
  mirror(t);  // exact: the device is idle
  if (which == 1) {
    if (value < t->scan_seq) return SHM_EINVAL;
    const seq::ScanJump j = seq::scan_jump(t->scan_seq, value);
    if (j.clear)
      HIP_OK(hipMemset(t->bsum64, 0, sizeof(uint64_t) * (dev::seg_tiles(t->nmax) + 1)));
    t->scan_seq = j.seq;
    return SHM_OK;
  }
  if (t->sync.n_pend || value < t->chunks) return SHM_EINVAL;
  const uint32_t cur = t->chunks;
  if (value == cur) return SHM_OK;
  const seq::ChunkJump j = seq::chunk_jump(cur, value);
  if (j.marks) HIP_OK(hipMemset(t->pnew, 0, t->cap_pages));
  if (j.fan) {
    HIP_OK(hipMemset(t->leaf_rd, 0, sizeof(uint64_t) * t->sep_cap));
    HIP_OK(hipMemset(t->int_rd, 0, sizeof(uint64_t) * t->sep_cap));
  }
  uint8_t* const ctl = reinterpret_cast<uint8_t*>(t->ctl);
  HIP_OK(hipMemset(ctl, 0, offsetof(dev::UpperCtl, gate)));
  HIP_OK(hipMemset(ctl + offsetof(dev::UpperCtl, leaf_np), 0,
                   offsetof(dev::UpperCtl, skip) - offsetof(dev::UpperCtl, leaf_np)));
  for (uint32_t k = 0; k < 2 && value - k > cur; ++k) {
    const uint32_t v = value - k;
    const uint64_t sk = v, nd = 0;
    HIP_OK(hipMemcpy(&t->ctl->skip[v & 1u][0], &sk, sizeof(sk), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(&t->ctl->ndel[v & 1u][0], &nd, sizeof(nd), hipMemcpyHostToDevice));
  }
  {
    std::vector<uint64_t> w((size_t)dev::kCoarse, (uint64_t)(value & 0xFFFFu) << 48);
    HIP_OK(hipMemcpy(reinterpret_cast<uint64_t*>(t->bins + 2 * dev::kCoarse), w.data(),
                     sizeof(uint64_t) * w.size(), hipMemcpyHostToDevice));
  }
  t->chunks = value;
  for (int p = 0; p < 2; ++p) t->sync.app_valid[p] = false;
  pub_words(t)[dev::kPubApplied] = value;
  if (write_superblock(t, t->stream)) return SHM_EIO;  // batches = V; publish_host: word 0 = V
  t->pub_batch = value;
  dir_tag_reset(t, value);
  HIP_OK(hipStreamSynchronize(t->stream));
  return SHM_OK;
}

// Diagnostics: the pages the last insert chunk's early splits took (its
// upsert kernel's, upsert.hip), after synchronising the tree
int shm__early_pages(shm_tree* t, uint64_t* out) {
  if (!t || !out) return SHM_EINVAL;
  const int rc = shm_synchronize(t);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(t->mu);
  HIP_OK(hipMemcpy(out, &t->ctl->ualloc[t->chunks & 1u][0], sizeof(uint64_t),
                   hipMemcpyDeviceToHost));
  return SHM_OK;
}

// Test hook, not part of include/sherman_amd.h: the ordered chunk of an
// outstanding shm_insert_order ticket, as its apply will read it.  Waits for
// the ticket's ordering; counts_host[0..1] = {upserts, deletes}, then
// uk_host / uv_host [0, upserts) and dk_host [0, deletes) (host buffers of the
// chunk's n words each).  Changes no state: the ticket stays outstanding.
// SHM_EINVAL for any ticket that is not outstanding.
int shm__order_read(shm_tree* t, uint32_t ticket, uint64_t* uk_host, uint64_t* uv_host,
                    uint64_t* dk_host, uint64_t* counts_host) {
  if (!t || !uk_host || !uv_host || !dk_host || !counts_host) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  const shm_tree::Pending* pd = nullptr;
  for (int i = 0; i < t->sync.n_pend; ++i)
    if (t->sync.pend[i].tag == ticket) pd = &t->sync.pend[i];
  if (!pd) return SHM_EINVAL;
  HIP_OK(hipEventSynchronize(pd->ev));
  HIP_OK(hipMemcpy(counts_host, op_counts(t, ticket), 2 * sizeof(uint64_t),
                   hipMemcpyDeviceToHost));
  const uint64_t nu = counts_host[0], nd = counts_host[1];
  if (nu > pd->n || nd > pd->n) return SHM_EIO;  // the buffers hold n words
  if (nu) {
    HIP_OK(hipMemcpy(uk_host, op_keys(t, ticket), nu * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(uv_host, op_vals(t, ticket), nu * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  if (nd)
    HIP_OK(hipMemcpy(dk_host, op_dels(t, ticket), nd * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SHM_OK;
}

// Test hook, not part of include/sherman_amd.h: the compiled constants that
// decide the path an ordering takes (isort.hip order_limits): out[0..5] =
// kIsortTile, kMaxTiles, kUniqCap, kSubRankCap, kCoarse, kFine
int shm__order_limits(uint64_t* out) {
  if (!out) return SHM_EINVAL;
  dev::order_limits(out);
  return SHM_OK;
}

// Diagnostics, not part of include/sherman_amd.h: enable = 1 turns k_upper's
// phase clock on, 0 off; out (nullable, kUpperStamps words) receives the last
// chunk's stamps (out[0] = count, then 100 MHz wall-clock values).
int shm__upper_stamps(shm_tree* t, int enable, uint64_t* out) {
  if (!t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  if (enable == 1 && !t->stamps) {
    if (hipMalloc(&t->stamps, sizeof(uint64_t) * dev::kStampWords) != hipSuccess)
      return SHM_ENOMEM;
    HIP_OK(hipMemset(t->stamps, 0, sizeof(uint64_t) * dev::kStampWords));
  }
  if (out && t->stamps) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, t->stamps, sizeof(uint64_t) * dev::kStampWords,
                     hipMemcpyDeviceToHost));
  }
  if (enable == 0 && t->stamps) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipFree(t->stamps));
    t->stamps = nullptr;
  }
  return SHM_OK;
}
}  // extern "C"
