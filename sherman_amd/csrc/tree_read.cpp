// tree_read.cpp — the calls that read the tree: batched gets, range queries
// and limited scans.
//
// A get is a shared call (Order): it may run beside other gets on other
// streams, and turns exclusive only to rebuild the directory or the top
// replica (tree_dir.cpp decides when).  Range queries and scans refresh the
// directory first and are exclusive, for their workspaces.  shm_mixed_batch is
// here whole: its gets and its insert chunks run under one lock and one Order.
#include "tree_internal.h"

namespace shm {
namespace host __attribute__((visibility("hidden"))) {

constexpr uint64_t kSortMinGets = 8192;   // below this, walk in input order
constexpr uint32_t kRangeStage = 160;      // staged values per range scan
constexpr uint64_t kRangeStageBytes = 256ull << 20;  // staging budget

dev::RangeArgs range_args(shm_tree* t, const uint64_t* from, const uint64_t* to, uint64_t n,
                          uint64_t* counts, const uint64_t* offsets, uint64_t* vals) {
  dev::RangeArgs a = arena_args<dev::RangeArgs>(t);
  a.from = from;
  a.to = to;
  a.n = n;
  a.counts = counts;
  a.offsets = offsets;
  a.vals = vals;
  a.vals_cap = ~0ull;
  dir_view(t, a);
  return a;
}

// a fresh tag for launch_scan_u64_total's tile words (16 bits: the words
// are zeroed again when the tag wraps, so no stale word can match)
uint32_t scan_tag(shm_tree* t, hipStream_t s) {
  uint32_t tag = ++t->scan_seq & 0xFFFFu;
  if (tag == 0) {
    (void)hipMemsetAsync(t->bsum64, 0, sizeof(uint64_t) * (dev::seg_tiles(t->nmax) + 1), s);
    tag = ++t->scan_seq & 0xFFFFu;
  }
  return tag;
}

// one timed k_range launch
int range_launch(shm_tree* t, hipStream_t s, const dev::RangeArgs& a) {
  return timed_launch(t, s, a.n, [&] { dev::launch_range(a, s); });
}

// one-chunk batches whose staging fits kRangeStageBytes keep up to
// kRangeStage values per scan from the count pass for the fill pass
int range_stage(shm_tree* t, hipStream_t s, uint64_t n, bool* staged) {
  *staged = n <= t->nmax && n * kRangeStage * 8 <= kRangeStageBytes;
  if (*staged && t->rstage_words < n * kRangeStage) {
    if (t->rstage) {
      HIP_OK(hipStreamSynchronize(s));
      HIP_OK(hipFree(t->rstage));
      t->rstage = nullptr;
      t->rstage_words = 0;
    }
    // headroom: batches of similar size must not each reallocate (a
    // reallocation waits for the stream)
    const uint64_t words = std::max<uint64_t>(n + n / 4, 1u << 14) * kRangeStage;
    if (dalloc(&t->rstage, words)) return SHM_ENOMEM;
    t->rstage_words = words;
  }
  return SHM_OK;
}

// range scans read what the directory points at: refresh it first
int range_prepare(shm_tree* t, hipStream_t s) {
  mirror(t);
  if (use_leaf_dir(t)) return refresh_dir(t, s);
  return SHM_OK;
}

// The batched get on s under ord (the leaf directory is current).
int search_impl(shm_tree* t, hipStream_t s, Order& ord, const uint64_t* keys,
                uint64_t n, uint64_t* vals_out, uint8_t* found_out) {
  // Unordered batches take the summary walk (k_get_sum: directory entry,
  // summary line, matching entry: ~3 random lines per get).  Ordering the
  // batch by key first (SHM_FLAG_SORT_GETS) feeds the page walk (k_get),
  // which shares a leaf's 1 KB read among the queries that need it; at C2
  // that is 6.3 G gets/s against 15.4 for the summary walk, so the auto mode
  // no longer orders.
  const bool ordered = (t->cfg.flags & SHM_FLAG_SORT_GETS) && n >= kSortMinGets;
  for (uint64_t off = 0; off < n; off += t->nmax) {
    const uint64_t m = std::min(t->nmax, n - off);
    dev::WalkArgs a = arena_args<dev::WalkArgs>(t);
    a.out_val = vals_out + off;
    a.out_found = found_out ? found_out + off : nullptr;
    a.n = m;
    a.page_check = (t->cfg.flags & SHM_FLAG_PAGE_CHECK) ? 1 : 0;
    dir_view_get(t, a);
    a.stats = t->prof.stats ? t->prof.idx_stats : nullptr;
    bool gathered = false;
    shm_tree::ProfRec pr{};
    if (t->prof.on) {
      if (t->prof.clk_live >= shm_tree::kClkSlots) {  // every clock slot holds a record
        const int rc = drain_profile(t);
        if (rc) return rc;
      }
      const int rc = prof_begin(t, s, shm_tree::kProfGet, m, 3, pr);
      if (rc) return rc;
    }
    if (ordered && m >= kSortMinGets) {
      // order the batch by its top key bits so queries that share pages are
      // walked by the same wave (one page read per group, not per query)
      // (keys1, pos1, walk order keys_out, src); the walk stores result p at
      // vals1[src[p]] (= keys1, inside p's chunk), unpartition gathers
      const shm_tree::GetWs& w = t->sync.gws[ord.ws >= 0 ? ord.ws : ord.take_ws()];
      if (ord.rc) return ord.rc;
      dev::launch_partition(keys + off, m, t->cfg.key_lo, t->cfg.key_bits, w.M, w.S, w.chunks,
                            w.keys1, w.pos1, w.keys_out, w.src, s);
      a.keys = w.keys_out;
      a.perm = w.src;
      a.out_val = w.keys1;
      a.out_found = nullptr;
      a.xcd_remap = 1;
      gathered = true;
      DBG(s, "sort(get)");
    } else {
      // unordered: every wave sorts its own 64 keys and starts at the leaf
      // directory; results land in input order (no unpartition pass)
      a.keys = keys + off;
      a.perm = nullptr;
      a.xcd_remap = 0;
    }
    // leaf DMA policy: an ordered walk reads each leaf once per batch, so
    // non-temporal loads keep the directory in L2 (C2 +5 %)
    a.nt = gathered ? 1 : 0;
    // the walk's profile events: around the page walk's launch; the summary
    // walk's own dispatch carries them (hipExtLaunchKernel: its start and
    // end, the span a kernel trace reports, with no marker packets between)
    if (t->prof.on && gathered) HIP_OK(hipEventRecord(pr.e[1], s));
    // ordered: the page walk (k_get); unordered: the summary walk (k_get_sum,
    // three lines per get)
    if (t->prof.on && !gathered && t->prof.clk) {
      pr.clk = t->prof.clk_next;
      pr.blocks = dev::get_sum_blocks(m);
      t->prof.clk_next = (t->prof.clk_next + 1) % shm_tree::kClkSlots;
      ++t->prof.clk_live;
      a.clk = t->prof.clk + (uint64_t)pr.clk * t->prof.clk_words;
    }
    if (gathered)
      dev::launch_get(a, m, s);
    else
      dev::launch_get_sum(a, m, s, t->prof.on ? pr.e[1] : nullptr, t->prof.on ? pr.e[2] : nullptr);
    DBG(s, "walk(get)");
    if (t->prof.on) {
      if (gathered) HIP_OK(hipEventRecord(pr.e[2], s));
      t->prof.pending.push_back(pr);
    }
    if (gathered) {
      const shm_tree::GetWs& w = t->sync.gws[ord.ws];
      dev::launch_unpartition(w.keys1, w.pos1, m, vals_out + off,
                              found_out ? found_out + off : nullptr, s);
      DBG(s, "gather");
    }
  }
  HIP_OK(hipGetLastError());
  return SHM_OK;
}
}  // namespace host
}  // namespace shm

extern "C" {

int shm_search_batch(shm_tree* t, const uint64_t* keys, uint64_t n,
                     uint64_t* vals_out, uint8_t* found_out, void* stream) {
  if (!t || (n && (!keys || !vals_out))) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  hipStream_t s = pick(stream);
  mirror(t);
  Order ord(t, s, false);
  dir_note_read(t);
  if (use_leaf_dir(t)) {
    dir_note_gets(t, n);
    if (const int rc = vt_poll(t, false)) return rc;
    if (dir_stale(t)) ord.make_exclusive();  // the rebuild rewrites what searches read
    const int rc = ord.rc ? ord.rc : refresh_dir(t, s);
    if (rc) return rc;
  } else if (use_top(t)) {
    if (top_stale(t)) ord.make_exclusive();
    const int rc = ord.rc ? ord.rc : refresh_top(t, s);
    if (rc) return rc;
  }
  return search_impl(t, s, ord, keys, n, vals_out, found_out);
}

int shm_mixed_batch(shm_tree* t, const uint64_t* get_keys, uint64_t n_get, uint64_t* vals_out,
                    uint8_t* found_out, const uint64_t* ins_keys, const uint64_t* ins_vals,
                    uint64_t n_ins, void* stream) {
  if (!t || (n_get && (!get_keys || !vals_out)) || (n_ins && (!ins_keys || !ins_vals)))
    return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  if (t->sync.n_pend && n_ins) return SHM_EINVAL;  // apply the ordered chunks first
  hipStream_t s = pick(stream);
  mirror(t);
  Order ord(t, s, true);
  if (ord.rc) return ord.rc;
  if (use_leaf_dir(t)) {
    dir_note_gets(t, n_get);
    const int rc = refresh_dir(t, s);
    if (rc) return rc;
  }
  // the gets, then the inserts, on s.  (Running the inserts' ordering on a
  // second stream beside the walk was measured: the walk's blocks hold every
  // CU, the ordering kernels ran in its tail anyway and the join cost
  // ~10 us; C3 4125 vs 4160-4188 Mops/s.)
  int rc = search_impl(t, s, ord, get_keys, n_get, vals_out, found_out);
  for (uint64_t off = 0; off < n_ins && rc == SHM_OK; off += t->nmax)
    rc = insert_chunk(t, s, ins_keys + off, ins_vals + off, std::min(t->nmax, n_ins - off));
  if (rc == SHM_OK && n_ins) t->batches += 1;
  return rc;
}

int shm_range_query(shm_tree* t, const uint64_t* from, const uint64_t* to,
                    uint64_t n, uint64_t* counts_out, const uint64_t* offsets,
                    uint64_t* vals_out, void* stream) {
  if (!t || (n && (!from || !to || !counts_out))) return SHM_EINVAL;
  if (offsets && !vals_out) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  hipStream_t s = pick(stream);
  Order ord(t, s, true);  // range workspace (scan temp, staging)
  if (ord.rc) return ord.rc;
  if (const int rc = range_prepare(t, s)) return rc;
  t->err_pending = true;
  return range_launch(t, s, range_args(t, from, to, n, counts_out, offsets, vals_out));
}

int shm_range_query_batch(shm_tree* t, const uint64_t* from, const uint64_t* to, uint64_t n,
                          uint64_t* counts_out, uint64_t* offsets_out, uint64_t* vals_out,
                          uint64_t vals_cap, uint64_t* total_out, void* stream) {
  if (!t || !total_out || (n && (!from || !to || !counts_out || !offsets_out))) return SHM_EINVAL;
  if (vals_cap && !vals_out) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  hipStream_t s = pick(stream);
  Order ord(t, s, true);  // range workspace (scan temp, staging)
  if (ord.rc) return ord.rc;
  *total_out = 0;
  if (n == 0) return SHM_OK;
  if (const int rc = range_prepare(t, s)) return rc;
  // pass 1 per chunk (the scan workspace holds nmax): counts, exclusive scan,
  // chunk total and error word back in one read.  A single chunk whose
  // staging fits kRangeStageBytes keeps its values for pass 2.
  uint64_t total = 0;
  std::vector<uint64_t> base;
  bool staged = false;
  if (const int rc = range_stage(t, s, n, &staged)) return rc;
  auto rargs = [&](uint64_t off, uint64_t m, const uint64_t* offs, uint64_t* vals) {
    dev::RangeArgs a = range_args(t, from + off, to + off, m, counts_out + off, offs, vals);
    if (staged) {
      a.stage = t->rstage;
      a.stage_cap = kRangeStage;
    }
    return a;
  };
  for (uint64_t off = 0; off < n; off += t->nmax) {
    const uint64_t m = std::min(t->nmax, n - off);
    int rc = range_launch(t, s, rargs(off, m, nullptr, nullptr));
    if (rc) return rc;
    dev::launch_scan_u64_total(counts_out + off, offsets_out + off, m, t->bsum64,
                               scan_tag(t, s), t->d_err, t->d_counts + 12, t->d_err,
                               lb_ctr(t, dev::kLbScan), s);
    rc = readback(t, s, t->d_counts + 12, 2 * sizeof(uint64_t));
    if (rc) return rc;
    if (t->h_pin[1]) return check_err(t, s);
    base.push_back(total);
    total += t->h_pin[0];
  }
  *total_out = total;
  // offsets are chunk-relative until shifted by the totals before them
  for (size_t c = 1; c < base.size(); ++c) {
    const uint64_t off = c * t->nmax;
    dev::launch_add_u64(offsets_out + off, std::min(t->nmax, n - off), base[c], s);
  }
  if (total > vals_cap) return SHM_ENOSPC;  // counts / offsets stay valid
  // pass 2: values
  for (uint64_t off = 0, c = 0; off < n; off += t->nmax, ++c) {
    const uint64_t m = std::min(t->nmax, n - off);
    const int rc = range_launch(t, s, rargs(off, m, offsets_out + off, vals_out));
    if (rc) return rc;
  }
  t->err_pending = true;
  return SHM_OK;
}

int shm_range_query_batch_async(shm_tree* t, const uint64_t* from, const uint64_t* to,
                                uint64_t n, uint64_t* counts_out, uint64_t* offsets_out,
                                uint64_t* vals_out, uint64_t vals_cap, uint64_t* total_dev,
                                void* stream) {
  if (!t || !total_dev || (n && (!from || !to || !counts_out || !offsets_out)))
    return SHM_EINVAL;
  if (vals_cap && !vals_out) return SHM_EINVAL;
  if (n > t->nmax) return SHM_EINVAL;  // one chunk: offsets need no host-side base
  std::lock_guard<std::mutex> g(t->mu);
  hipStream_t s = pick(stream);
  Order ord(t, s, true);
  if (ord.rc) return ord.rc;
  if (n == 0) {
    HIP_OK(hipMemsetAsync(total_dev, 0, 2 * sizeof(uint64_t), s));
    return SHM_OK;
  }
  if (const int rc = range_prepare(t, s)) return rc;
  bool staged = false;
  if (const int rc = range_stage(t, s, n, &staged)) return rc;
  dev::RangeArgs a = range_args(t, from, to, n, counts_out, nullptr, nullptr);
  if (staged) {
    a.stage = t->rstage;
    a.stage_cap = kRangeStage;
  }
  t->err_pending = true;
  int rc = range_launch(t, s, a);
  if (rc) return rc;
  // count pass -> offsets and (total, error word) into total_dev, then the
  // fill pass bounded by vals_cap; no host synchronisation
  dev::launch_scan_u64_total(counts_out, offsets_out, n, t->bsum64, scan_tag(t, s), t->d_err,
                             total_dev, t->d_err, lb_ctr(t, dev::kLbScan), s);
  if (!vals_cap) return SHM_OK;
  a.offsets = offsets_out;
  a.vals = vals_out;
  a.vals_cap = vals_cap;
  return range_launch(t, s, a);
}

// one pass: the count walk with the caller's per-scan buffers as its staging
int shm_range_query_slots(shm_tree* t, const uint64_t* from, const uint64_t* to, uint64_t n,
                          uint64_t slot_cap, uint64_t* counts_out, uint64_t* vals_out,
                          uint64_t* status_dev, void* stream) {
  if (!t || (n && (!from || !to || !counts_out)) || slot_cap >= (1ull << 32))
    return SHM_EINVAL;
  if (slot_cap && n && !vals_out) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  hipStream_t s = pick(stream);
  Order ord(t, s, true);  // the directory refresh
  if (ord.rc) return ord.rc;
  if (n == 0) return SHM_OK;
  if (const int rc = range_prepare(t, s)) return rc;
  dev::RangeArgs a = range_args(t, from, to, n, counts_out, nullptr, nullptr);
  a.stage = slot_cap ? vals_out : nullptr;
  a.stage_cap = (uint32_t)slot_cap;
  a.status = status_dev;
  t->err_pending = true;
  return range_launch(t, s, a);
}

namespace {
// shm_scan_batch and shm_rscan_batch: one argument check, one queueing, the
// kernel by direction (static: inside extern "C" an unnamed namespace alone
// leaves the name exported)
static int scan_call(shm_tree* t, const uint64_t* from, const uint64_t* to, uint64_t n,
                     uint64_t limit, uint64_t* keys_out, uint64_t* vals_out, uint64_t* counts_out,
                     uint64_t* status_dev, void* stream, bool descending) {
  // the arguments first: a rejected call uses neither the handle nor the GPU
  if (limit == 0 || limit >= (1ull << 31)) return SHM_EINVAL;
  if (n && (!from || !keys_out || !vals_out || !counts_out)) return SHM_EINVAL;
  if (!t) return SHM_EINVAL;
  if (n == 0) return SHM_OK;
  std::lock_guard<std::mutex> g(t->mu);
  hipStream_t s = pick(stream);
  Order ord(t, s, true);  // the directory refresh
  if (ord.rc) return ord.rc;
  if (const int rc = range_prepare(t, s)) return rc;
  dev::ScanArgs a = arena_args<dev::ScanArgs>(t);
  a.from = from;
  a.to = to;
  a.n = n;
  a.limit = (uint32_t)limit;
  a.keys = keys_out;
  a.vals = vals_out;
  a.counts = counts_out;
  dir_view(t, a);
  a.status = status_dev;
  t->err_pending = true;
  return timed_launch(t, s, n, [&] {
    if (descending)
      dev::launch_rscan(a, s);
    else
      dev::launch_scan(a, s);
  });
}
}  // namespace

int shm_scan_batch(shm_tree* t, const uint64_t* from, const uint64_t* to, uint64_t n,
                   uint64_t limit, uint64_t* keys_out, uint64_t* vals_out, uint64_t* counts_out,
                   uint64_t* status_dev, void* stream) {
  return scan_call(t, from, to, n, limit, keys_out, vals_out, counts_out, status_dev, stream,
                   false);
}

int shm_rscan_batch(shm_tree* t, const uint64_t* from, const uint64_t* to, uint64_t n,
                    uint64_t limit, uint64_t* keys_out, uint64_t* vals_out, uint64_t* counts_out,
                    uint64_t* status_dev, void* stream) {
  return scan_call(t, from, to, n, limit, keys_out, vals_out, counts_out, status_dev, stream,
                   true);
}

// Library-internal (shard.cpp): exclusive scan of n <= max_batch u64 words
// on `stream`; tot_dev (device, 2 words) = {total, the tree's error word}
int shm__scan_u64(shm_tree* t, const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* tot_dev,
                  void* stream) {
  if (!t || !tot_dev || (n && (!in || !out))) return SHM_EINVAL;
  if (n > t->nmax) return SHM_E2BIG;
  std::lock_guard<std::mutex> g(t->mu);
  hipStream_t s = pick(stream);
  // the tile words and the look-back counter are the tree's: no other scan
  // of the tree (shm_range_query_*) may run beside this one
  Order ord(t, s, true);
  if (ord.rc) return ord.rc;
  if (n == 0) {
    HIP_OK(hipMemsetAsync(tot_dev, 0, 2 * sizeof(uint64_t), s));
    return SHM_OK;
  }
  dev::launch_scan_u64_total(in, out, n, t->bsum64, scan_tag(t, s), t->d_err, tot_dev, t->d_err,
                             lb_ctr(t, dev::kLbScan), s);
  HIP_OK(hipGetLastError());
  return SHM_OK;
}
}  // extern "C"
