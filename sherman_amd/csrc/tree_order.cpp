// tree_order.cpp — order statistics: the order index and the calls that answer
// from it (shm_rank_batch, shm_count_batch, shm_select_batch, shm_order_stats).
//
// The index is the whole tree's leaf units in key order as the export's count
// pass lists them (tree_image.cpp order_count: page, bound and the exclusive
// scan of the valid-pair counts), copied out of the export workspace, which
// the next export overwrites, with the total appended and two pyramids of
// sampled levels for the searches (order.hip).  Its validity is a generation:
// every host-side issue of work that can change the stored pairs or the pages
// bumps shm_tree::ord_gen, and a call here rebuilds the index first when it
// was built at another generation.  The rebuilding call is synchronising (the
// count pass reads its totals); with the index valid a call queues one kernel.
#include "tree_internal.h"

namespace shm {
namespace host __attribute__((visibility("hidden"))) {

namespace {
constexpr uint64_t kFan = dev::kOrdFan;
uint64_t blocks_of(uint64_t n) { return (n + kFan - 1) / kFan; }

// where the index's parts stand, in words from its start, for `units` units
struct OrdLayout {
  uint64_t page = 0, off = 0;  // off: units + 1 words, off + 1 on a block boundary
  uint64_t blv[dev::kOrdLevels], olv[dev::kOrdLevels];
  uint64_t nblk[dev::kOrdLevels];
  uint32_t nlev = 0;
  uint64_t words = 0;
};
OrdLayout order_layout(uint64_t units) {
  OrdLayout l{};
  uint64_t at = 0;
  l.page = at;
  at += blocks_of(units) * kFan;
  // level 0 holds `units` words, level j + 1 one word per block of level j;
  // the first level that is one block is the top
  uint64_t n = units;
  for (uint32_t j = 0; j < (uint32_t)dev::kOrdLevels; ++j) {
    l.nblk[j] = blocks_of(n);
    l.nlev = j + 1;
    if (l.nblk[j] == 1) break;
    n = l.nblk[j];
  }
  for (uint32_t j = 0; j < l.nlev; ++j) {
    l.blv[j] = at;
    at += l.nblk[j] * kFan;
  }
  // off[0] in the last word of a block of its own, so that off[1 ..], the
  // searched array, starts a block
  l.off = at + kFan - 1;
  at += kFan;
  for (uint32_t j = 0; j < l.nlev; ++j) {
    l.olv[j] = at;
    at += l.nblk[j] * kFan;
  }
  l.words = at;
  return l;
}

// the index of the tree as it is: built when none is, or when work that can
// change the pairs was issued since the last build
int order_refresh(shm_tree* t, hipStream_t s) {
  shm_tree::Oidx& o = t->oidx;
  if (o.valid && o.gen == t->ord_gen) return SHM_OK;
  const auto t0 = std::chrono::steady_clock::now();
  o.valid = false;
  const uint64_t *page, *bound, *off, *total_dev;
  uint64_t total = 0;
  if (const int rc = order_count(t, s, &page, &bound, &off, &total_dev, &total)) return rc;
  const uint64_t units = t->ex_units;
  const OrdLayout l = order_layout(units);
  if (l.words > o.cap_words) {
    // headroom as the export workspace has it, so a growing tree does not
    // reallocate at every build
    const uint64_t cap = order_layout(units + units / 4 + 1024).words;
    uint64_t* nw = nullptr;
    if (dalloc(&nw, cap)) {
      (void)hipGetLastError();
      return SHM_ENOMEM;  // the old allocation stays, unused: the handle is as it was
    }
    if (o.ws) (void)hipFree(o.ws);
    o.ws = nw;
    o.cap_words = cap;
  }
  // every pad word is ~0: above every searched value
  HIP_OK(hipMemsetAsync(o.ws, 0xFF, l.words * sizeof(uint64_t), s));
  const size_t ub = units * sizeof(uint64_t);
  HIP_OK(hipMemcpyAsync(o.ws + l.page, page, ub, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(o.ws + l.blv[0], bound, ub, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(o.ws + l.off, off, ub, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(o.ws + l.off + units, total_dev, sizeof(uint64_t),
                        hipMemcpyDeviceToDevice, s));
  uint64_t n = units;
  for (uint32_t j = 0; j + 1 < l.nlev; ++j) {
    dev::launch_order_sample(o.ws + l.blv[j], n, o.ws + l.blv[j + 1], s);
    dev::launch_order_sample(o.ws + l.olv[j], n, o.ws + l.olv[j + 1], s);
    n = l.nblk[j];
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(s));
  o.units = units;
  o.total = total;
  o.max_pages = t->next_page;
  o.gen = t->ord_gen;
  o.valid = true;
  o.builds += 1;
  o.last_ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SHM_OK;
}

dev::OrderArgs order_args(const shm_tree* t, uint64_t* status) {
  const shm_tree::Oidx& o = t->oidx;
  const OrdLayout l = order_layout(o.units);
  dev::OrderArgs a = arena_args<dev::OrderArgs>(t);
  a.status = status;
  a.page = o.ws + l.page;
  a.bound = o.ws + l.blv[0];
  a.off = o.ws + l.off;
  for (uint32_t j = 0; j < l.nlev; ++j) {
    a.blv[j] = o.ws + l.blv[j];
    a.olv[j] = o.ws + l.olv[j];
    a.nblk[j] = l.nblk[j];
  }
  a.nlev = l.nlev;
  a.units = o.units;
  a.total = o.total;
  a.max_pages = o.max_pages;
  return a;
}

// the part the three calls share: ordering, the ticket rule, the index, the
// launch.  The arguments were checked
template <class Fill>
int order_call(shm_tree* t, uint64_t n, uint64_t* status_dev, void* stream,
               void (*launch)(const dev::OrderArgs&, hipStream_t), Fill&& fill) {
  std::lock_guard<std::mutex> g(t->mu);
  if (t->sync.n_pend) return SHM_EINVAL;  // an ordered chunk waits for its apply
  hipStream_t s = pick(stream);
  Order ord(t, s, true);  // the export workspace of a rebuild; later calls follow
  if (ord.rc) return ord.rc;
  if (const int rc = order_refresh(t, s)) return rc;
  dev::OrderArgs a = order_args(t, status_dev);
  a.n = n;
  fill(a);
  t->err_pending = true;
  return timed_launch(t, s, n, [&] { launch(a, s); });
}
}  // namespace

}  // namespace host
}  // namespace shm

extern "C" {

int shm_rank_batch(shm_tree* t, const uint64_t* keys, uint64_t n, uint64_t* ranks_out,
                   uint64_t* status_dev, void* stream) {
  // the arguments first: a rejected call uses neither the handle nor the GPU
  if (n && (!keys || !ranks_out)) return SHM_EINVAL;
  if (!t) return SHM_EINVAL;
  if (n == 0) return SHM_OK;
  return order_call(t, n, status_dev, stream, dev::launch_order_rank, [&](dev::OrderArgs& a) {
    a.in0 = keys;
    a.out0 = ranks_out;
  });
}

int shm_count_batch(shm_tree* t, const uint64_t* from, const uint64_t* to, uint64_t n,
                    uint64_t* counts_out, uint64_t* status_dev, void* stream) {
  if (n && (!from || !to || !counts_out)) return SHM_EINVAL;
  if (!t) return SHM_EINVAL;
  if (n == 0) return SHM_OK;
  return order_call(t, n, status_dev, stream, dev::launch_order_count, [&](dev::OrderArgs& a) {
    a.in0 = from;
    a.in1 = to;
    a.out0 = counts_out;
  });
}

int shm_select_batch(shm_tree* t, const uint64_t* ranks, uint64_t n, uint64_t* keys_out,
                     uint64_t* vals_out, uint8_t* found_out, uint64_t* status_dev, void* stream) {
  if (n && (!ranks || (!keys_out && !vals_out && !found_out))) return SHM_EINVAL;
  if (!t) return SHM_EINVAL;
  if (n == 0) return SHM_OK;
  return order_call(t, n, status_dev, stream, dev::launch_order_select, [&](dev::OrderArgs& a) {
    a.in0 = ranks;
    a.out0 = keys_out;
    a.out1 = vals_out;
    a.found = found_out;
  });
}

int shm_order_stats(shm_tree* t, shm_order_stats_t* out) {
  if (!t || !out) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  const shm_tree::Oidx& o = t->oidx;
  out->units = o.units;
  out->pairs = o.total;
  out->bytes = o.cap_words * sizeof(uint64_t);
  out->builds = o.builds;
  out->last_build_ms = o.last_ms;
  return SHM_OK;
}
}  // extern "C"
