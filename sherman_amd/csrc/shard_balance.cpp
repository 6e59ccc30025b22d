// shard_balance.cpp — shard boundaries that follow the stored keys: the
// splitters' set / get, the host plan of an even re-cut (shm_rebalance_plan)
// and the collective that carries it out (shm_shard_rebalance; DESIGN.md
// section 6.1).
#include "shard_internal.h"

namespace shm {
namespace shard __attribute__((visibility("hidden"))) {

bool splitters_ok(const uint64_t* sp, uint32_t P) {
  for (uint32_t j = 0; j + 1 < P; ++j)
    if (sp[j] == ~0ull || (j && sp[j] < sp[j - 1])) return false;
  return true;
}

// `per` words of this rank to every rank and theirs back, through the
// exclusive calls' transport on stream s, with a host wait: send = P runs of
// per words (run p for rank p), recv likewise (run q from rank q).  d: 2 * P *
// per device words.
int exchange_words(shm_shard* h, uint64_t* d, const std::vector<uint64_t>& send,
                   std::vector<uint64_t>& recv, uint32_t per, hipStream_t s) {
  const uint64_t w = (uint64_t)h->world * per;
  recv.assign(w, 0);
  HIP_OK2(hipMemcpyAsync(d, send.data(), 8 * w, hipMemcpyHostToDevice, s));
  RC_OK(h->xp[2]->a2a(d, d + w, per, 8, s));
  HIP_OK2(hipMemcpyAsync(recv.data(), d + w, 8 * w, hipMemcpyDeviceToHost, s));
  HIP_OK2(hipStreamSynchronize(s));
  return SHM_OK;
}

}  // namespace shard
}  // namespace shm

extern "C" {

int shm_shard_set_splitters(shm_shard* h, const uint64_t* splitters_host) {
  if (!h) return SHM_EINVAL;
  const uint32_t P = h->world;
  if (splitters_host && !splitters_ok(splitters_host, P)) return SHM_EINVAL;
  if (h->slot[0].busy || h->slot[1].busy) return SHM_EINVAL;  // a begun get was placed by the old bounds
  RC_OK(flush(h));
  // every rank passes the same words: one exchange of {set, the P - 1 words}
  std::vector<uint64_t> mine(P, 0), send((uint64_t)P * P), recv;
  mine[0] = splitters_host ? 1 : 0;
  for (uint32_t j = 0; splitters_host && j + 1 < P; ++j) mine[1 + j] = splitters_host[j];
  for (uint32_t p = 0; p < P; ++p) std::copy(mine.begin(), mine.end(), send.begin() + (uint64_t)p * P);
  DevBuf<uint64_t> d;
  RC_OK(d.alloc(2ull * P * P));
  RC_OK(exchange_words(h, d, send, recv, P, h->side));
  for (uint32_t q = 0; q < P; ++q)
    if (!std::equal(mine.begin(), mine.end(), recv.begin() + (uint64_t)q * P)) {
      fprintf(stderr, "sherman_amd: rank %u and rank %u passed different splitters\n", h->rank, q);
      return SHM_EINVAL;
    }
  if (splitters_host)
    split_bounds(h, splitters_host);
  else
    equal_bounds(h);
  h->rng.last_ok = false;
  return SHM_OK;
}

int shm_shard_get_splitters(shm_shard* h, uint64_t* out_host) {
  if (!h || (h->world > 1 && !out_host)) return SHM_EINVAL;
  for (uint32_t p = 1; p < h->world; ++p) out_host[p - 1] = h->bnd.b[p];
  return SHM_OK;
}

int shm_rebalance_plan(const uint64_t* counts, uint32_t P, uint32_t rank, uint64_t* cut,
                       uint64_t* send_cnt, uint64_t* recv_cnt) {
  if (!counts || !cut || !send_cnt || !recv_cnt || P == 0 || P > kMaxWorld || rank >= P)
    return SHM_EINVAL;
  uint64_t off[kMaxWorld + 1];
  off[0] = 0;
  for (uint32_t p = 0; p < P; ++p) off[p + 1] = off[p] + counts[p];
  const uint64_t N = off[P];
  for (uint32_t p = 0; p <= P; ++p) cut[p] = (uint64_t)(((unsigned __int128)N * p) / P);
  auto overlap = [](uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1) -> uint64_t {
    const uint64_t lo = std::max(a0, b0), hi = std::min(a1, b1);
    return hi > lo ? hi - lo : 0;
  };
  for (uint32_t p = 0; p < P; ++p) {
    send_cnt[p] = overlap(off[rank], off[rank + 1], cut[p], cut[p + 1]);
    recv_cnt[p] = overlap(off[p], off[p + 1], cut[rank], cut[rank + 1]);
  }
  return SHM_OK;
}

int shm_shard_rebalance(shm_shard* h, uint32_t leaf_fill, uint32_t internal_fill,
                        uint64_t* n_local_out, void* stream) {
  if (!h || !n_local_out) return SHM_EINVAL;
  if (h->slot[0].busy || h->slot[1].busy) return SHM_EINVAL;
  RC_OK(flush(h));
  const uint32_t P = h->world, me = h->rank;
  hipStream_t s = (hipStream_t)stream;
  Xport* xp = h->xp[2].get();
  h->rng.last_ok = false;
  // From here on a rank that fails keeps taking part until the ranks have
  // agreed (st travels with the counts and again with the splitters): no rank
  // writes its tree unless every rank can.
  shm_bulk_plan_t pl{};
  int st = shm_bulk_plan(0, leaf_fill, internal_fill, &pl);
  // the old pairs (keys [0, n_old), values [n_old, 2 n_old)), the exchanges'
  // words and the new pairs: released wherever the call returns
  DevBuf<uint64_t> pairs, d, rk;
  uint64_t n_old = 0;
  if (!st) st = shm__export_all(h->local, &pairs.p, &n_old, s);
  RC_OK(d.alloc(2ull * P * (P + 1)));
  auto first_bad = [&](const std::vector<uint64_t>& r, uint32_t per) {
    for (uint32_t q = 0; q < P; ++q)
      if (r[(uint64_t)q * per + per - 1]) return (int)(int64_t)r[(uint64_t)q * per + per - 1];
    return SHM_OK;
  };
  // the counts (an all-gather: the same {count, status} to every rank)
  std::vector<uint64_t> send(2ull * P), recv;
  for (uint32_t p = 0; p < P; ++p) {
    send[2 * p] = n_old;
    send[2 * p + 1] = (uint64_t)(int64_t)st;
  }
  RC_OK(exchange_words(h, d, send, recv, 2, s));
  RC_OK(first_bad(recv, 2));
  std::vector<uint64_t> counts(P), cut(P + 1), to(P), from(P);
  for (uint32_t p = 0; p < P; ++p) counts[p] = recv[2 * p];
  RC_OK(shm_rebalance_plan(counts.data(), P, me, cut.data(), to.data(), from.data()));
  const uint64_t N = cut[P], n_new = cut[me + 1] - cut[me];
  if (N == 0) {  // nothing stored anywhere: the bounds and the trees stay
    *n_local_out = 0;
    return SHM_OK;
  }
  // everything that can fail, before any tree is written
  st = shm_bulk_plan(n_new, leaf_fill, internal_fill, &pl);
  shm_stats_t stats{};
  if (!st) st = shm_stats(h->local, &stats);
  // as shm_bulk_load: the plan's pages and the superblock (pages_capacity
  // leaves the superblock out)
  if (!st && pl.pages > stats.pages_capacity) st = SHM_ENOMEM;
  if (!st && n_new && rk.alloc(2 * n_new)) {
    (void)hipGetLastError();
    st = SHM_ENOMEM;
  }
  // splitter j = the key at global position cut[j]: the rank holding that
  // position reads it from its export, the others contribute 0
  uint64_t my_off = 0;
  for (uint32_t p = 0; p < me; ++p) my_off += counts[p];
  std::vector<uint64_t> mine(P + 1, 0);
  for (uint32_t j = 1; j < P; ++j)
    if (cut[j] >= my_off && cut[j] - my_off < n_old &&
        hipMemcpyAsync(&mine[j - 1], pairs + (cut[j] - my_off), 8, hipMemcpyDeviceToHost, s) !=
            hipSuccess)
      st = st ? st : SHM_EIO;
  if (hipStreamSynchronize(s) != hipSuccess) st = st ? st : SHM_EIO;
  mine[P] = (uint64_t)(int64_t)st;
  send.assign((uint64_t)P * (P + 1), 0);
  for (uint32_t p = 0; p < P; ++p)
    std::copy(mine.begin(), mine.end(), send.begin() + (uint64_t)p * (P + 1));
  RC_OK(exchange_words(h, d, send, recv, P + 1, s));
  RC_OK(first_bad(recv, P + 1));
  uint64_t sp[kMaxWorld] = {};
  for (uint32_t j = 1; j < P; ++j)
    for (uint32_t q = 0; q < P; ++q) sp[j - 1] = std::max(sp[j - 1], recv[(uint64_t)q * (P + 1) + j - 1]);
  if (!splitters_ok(sp, P)) return SHM_EIO;  // the exports were not one ascending run
  // the move: destination p's contiguous run of the export, keys then values;
  // the receive buffer fills in source-rank order, so it ascends
  ExchangePlan x = plan_packed(to.data(), from.data(), P);
  if (x.ns != n_old || x.nr != n_new || x.scnt[me] != x.rcnt[me]) return SHM_EIO;
  int rc = SHM_OK;
  // this rank's own part never enters the transport
  const uint64_t own = x.scnt[me];
  if (own &&
      (hipMemcpyAsync(rk + x.roff[me], pairs + x.soff[me], 8 * own, hipMemcpyDeviceToDevice, s) !=
           hipSuccess ||
       hipMemcpyAsync(rk + n_new + x.roff[me], pairs + n_old + x.soff[me], 8 * own,
                      hipMemcpyDeviceToDevice, s) != hipSuccess))
    rc = SHM_EIO;
  x.skip(me);
  if (!rc) rc = xp->group_start();
  if (!rc) rc = xp->p2p_plan(pairs, rk, x, 8, s);
  if (!rc) rc = xp->p2p_plan(pairs ? pairs + n_old : nullptr, rk ? rk + n_new : nullptr, x, 8, s);
  if (!rc) rc = xp->group_end();
  if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = SHM_EIO;
  // the hint from the run: [first, first + 2^bits) holds every key of it
  if (!rc && n_new >= 2) {
    uint64_t fl[2] = {0, 0};
    if (hipMemcpy(&fl[0], rk, 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&fl[1], rk + n_new - 1, 8, hipMemcpyDeviceToHost) != hipSuccess)
      rc = SHM_EIO;
    const uint64_t span1 = fl[1] - fl[0];  // span - 1 >= 1 for an ascending run
    const uint32_t bits = std::max(1, 64 - __builtin_clzll(span1 | 1));
    if (!rc && fl[1] > fl[0]) rc = shm_tree_set_key_range(h->local, fl[0], bits);
  }
  if (!rc) rc = shm_bulk_load(h->local, rk, rk ? rk + n_new : nullptr, n_new, leaf_fill, internal_fill, s);
  RC_OK(rc);
  split_bounds(h, sp);
  *n_local_out = n_new;
  return SHM_OK;
}

}  // extern "C"
