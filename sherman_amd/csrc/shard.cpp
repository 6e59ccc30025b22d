// shard.cpp — the multi-GPU boundary of the C-ABI: range shards over RCCL.
//
// Replaces the reference's memory-node placement (pages spread over memory
// nodes in 32 MB chunks, include/DSM.h:198-224; every Tree::search walks
// remote pages over RDMA, src/Tree.cpp:405-459) with key-range shards: rank
// r owns [r * 2^64 / P, (r+1) * 2^64 / P) and holds a complete B-link tree of
// its slice, so no page pointer crosses GPUs and a query touches one shard.
// One exchange each way per batch, over RCCL (xGMI between the GPUs of a
// node):
//
//   search : every key straight into its owner's run of fixed-capacity
//            slots (cap = n / P + 6 sqrt(n / P) + 256, shard_plan.h
//            get_slot_cap; kKeyMax padding; a per-peer
//            cursor places it, spos records where; this rank's own run is
//            placed straight into its receive slot) -> grouped ncclSend /
//            ncclRecv of the P - 1 peers' runs and key counts (nothing at
//            P = 1) -> local batched get over all received slots (a kKeyMax
//            finds nothing) -> the peers' results back the same way ->
//            gather to input order through spos, the own run's results
//            read in place (found = value != 0, Tree.cpp:445-448).  No host wait before the key
//            exchange.  A run longer than its slot (keys far from uniform
//            over the shards, e.g. a zipf hot key) puts the rest of its keys
//            on an overflow list; end() reads the key counts back once (they
//            are ready as soon as the key exchange is), and where a count
//            passed the slot both sides know it and run a second, exact
//            round: grouped ncclSend / ncclRecv of the cut keys, a local get,
//            the values back and scattered to their inputs.  No lookup is
//            ever dropped (Tree::search always answers, Tree.cpp:405-459).
//   insert : stable bucketing by owner, the values permuted alongside, each
//            owner's run packed into a slot of max_batch / P (kKeyMax
//            padding), keys / values / counts exchanged, then the received
//            slots queued as one local insert that skips the padding: no
//            host wait (a batch holding kKeyMax routes nothing and reports
//            SHM_EINVAL, as a local insert rejects its chunk).  Received
//            slots arrive in source-rank order and the bucketing is stable,
//            so the slots apply in rank-major batch order.  A run longer
//            than its slot keeps its tail, which the next call on the shard
//            (or shm_shard_synchronize) sends in an exact second round and
//            applies before anything else; each rank's ops stay in its own
//            order, but a tail applies after every rank's slots, so across
//            ranks the result is one valid linearisation of the ranks'
//            concurrent batches (Sherman's clients are not ordered either),
//            not strict rank-major order.
//   range  : scan j's overlap with shard p is piece (p, j) of a P x n_cap
//            matrix (empty where it misses the shard); row p goes to rank p
//            (ncclAllToAll, no count exchange), the owner scans the pieces
//            (count, offsets, staged fill), the counts come back, and ONE
//            read-back of the per-peer value totals sizes the grouped
//            ncclSend / ncclRecv of the values; scan j's values are its
//            pieces' values in shard order = key order (Tree::range_query,
//            Tree.cpp:461-540, intended semantics).
//
// The shards start as equal slices; shm_shard_set_splitters and
// shm_shard_rebalance replace them with boundaries that follow the stored
// keys (shard p owns [b[p], b[p + 1]), an owner = the number of splitters <=
// the key), and every route above then cuts at those.
//
// A search is split in two calls so a caller can pipeline batches: begin
// (placement + key exchange) and end (the rest).  Each of the handle's two
// search slots has its own buffers and its own communicator (split from the
// first), so a begun batch's key exchange is never queued behind the other
// slot's value exchange; inserts and range scans use a third communicator
// and buffers of their own.
//
// The transport is an interface (shard_internal.h Xport): RCCL, or an
// in-process group of P handles on one GPU (shard_xport.cpp, which also
// creates the handles).  This unit holds the handle's lifecycle, the routed
// get and the routed insert; the range scans are shard_range.cpp's, the
// splitters and the rebalance shard_balance.cpp's, the test hooks
// shard_hooks.cpp's.  The counts and offsets of every second round come from
// shard_plan.h.
#include "shard_internal.h"

namespace shm {
namespace shard __attribute__((visibility("hidden"))) {

void equal_bounds(shm_shard* h) {
  const uint32_t P = h->world;
  h->has_split = false;
  h->split = shm::dev::RouteSplit{};
  for (uint32_t p = 0; p < P; ++p)
    h->bnd.b[p] = (uint64_t)((((unsigned __int128)p << 64) + P - 1) / P);
}
void split_bounds(shm_shard* h, const uint64_t* sp) {
  h->has_split = true;
  h->split = shm::dev::RouteSplit{};
  h->bnd.b[0] = 0;
  for (uint32_t p = 1; p < h->world; ++p) h->bnd.b[p] = h->split.s[p - 1] = sp[p - 1];
}

namespace {

// every buffer, event and stream of a handle; any failure is SHM_ENOMEM
int alloc_shard(shm_shard* h) {
  const uint32_t P = h->world;
  const uint64_t cap = h->cap;
  int rc = SHM_OK;
  for (GetSlot& s : h->slot) {
    // a peer's share of a uniform batch with its slack (get_slot_cap), never
    // more than a whole batch
    s.pcap = P == 1 ? cap : std::min<uint64_t>(cap, get_slot_cap(cap, P));
    const uint64_t slots = (uint64_t)P * s.pcap;
    rc |= s.cw.alloc(2 * (uint64_t)P + 2);
    rc |= s.ctr.alloc(shm::dev::route_ctr_words(P));
    if (s.ctr && hipMemset(s.ctr, 0, 4 * shm::dev::route_ctr_words(P)) != hipSuccess) rc |= SHM_EIO;
    rc |= s.pk.alloc(slots);
    rc |= s.pr.alloc(slots);
    rc |= s.pv.alloc(slots);
    rc |= s.pb.alloc(slots);
    rc |= s.spos.alloc(cap);
    rc |= s.ovk.alloc(cap);
    rc |= s.ovi.alloc(cap);
    rc |= s.ocnt.alloc(P);
    rc |= s.okb.alloc(cap);
    rc |= s.operm.alloc(cap);
    rc |= s.ores.alloc(cap);
    rc |= s.ev_keys.create();
  }
  InsCtx& e = h->ins;
  e.icap = P == 1 ? cap : cap / P;
  rc |= e.icnt.alloc(2 * (uint64_t)P);
  rc |= e.kb.alloc(cap);
  rc |= e.vb.alloc(cap);
  rc |= e.perm.alloc(cap);
  rc |= e.pk.alloc((uint64_t)P * e.icap);
  rc |= e.pv.alloc((uint64_t)P * e.icap);
  rc |= e.rk.alloc((uint64_t)P * e.icap);
  rc |= e.rv.alloc((uint64_t)P * e.icap);
  rc |= h->rng.rw.alloc(2 * (uint64_t)P + 8);
  rc |= e.ev_ins.create();
  rc |= h->side.create();
  equal_bounds(h);
  return rc ? SHM_ENOMEM : SHM_OK;
}

// `bytes` of device words at src, once event ev has completed (the side
// stream waits for it; the caller's stream keeps going)
int read_after(shm_shard* h, hipEvent_t ev, const void* src, uint64_t bytes, void* out) {
  HIP_OK2(hipStreamWaitEvent(h->side, ev, 0));
  return shm_read_words(h->local, src, bytes, out, h->side);
}

// Every rank must have created its tree with the same max_batch: the slot
// sizes of the exchanges derive from it (one read-back, at creation)
int check_caps(shm_shard* h) {
  const uint32_t P = h->world;
  std::vector<uint64_t> w(2 * P, h->cap);
  uint64_t* d = h->rng.rw;  // 2P + 8 words, idle until the first range scan
  HIP_OK2(hipMemcpyAsync(d, w.data(), 8ull * P, hipMemcpyHostToDevice, h->side));
  RC_OK(h->xp[2]->a2a(d, d + P, 1, 8, h->side));
  RC_OK(shm_read_words(h->local, d, 16ull * P, w.data(), h->side));
  for (uint32_t p = 0; p < P; ++p)
    if (w[P + p] != h->cap) {
      fprintf(stderr, "sherman_amd: shard %u has max_batch %llu, rank %u %llu: they must match\n",
              p, (unsigned long long)w[P + p], h->rank, (unsigned long long)h->cap);
      return SHM_EINVAL;
    }
  return SHM_OK;
}

}  // namespace

int make_shard(shm_tree* local, std::unique_ptr<Xport> (&x)[3], uint32_t world, uint32_t rank,
               shm_shard** out) {
  std::unique_ptr<shm_shard> h(new shm_shard());
  h->local = local;
  h->world = world;
  h->rank = rank;
  h->cap = shm_tree_max_batch(local);
  for (int i = 0; i < 3; ++i) {
    h->xp[i] = std::move(x[i]);
    h->xp[i]->P = world;
    h->xp[i]->rank = rank;
  }
  h->slot[0].x = h->xp[0].get();
  h->slot[1].x = h->xp[1].get();
  h->ins.x = h->rng.x = h->xp[2].get();
  RC_OK(alloc_shard(h.get()));
  RC_OK(check_caps(h.get()));
  *out = h.release();
  return SHM_OK;
}

// ---- routed insert: the overflow tails of the last insert ------------------------
// Called before anything else the shard does (and by shm_shard_synchronize):
// one read-back of the last insert's sent and received counts (ready once its
// key exchange has run); where a run passed its slot, both sides send /
// receive the tail in an exact second round, applied behind the slots.
int flush(shm_shard* h) {
  InsCtx& e = h->ins;
  if (!e.pending) return SHM_OK;
  e.pending = false;
  const uint32_t P = h->world;
  std::vector<uint64_t> c(2 * P);
  RC_OK(read_after(h, e.ev_ins, e.icnt, 16ull * P, c.data()));
  // the tail of run p lies behind its slot's worth in kb / vb
  const ExchangePlan x = plan_tails(&c[0], &c[P], P, h->rank, e.icap, TailsAt::kInRuns);
  if (x.ns == 0 && x.nr == 0) return SHM_OK;
  hipStream_t s = e.pstream;
  RC_OK(e.ork.ensure(x.nr, s));
  RC_OK(e.orv.ensure(x.nr, s));
  RC_OK(e.x->group_start());
  RC_OK(e.x->p2p_plan(e.kb, e.ork, x, 8, s));
  RC_OK(e.x->p2p_plan(e.vb, e.orv, x, 8, s));
  RC_OK(e.x->group_end());
  return x.nr ? shm_insert_batch_async(h->local, e.ork, e.orv, x.nr, s) : SHM_OK;
}

namespace {

// ---- routed get: the overflow round of one slot --------------------------------------
int get_overflow(shm_shard* h, GetSlot& s, uint64_t* vals_out, uint8_t* found_out) {
  const uint32_t P = h->world;
  std::vector<uint32_t> w(2 * P + 1);
  RC_OK(read_after(h, s.ev_keys, s.cw, 4ull * (2 * P + 1), w.data()));
  // the cut keys lie on the overflow list, which the bucketing below packs by owner
  const ExchangePlan x = plan_tails(&w[0], &w[P + 1], P, h->rank, s.ncap, TailsAt::kPacked);
  const uint64_t m = x.ns, mr = x.nr;
  if (m != w[P]) return SHM_EIO;  // the overflow list disagrees with the counts
  if (m == 0 && mr == 0) return SHM_OK;
  hipStream_t st = s.stream;
  // the cut keys grouped by owner (stable), exchanged exactly, searched, and
  // their values sent back and scattered to the inputs they came from
  if (m)
    RC_OK(shm_route_bucket_bounds(h->local, s.ovk, m, P, h->host_split(), s.ocnt, s.okb, s.operm,
                                  st));
  RC_OK(s.ork.ensure(mr, st));
  RC_OK(s.orv.ensure(mr, st));
  RC_OK(s.x->p2p_plan(s.okb, s.ork, x, 8, st));
  if (mr) RC_OK(shm_search_batch(h->local, s.ork, mr, s.orv, nullptr, st));
  RC_OK(s.x->p2p_back(s.orv, s.ores, x, 8, st));
  shm::dev::launch_route_ov_scatter(s.ores, s.operm, s.ovi, m, vals_out, found_out, st);
  return hipGetLastError() == hipSuccess ? SHM_OK : SHM_EIO;
}

}  // namespace
}  // namespace shard
}  // namespace shm

extern "C" {

int shm_shard_destroy(shm_shard* h) {
  if (!h) return SHM_EINVAL;
  const int rc = flush(h);  // a collective: every rank destroys its handle
  (void)hipDeviceSynchronize();
  delete h;  // shard_internal.h: buffers, events and the stream, then the transports
  return rc;
}

int shm_shard_synchronize(shm_shard* h) {
  if (!h) return SHM_EINVAL;
  const int rc = flush(h);
  const int rs = shm_synchronize(h->local);
  return rc ? rc : rs;
}

int shm_shard_search_begin(shm_shard* h, const uint64_t* keys, uint64_t n, void* stream,
                           uint32_t* ticket) {
  if (!h || !ticket || (n && !keys)) return SHM_EINVAL;
  const int i = h->next;
  GetSlot& s = h->slot[i];
  if (s.busy) return SHM_EINVAL;  // end the slot's batch first
  if (n > h->cap) return SHM_E2BIG;
  RC_OK(flush(h));
  h->next = (i + 1) % 2;
  s.keys = keys;
  s.n = n;
  s.stream = (hipStream_t)stream;
  *ticket = (uint32_t)i;
  const uint32_t P = h->world;
  s.ncap = P == 1 ? n : std::min<uint64_t>(s.pcap, get_slot_cap(n, P));
  // this rank's own run goes straight into its receive slot (s.pr), so only
  // the P - 1 peers' runs cross the collective (none at P = 1)
  const uint32_t me = h->rank;
  s.busy = true;
  if (P == 1 && !h->force_route) return SHM_OK;  // nothing to route: _end is the local get
  // (forced: the own run crosses the transport like the peers')
  // the runs are padded once per capacity: later batches leave earlier keys
  // of the same owner in the tails (searched, never gathered)
  const bool fill = s.filled != s.ncap;
  s.filled = s.ncap;
  shm::dev::launch_route_slots(s.keys, s.n, P, s.ncap, s.cw, s.ctr, s.pk, s.spos, s.ovk, s.ovi,
                               shm__error_word(h->local), s.stream, me,
                               h->force_route ? nullptr : s.pr + (uint64_t)me * s.ncap, fill,
                               h->route_split());
  HIP_OK2(hipGetLastError());
  RC_OK(s.x->group_start());
  RC_OK(s.x->a2a_peers(s.pk, s.pr, s.ncap, 8, s.stream));
  RC_OK(s.x->a2a_peers(s.cw, s.cw + P + 1, 1, 4, s.stream));  // keys routed to each peer
  RC_OK(s.x->group_end());
  HIP_OK2(hipEventRecord(s.ev_keys, s.stream));
  return SHM_OK;
}

int shm_shard_search_end(shm_shard* h, uint32_t ticket, uint64_t* vals_out, uint8_t* found_out) {
  if (!h || ticket >= 2u || !h->slot[ticket].busy) return SHM_EINVAL;
  GetSlot& s = h->slot[ticket];
  if (s.n && (!vals_out || !found_out)) return SHM_EINVAL;
  s.busy = false;
  const uint32_t P = h->world;
  // one shard: the batch is all this rank's, searched where it lies
  if (P == 1 && !h->force_route)
    return shm_search_batch(h->local, s.keys, s.n, vals_out, found_out, s.stream);
  RC_OK(shm_search_batch(h->local, s.pr, (uint64_t)P * s.ncap, s.pv, nullptr, s.stream));
  // the results go back the way the keys came, slot for slot; the own run's
  // are gathered straight from the local results (forced: exchanged as well)
  RC_OK(s.x->a2a_peers(s.pv, s.pb, s.ncap, 8, s.stream));
  shm::dev::launch_route_gather(s.pb, s.spos, s.n, vals_out, found_out, s.stream, h->rank, s.ncap,
                                h->force_route ? nullptr : s.pv.p);
  HIP_OK2(hipGetLastError());
  return get_overflow(h, s, vals_out, found_out);
}

int shm_shard_search(shm_shard* h, const uint64_t* keys, uint64_t n, uint64_t* vals_out,
                     uint8_t* found_out, void* stream) {
  uint32_t ticket = 0;
  RC_OK(shm_shard_search_begin(h, keys, n, stream, &ticket));
  return shm_shard_search_end(h, ticket, vals_out, found_out);
}

int shm_shard_insert(shm_shard* h, const uint64_t* keys, const uint64_t* vals, uint64_t n,
                     void* stream) {
  if (!h || (n && (!keys || !vals))) return SHM_EINVAL;
  if (n > h->cap) return SHM_E2BIG;
  RC_OK(flush(h));
  InsCtx& e = h->ins;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t P = h->world;
  // a batch holding kKeyMax routes nothing (SHM_EINVAL at the next
  // synchronising call), as a local insert rejects its chunk
  RC_OK(shm__route_bucket_insert(h->local, keys, n, P, h->host_split(), e.icnt, e.kb, e.perm, s));
  RC_OK(shm_route_permute(h->local, vals, e.perm, n, e.vb, s));
  // this rank's own run is packed straight into its receive slot (forced:
  // it crosses the transport like the peers')
  const uint64_t mine = (uint64_t)h->rank * e.icap;
  const bool fr = h->force_route;
  shm::dev::launch_route_pack(e.kb, e.vb, e.icnt, P, e.icap, e.pk, e.pv, s, h->rank,
                              fr ? nullptr : e.rk + mine, fr ? nullptr : e.rv + mine);
  HIP_OK2(hipGetLastError());
  RC_OK(e.x->group_start());
  RC_OK(e.x->a2a_peers(e.pk, e.rk, e.icap, 8, s));
  RC_OK(e.x->a2a_peers(e.pv, e.rv, e.icap, 8, s));
  RC_OK(e.x->a2a_peers(e.icnt, e.icnt + P, 1, 8, s));
  RC_OK(e.x->group_end());
  HIP_OK2(hipEventRecord(e.ev_ins, s));
  e.pending = P > 1 || fr;
  e.pstream = s;
  return shm__insert_batch_padded(h->local, e.rk, e.rv, (uint64_t)P * e.icap, s);
}

}  // extern "C"
