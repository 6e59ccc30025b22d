// shard_internal.h — what the shard's units (shard*.cpp) share: the status
// macros, the three owning types (a device buffer, an event, a stream), the
// transport interface, the per-context state, the handle (struct shm_shard)
// and the declarations of the helpers that cross a unit boundary.  Host only:
// included by shard*.cpp and by nothing else.  Every helper is defined in
// exactly one unit, named above its declaration; everything in shm::shard is
// hidden from the library's dynamic symbols.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../include/sherman_amd.h"
#include "kernels.h"
#include "shard_plan.h"
#include "tree_hooks.h"

#define HIP_OK2(expr)                                 \
  do {                                                \
    if ((expr) != hipSuccess) return SHM_EIO;         \
  } while (0)
#define RC_OK(expr)                                   \
  do {                                                \
    const int _rc = (expr);                           \
    if (_rc) return _rc;                              \
  } while (0)

namespace shm {
namespace shard __attribute__((visibility("hidden"))) {

constexpr uint32_t kMaxWorld = 16;

// ---- owners ---------------------------------------------------------------------
// Each holds one HIP resource, releases it in its destructor, is never copied
// (a buffer moves; an event or a stream stays where it was created) and
// converts to the raw handle where a call takes one.

// a device buffer and the element count it was sized for
template <class T>
struct DevBuf {
  T* p = nullptr;
  uint64_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.detach(); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      o.detach();
    }
    return *this;
  }
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) (void)hipFree(p);
    detach();
  }
  // the pointer leaves with the caller
  T* detach() {
    T* q = p;
    p = nullptr;
    cap = 0;
    return q;
  }
  // count elements (at least one, so an empty buffer is still a pointer);
  // what it held before goes first
  int alloc(uint64_t count) {
    release();
    if (hipMalloc((void**)&p, sizeof(T) * std::max<uint64_t>(count, 1)) != hipSuccess) {
      p = nullptr;
      return SHM_ENOMEM;
    }
    cap = count;
    return SHM_OK;
  }
  // grow to >= need elements, with a quarter and 1024 to spare (waits for
  // the stream before the old buffer goes; the contents are not kept)
  int ensure(uint64_t need, hipStream_t s) {
    if (need <= cap && p) return SHM_OK;
    HIP_OK2(hipStreamSynchronize(s));
    return alloc(need + need / 4 + 1024);
  }
};

// an event without timing
struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(const DevEvent&) = delete;
  ~DevEvent() {
    if (e) (void)hipEventDestroy(e);
  }
  operator hipEvent_t() const { return e; }
  int create() {
    return hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess ? SHM_OK : SHM_EIO;
  }
};

// a non-blocking stream
struct DevStream {
  hipStream_t s = nullptr;
  DevStream() = default;
  DevStream(const DevStream&) = delete;
  ~DevStream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
  int create() {
    return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? SHM_OK : SHM_EIO;
  }
};

// ---- transports (shard_xport.cpp) -------------------------------------------------
struct Xport {
  uint32_t P = 1, rank = 0;
  // a2a_peers also exchanges this rank's own part with itself (shm__shard_
  // force_route: a world-1 shard's routed path through the transport)
  bool self_too = false;
  virtual ~Xport() = default;
  virtual int group_start() { return SHM_OK; }
  virtual int group_end() { return SHM_OK; }
  // `count` elements of eb (4 or 8) bytes to and from every peer: peer p's
  // part of send / recv at p * count
  virtual int a2a(const void* send, void* recv, uint64_t count, int eb, hipStream_t s) = 0;
  // a2a without this rank's own part (it never leaves the rank: the callers
  // place it straight where the local kernel reads it); nothing at P = 1
  virtual int a2a_peers(const void* send, void* recv, uint64_t count, int eb, hipStream_t s) = 0;
  // grouped point-to-point: scnt[p] elements at send + soff[p] to peer p,
  // rcnt[p] elements from peer p to recv + roff[p] (both sides know both)
  virtual int p2p(const void* send, const uint64_t* scnt, const uint64_t* soff, void* recv,
                  const uint64_t* rcnt, const uint64_t* roff, int eb, hipStream_t s) = 0;
  // one plan, forwards (send -> recv) ...
  int p2p_plan(const void* send, void* recv, const ExchangePlan& x, int eb, hipStream_t s) {
    return p2p(send, x.scnt.data(), x.soff.data(), recv, x.rcnt.data(), x.roff.data(), eb, s);
  }
  // ... and the answers back the way the requests came
  int p2p_back(const void* send, void* recv, const ExchangePlan& x, int eb, hipStream_t s) {
    return p2p(send, x.rcnt.data(), x.roff.data(), recv, x.scnt.data(), x.soff.data(), eb, s);
  }
};

// ---- per-context state ------------------------------------------------------------
// a search slot: one routed get in flight
struct GetSlot {
  Xport* x = nullptr;
  uint64_t pcap = 0;          // slot capacity per peer (allocated)
  uint64_t ncap = 0;          // this batch's: min(pcap, get_slot_cap(n, P))
  DevBuf<uint32_t> cw;        // [P] keys routed to each peer, [P] overflow count, [P + 1 ..] received counts
  DevBuf<uint32_t> ctr;       // the placement's claim words (route_ctr_words), zero at rest
  uint64_t filled = 0;        // the capacity the runs were last padded at (0: never)
  DevBuf<uint64_t> pk, pr, pv, pb;  // P * pcap
  DevBuf<uint32_t> spos;      // input -> slot
  DevBuf<uint64_t> ovk;       // overflow list: keys, their inputs
  DevBuf<uint32_t> ovi;
  DevBuf<uint64_t> ocnt;      // overflow round: bucket counts [P], keys by owner, permutation, results
  DevBuf<uint64_t> okb;
  DevBuf<uint32_t> operm;
  DevBuf<uint64_t> ores;
  DevBuf<uint64_t> ork, orv;  // received overflow keys / their values (grown on demand)
  DevEvent ev_keys;
  const uint64_t* keys = nullptr;
  uint64_t n = 0;
  hipStream_t stream = nullptr;
  bool busy = false;
};

// routed inserts (exclusive calls on the tree)
struct InsCtx {
  Xport* x = nullptr;
  uint64_t icap = 0;          // insert slot per peer: max_batch / P
  DevBuf<uint64_t> icnt;      // bucket counts: [P] sent, [P] received
  DevBuf<uint64_t> kb, vb;
  DevBuf<uint32_t> perm;
  DevBuf<uint64_t> pk, pv, rk, rv;  // P * icap
  DevBuf<uint64_t> ork, orv;  // overflow tails received (grown on demand)
  DevEvent ev_ins;
  bool pending = false;       // an insert whose overflow check is still due
  hipStream_t pstream = nullptr;
};

// routed range scans (exclusive calls, over the same transport as inserts)
struct RangeCtx {
  Xport* x = nullptr;
  // P x n_cap piece matrices (grown on demand, all eight together)
  uint64_t pcap = 0;
  DevBuf<uint64_t> plo, phi, rlo, rhi, rc, roff, bc, bsc;
  DevBuf<uint64_t> rvals;     // the values this rank's scans of received pieces found
  DevBuf<uint64_t> bv;        // the values received back
  DevBuf<uint64_t> pvs;       // async scans: the values to send, peer_cap per peer
  DevBuf<uint64_t> rw;        // [2P + 8] small words read back once per scan batch
  // the last batch, for shm_shard_range_values after SHM_ENOSPC
  uint64_t last_n = 0, last_ncap = 0, last_total = 0;
  const uint64_t* last_off = nullptr;
  bool last_ok = false;
};

}  // namespace shard
}  // namespace shm

// Members are destroyed last to first: the side stream, the contexts' buffers
// and events, then the transports 2, 1, 0 -- xp[0] may own the base
// communicator the other two were split from, and no buffer outlives the
// transport it was exchanged over.  xp stays the first resource member.
struct __attribute__((visibility("hidden"))) shm_shard {
  shm_tree* local = nullptr;
  uint32_t world = 1, rank = 0;
  uint64_t cap = 0;               // the local tree's max_batch
  std::unique_ptr<shm::shard::Xport> xp[3];  // search slots 0 / 1, exclusive calls
  shm::shard::GetSlot slot[2];
  int next = 0;
  shm::shard::InsCtx ins;
  shm::shard::RangeCtx rng;
  shm::shard::DevStream side;     // read-backs that wait on an event
  shm::dev::ShardBounds bnd{};
  // shm_shard_set_splitters / shm_shard_rebalance: the boundaries b[1 .. P - 1]
  // as the routing kernels take them; unset: equal slices (the kernels and
  // bnd as they were before splitters)
  bool has_split = false;
  shm::dev::RouteSplit split{};
  const shm::dev::RouteSplit* route_split() const { return has_split ? &split : nullptr; }
  const uint64_t* host_split() const { return has_split ? split.s : nullptr; }
  // shm__shard_force_route: even at world 1 every get and insert takes the
  // routed path -- slot placement, the exchange through the transport (each
  // rank's own run included, so RCCL sends it to itself), the local batch,
  // the results back, the gather -- as at world > 1
  bool force_route = false;
};

namespace shm {
namespace shard __attribute__((visibility("hidden"))) {

// ---- shard.cpp ----------------------------------------------------------------
// the handle over three transports of one kind (taken over, also on failure)
int make_shard(shm_tree* local, std::unique_ptr<Xport> (&x)[3], uint32_t world, uint32_t rank,
               shm_shard** out);
// the overflow tails of the last routed insert: before anything else a call
// on the shard does
int flush(shm_shard* h);
// shard p owns [ceil(p 2^64 / P), ceil((p + 1) 2^64 / P))
void equal_bounds(shm_shard* h);
// shard p owns [sp[p - 1], sp[p]) (sp: P - 1 ascending words; b[0] = 0)
void split_bounds(shm_shard* h, const uint64_t* sp);

// ---- shard_balance.cpp --------------------------------------------------------
// P - 1 host words: ascending (repeats allowed), none kKeyMax
bool splitters_ok(const uint64_t* sp, uint32_t P);
int exchange_words(shm_shard* h, uint64_t* d, const std::vector<uint64_t>& send,
                   std::vector<uint64_t>& recv, uint32_t per, hipStream_t s);

}  // namespace shard
}  // namespace shm

using namespace shm::shard;
