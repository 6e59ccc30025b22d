// shard_plan.h — the host arithmetic of the shard's exchanges: the capacity of
// a routed get's slot, and the per-peer counts and offsets of a grouped
// point-to-point exchange (Xport::p2p), built in one place so that every
// caller agrees on them.  No HIP, no RCCL: tests/native/shard_plan_test.cpp
// checks it on the CPU, for every rank of a world at once.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

namespace shm {
namespace shard __attribute__((visibility("hidden"))) {

// A routed get's slot per peer: n / P + 6 sigma of the binomial count of
// keys a peer gets from n uniform (hashed) keys, + 256.  Past it a run's
// tail takes the exact overflow round (get_overflow), so a skewed batch is
// slower, never wrong; at C4's 2^20 keys and P = 8 the slots carry 1.9 %
// padding where 1.25 n / P + 256 carried 25 % (fewer bytes over xGMI, fewer
// padding lanes in the walk).
inline uint64_t get_slot_cap(uint64_t n, uint32_t P) {
  const uint64_t m = n / P;
  return m + 6 * (uint64_t)std::sqrt((double)m) + 256;
}

// One grouped point-to-point exchange as a rank sees it: scnt[p] elements at
// soff[p] of its send buffer go to peer p, rcnt[p] elements from peer p land
// at roff[p] of its receive buffer.  The exchange is sound when rank r's
// scnt[p] equals rank p's rcnt[r], for every pair.
struct ExchangePlan {
  std::vector<uint64_t> scnt, soff, rcnt, roff;
  uint64_t ns = 0, nr = 0;  // the sums of scnt and of rcnt as they were built
  explicit ExchangePlan(uint32_t P) : scnt(P, 0), soff(P, 0), rcnt(P, 0), roff(P, 0) {}
  // peer p's part travels another way (a rank's own part, copied in place);
  // the offsets and the totals stay
  void skip(uint32_t p) { scnt[p] = rcnt[p] = 0; }
};

// send[p] elements to peer p and recv[p] from it, each side packed in peer
// order
template <class C>
ExchangePlan plan_packed(const C* send, const C* recv, uint32_t P) {
  ExchangePlan x(P);
  for (uint32_t p = 0; p < P; ++p) {
    x.scnt[p] = send[p];
    x.soff[p] = x.ns;
    x.ns += x.scnt[p];
    x.rcnt[p] = recv[p];
    x.roff[p] = x.nr;
    x.nr += x.rcnt[p];
  }
  return x;
}

// where the tail of the run for peer p starts in the send buffer
enum class TailsAt {
  kInRuns,  // the buffer holds the whole runs in peer order: behind run p's first cap elements
  kPacked,  // the buffer holds only the tails, in peer order
};

// The second round of an exchange through slots of cap elements per peer: the
// part of every run past its slot.  sent[p]: the elements this rank routed to
// peer p; received[p]: the elements peer p routed to this rank, as the first
// round's count exchange delivered them.  A rank's own run never crosses the
// transport, so its received count is the one it sent itself.  The tails
// received are packed in peer order.
template <class C>
ExchangePlan plan_tails(const C* sent, const C* received, uint32_t P, uint32_t rank, uint64_t cap,
                        TailsAt at) {
  ExchangePlan x(P);
  uint64_t run = 0;  // where run p starts when the buffer holds whole runs
  for (uint32_t p = 0; p < P; ++p) {
    const uint64_t out = sent[p], got = p == rank ? sent[p] : received[p];
    x.scnt[p] = out > cap ? out - cap : 0;
    x.soff[p] = at == TailsAt::kInRuns ? run + cap : x.ns;
    run += out;
    x.ns += x.scnt[p];
    x.rcnt[p] = got > cap ? got - cap : 0;
    x.roff[p] = x.nr;
    x.nr += x.rcnt[p];
  }
  return x;
}

}  // namespace shard
}  // namespace shm
