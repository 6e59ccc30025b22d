// shard_range.cpp — the routed range scans of a shard (the protocol: the
// comment at the head of shard.cpp, "range"): the pieces to their shards, the
// owners' scans, the counts back, and the values either in exact runs sized by
// one read-back (shm_shard_range_query) or in fixed runs with no host wait
// (shm_shard_range_query_async).
#include "shard_internal.h"

namespace {

// What both forms begin with: the arguments they share, the piece matrices
// of P x n_cap (SHM_E2BIG past a batch), the last insert's tails.  The last
// batch is forgotten here, whatever follows.
int range_begin(shm_shard* h, const uint64_t* from, const uint64_t* to, uint64_t n, uint64_t n_cap,
                const uint64_t* counts_out, const uint64_t* offsets_out, const uint64_t* vals_out,
                uint64_t vals_cap, hipStream_t s) {
  if (n > n_cap || (n && (!from || !to || !counts_out || !offsets_out)) || (vals_cap && !vals_out))
    return SHM_EINVAL;
  const uint64_t m = (uint64_t)h->world * n_cap;
  if (m > h->cap) return SHM_E2BIG;
  RC_OK(flush(h));
  RangeCtx& e = h->rng;
  e.last_ok = false;
  if (m <= e.pcap && e.plo) return SHM_OK;
  HIP_OK2(hipStreamSynchronize(s));
  e.pcap = m;
  int rc = SHM_OK;
  for (DevBuf<uint64_t>* b : {&e.plo, &e.phi, &e.rlo, &e.rhi, &e.rc, &e.roff, &e.bc, &e.bsc})
    rc |= b->alloc(m);
  return rc ? SHM_ENOMEM : SHM_OK;
}

// ... and end with: what shm_shard_range_values needs of the batch (ok: its
// total is known on the host)
void range_done(RangeCtx& e, uint64_t n, uint64_t n_cap, uint64_t total, const uint64_t* offsets,
                bool ok) {
  e.last_n = n;
  e.last_ncap = n_cap;
  e.last_total = total;
  e.last_off = offsets;
  e.last_ok = ok;
}

// steps 1-3 of a routed range scan batch, all on the device: pieces to their
// shards, the local scans of the received pieces (values packed in rvals,
// row p = rank p's), counts back, per-peer totals (rw), counts_out,
// offsets_out and the received runs' offsets (bsc)
int range_scan_pieces(shm_shard* h, const uint64_t* from, const uint64_t* to, uint64_t n,
                      uint64_t n_cap, uint64_t* counts_out, uint64_t* offsets_out, hipStream_t s) {
  const uint32_t P = h->world;
  const uint64_t m = (uint64_t)P * n_cap;
  RangeCtx& e = h->rng;
  uint64_t* rw = e.rw;  // [0, P) sent, [P, 2P) received, scanner {total, err}, scans {total, err}, bsc {total, err}
  // 1. pieces, row p to rank p
  shm::dev::launch_range_pieces(from, to, n, n_cap, P, h->bnd, e.plo, e.phi, s);
  HIP_OK2(hipGetLastError());
  RC_OK(e.x->group_start());
  RC_OK(e.x->a2a(e.plo, e.rlo, n_cap, 8, s));
  RC_OK(e.x->a2a(e.phi, e.rhi, n_cap, 8, s));
  RC_OK(e.x->group_end());
  // 2. this shard scans every received piece (count, offsets, staged fill)
  RC_OK(shm_range_query_batch_async(h->local, e.rlo, e.rhi, m, e.rc, e.roff, e.rvals, e.rvals.cap,
                                    rw + 2 * P, s));
  // 3. piece counts back; per-peer totals, per-scan counts and offsets
  RC_OK(e.x->a2a(e.rc, e.bc, n_cap, 8, s));
  shm::dev::launch_range_sums(e.rc, e.bc, n, n_cap, P, rw, counts_out, s);
  HIP_OK2(hipGetLastError());
  RC_OK(shm__scan_u64(h->local, counts_out, offsets_out, n, rw + 2 * P + 2, s));
  RC_OK(shm__scan_u64(h->local, e.bc, e.bsc, m, rw + 2 * P + 4, s));
  return SHM_OK;
}

}  // namespace

extern "C" {

int shm_shard_range_query(shm_shard* h, const uint64_t* from, const uint64_t* to, uint64_t n,
                          uint64_t n_cap, uint64_t* counts_out, uint64_t* offsets_out,
                          uint64_t* vals_out, uint64_t vals_cap, uint64_t* total_out,
                          void* stream) {
  if (!h || !total_out) return SHM_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  RC_OK(range_begin(h, from, to, n, n_cap, counts_out, offsets_out, vals_out, vals_cap, s));
  const uint32_t P = h->world;
  const uint64_t m = (uint64_t)P * n_cap;
  RangeCtx& e = h->rng;
  // about n_cap non-empty pieces of ~100 values (C5): grown when a batch needs more
  if (!e.rvals) RC_OK(e.rvals.ensure(std::max<uint64_t>(n_cap * 160, 1u << 20), s));
  RC_OK(range_scan_pieces(h, from, to, n, n_cap, counts_out, offsets_out, s));
  // 4. the one host synchronisation: the value counts each way
  std::vector<uint64_t> w(2 * P + 6);
  RC_OK(shm_read_words(h->local, e.rw, 8ull * (2 * P + 6), w.data(), s));
  const uint64_t scanned = w[2 * P], total = w[2 * P + 2];
  if (scanned > e.rvals.cap) {
    // the fill pass dropped values past its buffer: grow it, fill again
    RC_OK(e.rvals.ensure(scanned, s));
    RC_OK(shm_range_query(h->local, e.rlo, e.rhi, m, e.rc, e.roff, e.rvals, s));
  }
  const ExchangePlan x = plan_packed(&w[0], &w[P], P);
  if (x.ns != scanned || x.nr != total) return SHM_EIO;
  RC_OK(e.bv.ensure(x.nr, s));
  RC_OK(e.x->p2p_plan(e.rvals, e.bv, x, 8, s));
  *total_out = total;
  range_done(e, n, n_cap, total, offsets_out, true);
  // counts / offsets stay valid; shm_shard_range_values fills a larger buffer
  if (total > vals_cap) return SHM_ENOSPC;
  shm::dev::launch_range_assemble(e.bv, e.bc, e.bsc, n, n_cap, P, offsets_out, vals_out, vals_cap,
                                  s);
  return hipGetLastError() == hipSuccess ? SHM_OK : SHM_EIO;
}

int shm_shard_range_query_async(shm_shard* h, const uint64_t* from, const uint64_t* to,
                                uint64_t n, uint64_t n_cap, uint64_t* counts_out,
                                uint64_t* offsets_out, uint64_t* vals_out, uint64_t vals_cap,
                                uint64_t peer_cap, uint64_t* status, void* stream) {
  if (!h || !status || peer_cap == 0) return SHM_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  RC_OK(range_begin(h, from, to, n, n_cap, counts_out, offsets_out, vals_out, vals_cap, s));
  const uint32_t P = h->world;
  RangeCtx& e = h->rng;
  // fixed runs of peer_cap values per peer each way: the scan pass's buffer
  // holds every run that fits (a longer one is flagged, not grown)
  const uint64_t runs = (uint64_t)P * peer_cap;
  RC_OK(e.rvals.ensure(runs, s));
  RC_OK(e.pvs.ensure(runs, s));
  RC_OK(e.bv.ensure(runs, s));
  RC_OK(range_scan_pieces(h, from, to, n, n_cap, counts_out, offsets_out, s));
  // 4. the runs padded to peer_cap on the device, exchanged whole
  shm::dev::launch_range_pitch(e.rvals, e.rw, P, peer_cap, e.pvs, e.rvals.cap, vals_cap, status, s);
  HIP_OK2(hipGetLastError());
  RC_OK(e.x->a2a(e.pvs, e.bv, peer_cap, 8, s));
  // the total is on the device (status[0]): shm_shard_range_values needs it
  // on the host, so not after this call
  range_done(e, n, n_cap, 0, offsets_out, false);
  shm::dev::launch_range_assemble(e.bv, e.bc, e.bsc, n, n_cap, P, offsets_out, vals_out, vals_cap,
                                  s, peer_cap);
  return hipGetLastError() == hipSuccess ? SHM_OK : SHM_EIO;
}

int shm_shard_range_values(shm_shard* h, uint64_t* vals_out, uint64_t vals_cap, void* stream) {
  if (!h || !h->rng.last_ok || (h->rng.last_total && !vals_out)) return SHM_EINVAL;
  const RangeCtx& e = h->rng;
  if (e.last_total > vals_cap) return SHM_ENOSPC;
  shm::dev::launch_range_assemble(e.bv, e.bc, e.bsc, e.last_n, e.last_ncap, h->world, e.last_off,
                                  vals_out, vals_cap, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? SHM_OK : SHM_EIO;
}

}  // extern "C"
