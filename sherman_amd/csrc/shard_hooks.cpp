// shard_hooks.cpp — library-internal test hooks of the shard's routing, not
// part of include/sherman_amd.h (the in-process group's are with the
// transports, shard_xport.cpp).
#include "shard_internal.h"

namespace {

// the claim words of the hooks' placements (zero at rest; one call at a time;
// kept for the life of the process)
uint32_t* hook_ctr() {
  static uint32_t* c = nullptr;
  if (!c) {
    const uint64_t words = shm::dev::route_ctr_words(64);
    DevBuf<uint32_t> b;
    if (b.alloc(words) == SHM_OK && hipMemset(b, 0, 4 * words) == hipSuccess) c = b.detach();
  }
  return c;
}

// The routed get's slot placement for P shards, so the placement can be
// checked on one GPU without P ranks (tests/test_gpu_shard.py).  cursor:
// P + 1 u32 of device scratch; ovk / ovi nullable (then the overflow bit
// goes to t's error word); fill: pad the runs (the shard pads only when a
// slot's capacity changed); splitters_host: P - 1 host words, nullable;
// mode: the owner search (kernels.h RouteSplit: 0 or 2 LDS, 1 kernel
// arguments).
int route_slots(shm_tree* t, const uint64_t* keys, uint64_t n, uint32_t P, uint64_t cap,
                uint32_t* cursor, uint64_t* slots, uint32_t* spos, uint64_t* ovk, uint32_t* ovi,
                bool fill, const uint64_t* splitters_host, int mode, void* stream) {
  if (!t || !cursor || !slots || !spos || P == 0 || P > 64 || (n && !keys) ||
      (uint64_t)P * cap >= ~0u || (splitters_host && !splitters_ok(splitters_host, P)))
    return SHM_EINVAL;
  uint32_t* ctr = hook_ctr();
  if (!ctr) return SHM_ENOMEM;
  shm::dev::RouteSplit sp{};
  for (uint32_t j = 0; splitters_host && j + 1 < P; ++j) sp.s[j] = splitters_host[j];
  shm::dev::launch_route_slots(keys, n, P, cap, cursor, ctr, slots, spos, ovk, ovi,
                               shm__error_word(t), (hipStream_t)stream, 0, nullptr, fill,
                               splitters_host ? &sp : nullptr, mode);
  return hipGetLastError() == hipSuccess ? SHM_OK : SHM_EIO;
}

}  // namespace

extern "C" {

// (1) the placement with equal slices, the runs padded ...
int shm__route_slots(shm_tree* t, const uint64_t* keys, uint64_t n, uint32_t P, uint64_t cap,
                     uint32_t* cursor, uint64_t* slots, uint32_t* spos, uint64_t* ovk,
                     uint32_t* ovi, void* stream) {
  return route_slots(t, keys, n, P, cap, cursor, slots, spos, ovk, ovi, true, nullptr, 0, stream);
}
// ... the shard's own form of it: padded only when fill ...
int shm__route_slots_ex(shm_tree* t, const uint64_t* keys, uint64_t n, uint32_t P, uint64_t cap,
                        uint32_t* cursor, uint64_t* slots, uint32_t* spos, uint64_t* ovk,
                        uint32_t* ovi, int fill, void* stream) {
  return route_slots(t, keys, n, P, cap, cursor, slots, spos, ovk, ovi, fill != 0, nullptr, 0,
                     stream);
}
// ... and with splitters and the owner search named
int shm__route_slots_bounds(shm_tree* t, const uint64_t* keys, uint64_t n, uint32_t P, uint64_t cap,
                            uint32_t* cursor, uint64_t* slots, uint32_t* spos, uint64_t* ovk,
                            uint32_t* ovi, int fill, const uint64_t* splitters_host, int mode,
                            void* stream) {
  return route_slots(t, keys, n, P, cap, cursor, slots, spos, ovk, ovi, fill != 0, splitters_host,
                     mode, stream);
}
// the result gather that goes with them
int shm__route_gather(const uint64_t* in, const uint32_t* spos, uint64_t n, uint64_t* vals_out,
                      uint8_t* found_out, void* stream) {
  if (n && (!in || !spos || !vals_out)) return SHM_EINVAL;
  shm::dev::launch_route_gather(in, spos, n, vals_out, found_out, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? SHM_OK : SHM_EIO;
}

// (2) The routed path at world 1 (shm_shard::force_route): every call through
// the transport, RCCL sending each run to this rank itself
// (tests/test_gpu_shard.py [nccl-1-routed]), so ncclSend / ncclRecv run on a
// one-GPU box.
int shm__shard_force_route(shm_shard* h, int on) {
  if (!h) return SHM_EINVAL;
  h->force_route = on != 0;
  for (auto& x : h->xp)
    if (x) x->self_too = on != 0;
  return SHM_OK;
}

}  // extern "C"
