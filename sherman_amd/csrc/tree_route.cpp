// tree_route.cpp — routing and key utilities.
//
// The bucketing of a batch by owning shard (route_bucket behind the
// shm_route_bucket* calls, by hash or by splitters), the permutes that carry
// results back into input order, and the small stand-alone launches of the
// C-ABI: the lock-table benchmark and the key generators.  None of them reads
// the tree; they use the handle for its scratch, its error word and its call
// ordering.
#include "tree_internal.h"

extern "C" {

namespace {
// static: inside extern "C" an unnamed namespace alone leaves the name exported
static int route_bucket(shm_tree* t, const uint64_t* keys, uint64_t n, uint32_t num_shards,
                        const uint64_t* splitters, uint64_t* counts_out, uint64_t* keys_out,
                        uint32_t* perm_out, void* stream, bool reject_keymax, int mode = 0) {
  if (!t || num_shards == 0 || num_shards > 64 || !counts_out) return SHM_EINVAL;
  if (n && (!keys || !keys_out || !perm_out)) return SHM_EINVAL;
  // ascending (repeats make empty shards), none kKeyMax: checked on the host
  // words before the handle is used
  dev::RouteSplit sp{};
  if (splitters)
    for (uint32_t j = 0; j + 1 < num_shards; ++j) {
      if (splitters[j] == kKeyMax || (j && splitters[j] < splitters[j - 1])) return SHM_EINVAL;
      sp.s[j] = splitters[j];
    }
  if (n > t->nmax) return SHM_E2BIG;
  std::lock_guard<std::mutex> g(t->mu);
  hipStream_t s = pick(stream);
  Order ord(t, s, false);  // reads only the caller's keys; scratch per stream
  if (ord.rc) return ord.rc;
  uint32_t* scratch = nullptr;
  for (auto& r : t->route_ws)
    if (r.first == s) scratch = r.second;
  if (!scratch) {
    if (t->route_ws.empty()) {
      scratch = t->route_scratch;
    } else if (dalloc(&scratch, dev::route_scratch_words(t->nmax))) {
      return SHM_ENOMEM;
    }
    t->route_ws.push_back({s, scratch});
  }
  // d_err[3]: the kKeyMax flag of a routed insert (zero between calls)
  dev::launch_route_bucket(keys, n, num_shards, counts_out, keys_out, perm_out, scratch,
                           reject_keymax ? t->d_err + 3 : nullptr, t->d_err, s,
                           splitters ? &sp : nullptr, mode);
  HIP_OK(hipGetLastError());
  return SHM_OK;
}
}  // namespace

int shm_route_bucket(shm_tree* t, const uint64_t* keys, uint64_t n,
                     uint32_t num_shards, uint64_t* counts_out,
                     uint64_t* keys_out, uint32_t* perm_out, void* stream) {
  return route_bucket(t, keys, n, num_shards, nullptr, counts_out, keys_out, perm_out, stream,
                      false);
}

int shm_route_bucket_bounds(shm_tree* t, const uint64_t* keys, uint64_t n, uint32_t num_shards,
                            const uint64_t* splitters_host, uint64_t* counts_out,
                            uint64_t* keys_out, uint32_t* perm_out, void* stream) {
  return route_bucket(t, keys, n, num_shards, splitters_host, counts_out, keys_out, perm_out,
                      stream, false);
}

// Library-internal (shard.cpp shm_shard_insert): the bucketing of a routed
// insert; a batch holding kKeyMax is rejected whole on the sending rank
// (nothing routed, SHM_EINVAL at the next synchronising call), as a local
// insert rejects its chunk (the receivers skip kKeyMax as slot
// padding, so it must be caught before packing).  splitters_host: nullable,
// as shm_route_bucket_bounds
int shm__route_bucket_insert(shm_tree* t, const uint64_t* keys, uint64_t n, uint32_t num_shards,
                             const uint64_t* splitters_host, uint64_t* counts_out,
                             uint64_t* keys_out, uint32_t* perm_out, void* stream) {
  return route_bucket(t, keys, n, num_shards, splitters_host, counts_out, keys_out, perm_out,
                      stream, true);
}

// Library-internal (tools/route_bounds.py, tests): shm_route_bucket_bounds with
// the owner search named (kernels.h RouteSplit: 0 or 2 LDS, 1 kernel arguments)
int shm__route_bucket_mode(shm_tree* t, const uint64_t* keys, uint64_t n, uint32_t num_shards,
                           const uint64_t* splitters_host, int mode, uint64_t* counts_out,
                           uint64_t* keys_out, uint32_t* perm_out, void* stream) {
  return route_bucket(t, keys, n, num_shards, splitters_host, counts_out, keys_out, perm_out,
                      stream, false, mode);
}

int shm_route_permute(shm_tree* t, const uint64_t* in, const uint32_t* perm,
                      uint64_t n, uint64_t* out, void* stream) {
  if (!t || (n && (!in || !perm || !out))) return SHM_EINVAL;
  dev::launch_permute(in, perm, n, out, pick(stream));
  HIP_OK(hipGetLastError());
  return SHM_OK;
}

int shm_route_unpermute(shm_tree* t, const uint64_t* in, const uint32_t* perm,
                        uint64_t n, uint64_t* out, void* stream) {
  if (!t || (n && (!in || !perm || !out))) return SHM_EINVAL;
  dev::launch_unpermute(in, perm, n, out, nullptr, pick(stream));
  HIP_OK(hipGetLastError());
  return SHM_OK;
}

int shm_route_unpermute_found(shm_tree* t, const uint64_t* in, const uint32_t* perm,
                              uint64_t n, uint64_t* out, uint8_t* found_out, void* stream) {
  if (!t || (n && (!in || !perm || !out || !found_out))) return SHM_EINVAL;
  dev::launch_unpermute(in, perm, n, out, found_out, pick(stream));
  HIP_OK(hipGetLastError());
  return SHM_OK;
}

int shm_lock_bench(shm_tree* t, const uint64_t* keys, uint64_t n, void* stream) {
  if (!t || (n && !keys)) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  hipStream_t s = pick(stream);
  Order ord(t, s, true);  // the lock words: no chunk may hold them meanwhile
  if (ord.rc) return ord.rc;
  // the tag of the last chunk issued: every word is free for it once that
  // chunk has retired (stream order)
  dev::launch_lock_bench(keys, n, t->locks, t->cfg.num_locks, (uint64_t)t->chunks << 32, t->d_err,
                         s);
  HIP_OK(hipGetLastError());
  t->err_pending = true;
  return SHM_OK;
}

int shm_gen_keys(shm_tree* t, uint64_t first, uint64_t n, uint64_t keyspace,
                 uint64_t* keys_out, void* stream) {
  if (!t || (n && !keys_out)) return SHM_EINVAL;
  dev::launch_gen_keys(first, n, keyspace, keys_out, pick(stream));
  HIP_OK(hipGetLastError());
  return SHM_OK;
}

int shm_hash_keys(shm_tree* t, const uint64_t* ids, uint64_t n, uint64_t keyspace,
                  uint64_t* keys_out, void* stream) {
  if (!t || (n && (!ids || !keys_out))) return SHM_EINVAL;
  dev::launch_hash_ids(ids, n, keyspace, keys_out, pick(stream));
  HIP_OK(hipGetLastError());
  return SHM_OK;
}
}  // extern "C"
