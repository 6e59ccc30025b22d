// valtab.h — the key-value bucket table a read phase's get reads first
// (DESIGN §3.1 "The bucket table").
//
// A bucket is one 128 B line, 128 B-aligned: 8 slots of (key u64, value u64),
// slot j at words 2j (key) and 2j + 1 (value).  Bucket b covers the keys
// [lo + (b << shift), lo + ((b + 1) << shift)) of the shard's range, half as
// many buckets as the read phase's directory has entries, so one random line
// answers a get whose bucket holds at most 8 keys.  The table is independent
// of the leaves (a split never touches it) and of the directory's entry
// format; it is trusted exactly while the directory is exact (tree.cpp).
//
// Slot states:
//   live         value != 0 (and its key word holds the key)
//   free         key word == 0 and value == 0: never used, or deleted (a
//                delete clears the value, then the key word)
//   dead bucket  key[0] == kKeyMax (never stored, never queried): more keys
//                than slots; its gets take the directory path.  A dead bucket
//                stays dead until the next build, whatever else the same
//                launch writes to it.
// Key 0 (kKeyMin) is the free slots' key word, so it never uses the table:
// vt_bucket_of refuses it and its gets take the directory path.
//
// Writers run lane = op, many lanes of one launch possibly in one bucket, a
// launch's ops unique by key, no get beside them (a chunk is exclusive).
// Every word is read and written with device-scope atomics: the lanes run on
// several XCDs, each with its own L2.
//
// Why the protocol is closed.  A key word changes only in three ways: 0 -> k
// by the one op of the launch that carries k (a compare-and-swap, so one
// claimant per slot), k -> 0 by the one op that deletes k (after it cleared
// the value), and key[0] -> kKeyMax by an exchange.  A slot's key word is
// claimed BEFORE its value becomes non-zero, so a slot never shows another
// op's key beside a claimant's value, and a key word equal to k is, for the
// op that carries k, always k's own live slot of before the launch: no other
// op of the launch writes k anywhere.  Neither compare-and-swap expects
// kKeyMax, so a marker is never overwritten.  (Claiming by the value word
// first, with the key written after it, let a second op match the stale key
// of a tombstone under the claimant's value: a wrong value in a live bucket.)
#pragma once
#include "device_common.h"
#include "kernels.h"

namespace shm {
namespace dev {

constexpr int kVtDead = -2, kVtAbsent = -1;
constexpr uint64_t kVtFreeKey = 0;

__host__ __device__ __forceinline__ bool vt_bucket_of(uint64_t lo, uint32_t shift, uint64_t n,
                                                      uint64_t k, uint64_t* b) {
  if (k < lo || k == kKeyMax || k == kVtFreeKey) return false;
  const uint64_t p = (k - lo) >> shift;
  *b = p;
  return p < n;
}

// The probe's per-slot predicates (w: one slot as key lo, key hi, value lo,
// value hi), shared by the lane that loads a whole bucket (vt_probe) and the
// eight lanes that load one slot each (get_sum.hip's cooperative probe).
// slot 0 carries the dead marker
__device__ __forceinline__ bool vt_slot_dead(const u32x4& w) {
  return (w.x & w.y) == 0xFFFFFFFFu;
}
// a live slot holding k; *sv = the slot's value either way
__device__ __forceinline__ bool vt_slot_match(const u32x4& w, uint64_t k, uint64_t* sv) {
  const uint64_t sk = (uint64_t)w.x | ((uint64_t)w.y << 32);
  *sv = (uint64_t)w.z | ((uint64_t)w.w << 32);
  return sk == k && *sv != kValueNull;
}

// the get's probe of a bucket it loaded whole (w: 8 slots): the dead marker
// first, then the highest live slot holding k
__device__ __forceinline__ int vt_probe(const u32x4 (&w)[kVtSlots], uint64_t k, uint64_t* val) {
  if (vt_slot_dead(w[0])) return kVtDead;
  int r = kVtAbsent;
#pragma unroll
  for (int j = 0; j < kVtSlots; ++j) {
    uint64_t sv;
    if (vt_slot_match(w[j], k, &sv)) {
      *val = sv;
      r = j;
    }
  }
  return r;
}

__device__ __forceinline__ uint64_t vt_ld(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void vt_st(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the key word's compare-and-swap: release (a delete's cleared value is
// visible before its freed key word) and acquire (a claimant's value store
// follows the delete's)
__device__ __forceinline__ bool vt_cas_key(uint64_t* p, uint64_t expect, uint64_t v) {
  return __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
}

// what a writer did with its key
enum VtPut { kVtStored = 0, kVtInDead = 1, kVtKilled = 2 };

// (k, v != 0) into bucket bk (k passed vt_bucket_of).  The slot whose key
// word is k is k's live slot: it takes the value.  Otherwise a free slot is
// claimed by compare-and-swap on its key word (0 -> k, lowest first; a lost
// claim moves on to the next free slot) and then takes the value.  No free
// slot: the bucket dies (kVtKilled for the one lane whose exchange set the
// marker over 8 claimed slots, kVtInDead for every other key that ends in a
// dead bucket and is not among those 8).
__device__ __forceinline__ VtPut vt_upsert(uint64_t* bk, uint64_t k, uint64_t v) {
  uint64_t key[kVtSlots];
#pragma unroll
  for (int j = 0; j < kVtSlots; ++j) key[j] = vt_ld(bk + 2 * j);
  if (key[0] == kKeyMax) return kVtInDead;
#pragma unroll
  for (int j = 0; j < kVtSlots; ++j)
    if (key[j] == k) {
      vt_st(bk + 2 * j + 1, v);
      return kVtStored;
    }
  // one compare-and-swap site for the whole wave (each carries a device-scope
  // release and acquire, the expensive part): a lane tries its lowest free
  // slot per round
  uint32_t freem = 0;
#pragma unroll
  for (int j = 0; j < kVtSlots; ++j) freem |= key[j] == kVtFreeKey ? 1u << j : 0u;
  while (freem) {
    const int j = __builtin_ctz(freem);
    freem &= freem - 1;
    if (!vt_cas_key(bk + 2 * j, kVtFreeKey, k)) continue;  // another lane's claim, or the marker
    vt_st(bk + 2 * j + 1, v);
    return kVtStored;
  }
  const uint64_t was = (uint64_t)atomicExch(reinterpret_cast<unsigned long long*>(bk),
                                            (unsigned long long)kKeyMax);
  return was == kKeyMax ? kVtInDead : kVtKilled;
}

// Tree::del for the table: k's slot loses its value, then its key word (by
// compare-and-swap: a marker that landed on slot 0 in between stays)
__device__ __forceinline__ void vt_delete(uint64_t* bk, uint64_t k) {
  if (vt_ld(bk) == kKeyMax) return;
  int at = -1;  // (k sits in at most one slot; one compare-and-swap site)
#pragma unroll
  for (int j = 1; j < kVtSlots; ++j) at = vt_ld(bk + 2 * j) == k ? j : at;
  at = vt_ld(bk) == k ? 0 : at;
  if (at < 0) return;
  vt_st(bk + 2 * at + 1, kValueNull);
  (void)vt_cas_key(bk + 2 * at, k, kVtFreeKey);
}

}  // namespace dev
}  // namespace shm
