// device_common.h — wave64 helpers for gfx950: lane primitives, the look-back
// index, the pointer check, the shard-range ordering key and the in-wave sort.
// A page's bytes are page_io.h's, a directory entry's dir_entry.h's, a
// summary line's sum_line.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.h"

namespace shm {
namespace dev {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;
constexpr int kBlock = 256;  // 4 waves per workgroup
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kPageDwords = 256;
constexpr int kMaxRounds = 4096;   // walk rounds per wave before giving up
constexpr int kMaxRetries = 1000;  // version-mismatch re-reads (Tree.cpp:600)
constexpr uint32_t kMaxLockSpins = 1u << 22;

__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }
__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ uint32_t rl32(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ uint64_t rl64(uint64_t v, int l) {
  return (uint64_t)rl32((uint32_t)v, l) |
         ((uint64_t)rl32((uint32_t)(v >> 32), l) << 32);
}
__device__ __forceinline__ int ctz64(uint64_t m) { return __builtin_ctzll(m); }
__device__ __forceinline__ int popc64(uint64_t m) { return __popcll(m); }
__device__ __forceinline__ uint32_t shfl32(uint32_t v, int src) {
  return (uint32_t)__shfl((int)v, src);
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  return (uint64_t)shfl32((uint32_t)v, src) |
         ((uint64_t)shfl32((uint32_t)(v >> 32), src) << 32);
}
__device__ __forceinline__ uint64_t lanemask_lt() {
  const int l = lane_id();
  return l == 0 ? 0ull : (~0ull >> (64 - l));
}
// order this wave's LDS traffic (LDS executes in order per wave; this keeps
// the compiler from moving accesses across and drains the counter)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// A block's index in a decoupled look-back launch (k_bin_unique, k_seg_fill,
// k_scan_u64), taken by one atomic add as the block starts: a block waits
// only on smaller indices, which blocks already running (or done) hold, so
// the look-back cannot wait on a block the dispatcher has not placed.  With
// blockIdx it could: another kernel or another process on the card may hold
// the CUs a smaller blockIdx needs while larger ones spin (seen with two
// ranks sharing one GPU: k_bin_unique's spin bound, kErrBinSpin).  The
// launch's last taker resets the counter for the next launch of the kernel
// (launches sharing a counter are stream-ordered).  Either every block of a
// launch calls this or none does (an exit taken before it must be uniform
// over the grid); ctr == nullptr keeps blockIdx.
__device__ __forceinline__ uint32_t lookback_index(uint32_t* ctr) {
  if (!ctr) return blockIdx.x;
  __shared__ uint32_t s_idx;
  if (threadIdx.x == 0) {
    const uint32_t i = atomicAdd(ctr, 1u);
    if (i == gridDim.x - 1) atomicExch(ctr, 0u);
    s_idx = i;
  }
  __syncthreads();
  return s_idx;
}

__device__ __forceinline__ bool ptr_ok(uint64_t ga, uint16_t node,
                                       uint64_t arena_bytes) {
  const uint64_t off = ga_offset(ga);
  return ga != 0 && ga_node(ga) == node && (off & (kPageSize - 1)) == 0 &&
         off >= kPageSize && off + kPageSize <= arena_bytes;
}

// a key's offset in the shard range [lo, lo + 2^bits), scaled to 64 bits
// (clamped outside the range): the ordering key of both passes
struct KeyRange {
  uint64_t lo;
  uint32_t bits;
};
__device__ __forceinline__ uint64_t rel_key(uint64_t k, KeyRange r) {
  if (r.bits >= 64) return k;
  if (k < r.lo) return 0;
  const uint64_t d = k - r.lo;
  return (d >> r.bits) ? ~0ull : d << (64 - r.bits);
}
__device__ __forceinline__ uint32_t coarse_of(uint64_t k, KeyRange r) {
  return (uint32_t)(rel_key(k, r) >> 56);
}
__device__ __forceinline__ uint32_t fine_of(uint64_t k, KeyRange r) {
  return (uint32_t)(rel_key(k, r) >> 48) & 0xFF;
}

// in-wave ascending bitonic sort of (key, tag) over 64 lanes; branch-free
// compare-exchange (xor shuffles with constant masks)
__device__ __forceinline__ void wave_sort64(uint64_t& key, uint32_t& tag) {
  const int l = lane_id();
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint64_t pk = (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)key, j) |
                          ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), j) << 32);
      const uint32_t pt = (uint32_t)__shfl_xor((int)tag, j);
      // keep the smaller key iff this lane is the lower one of an ascending
      // pair or the upper one of a descending pair
      const uint32_t want_min = (uint32_t)(((l & k) == 0) == ((l & j) == 0));
      const uint32_t take = (want_min & (uint32_t)(pk < key)) |
                            ((want_min ^ 1u) & (uint32_t)(pk > key));
      key = take ? pk : key;
      tag = take ? pt : tag;
    }
  }
}

// lower_bound over a sorted global u64 array [lo, hi)
__device__ __forceinline__ uint64_t lower_bound64(const uint64_t* a,
                                                  uint64_t lo, uint64_t hi,
                                                  uint64_t k) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (a[mid] < k)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace dev
}  // namespace shm
