// sum_line.h — a leaf's summary line (layout.h): written by every leaf
// writer, read by the gets and the upsert locate.
#pragma once
#include "device_common.h"

namespace shm {
namespace dev {

// A leaf's summary line (layout.h) from one wave: lane s < 54 gives slot
// s's fingerprint (0 = empty), lane 0 the highest fence; the tag byte last.
__device__ __forceinline__ void put_leaf_sum(uint8_t* sum, uint64_t page_off, uint64_t highest,
                                             uint32_t fp) {
  if (!sum) return;
  uint8_t* line = sum + (page_off >> 10) * kSumBytes;
  const int lane = lane_id();
  if (lane < kLeafCardinality) line[kSumOffFp + lane] = (uint8_t)fp;
  if (lane == 0) {
    *reinterpret_cast<uint64_t*>(line + kSumOffHighest) = highest;
    line[kSumOffTag] = kSumLeaf;
  }
}
// mark a page's line as not describing a leaf
__device__ __forceinline__ void clear_leaf_sum(uint8_t* sum, uint64_t page_off) {
  if (sum) sum[(page_off >> 10) * kSumBytes + kSumOffTag] = 0;
}
// clear slot s's fingerprint (the slot became empty)
__device__ __forceinline__ void clear_leaf_fp(uint8_t* sum, uint64_t page_off, int s) {
  if (sum) sum[(page_off >> 10) * kSumBytes + kSumOffFp + s] = 0;
}
// set slot s's fingerprint (a new key took the slot)
__device__ __forceinline__ void set_leaf_fp(uint8_t* sum, uint64_t page_off, int s, uint64_t k) {
  if (sum) sum[(page_off >> 10) * kSumBytes + kSumOffFp + s] = (uint8_t)key_fp(k);
}

// A leaf's summary line read whole (one 128 B request): false if it does not
// describe a current leaf; else its highest fence, sibling and the slots
// whose 8-bit fingerprint equals k's (bit s for slot s)
struct SumLine {
  uint64_t highest, cand;
};
__device__ __forceinline__ void sum_load(const uint8_t* sum, uint64_t page_off, u32x4 (&l)[4]) {
  const u32x4* line = reinterpret_cast<const u32x4*>(sum + (page_off >> 10) * kSumBytes);
#pragma unroll
  for (int j = 0; j < 4; ++j) l[j] = line[j];
}
__device__ __forceinline__ bool sum_decode(const u32x4 (&l)[4], uint64_t k, SumLine& o) {
  if ((l[0].z & 0xFF) != kSumLeaf) return false;
  o.highest = (uint64_t)l[0].x | ((uint64_t)l[0].y << 32);
  const uint32_t fq = key_fp(k);
  uint64_t cand = 0;
#pragma unroll
  for (int s = 0; s < kLeafCardinality; ++s) {  // byte 9 + s of the line
    const int b = (int)kSumOffFp + s;
    const u32x4 v = l[b >> 4];
    const int d = (b >> 2) & 3;
    const uint32_t x = d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w;
    cand |= (uint64_t)(((x >> (8 * (b & 3))) & 0xFFu) == fq) << s;
  }
  o.cand = cand;
  return true;
}
__device__ __forceinline__ bool sum_read(const uint8_t* sum, uint64_t page_off, uint64_t k,
                                         SumLine& o) {
  u32x4 l[4];
  sum_load(sum, page_off, l);
  return sum_decode(l, k, o);
}

}  // namespace dev
}  // namespace shm
