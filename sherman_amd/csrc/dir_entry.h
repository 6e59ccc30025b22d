// dir_entry.h — reading a leaf directory entry (leafdir.hip builds them,
// dir_upkeep.h keeps them): the start page of a key and the candidate slots
// of the entry's fingerprint and pair forms.
#pragma once
#include "device_common.h"

namespace shm {
namespace dev {

// leaf directory lookup (leafdir.hip): the start page for key k, `fallback`
// when k is outside the directory.  Entry p is 64 B (kDirWords u64), its
// first 32 B u32[8] = {pg0..pg3, t1..t3, count}: the leaves covering prefix
// p as page indices (GlobalAddress offset / 1 KB) and their split points
// t_i, the top 32 bits of (sep_i - lo_p) within the prefix (exact when the
// prefix spans <= 2^32 keys); count 0: pg0 is the deepest internal page
// covering the prefix.  count & kDirFp: ONE leaf covers the prefix and the
// entry carries a copy of its summary fingerprints (dir_fp_cand below) in
// place of pg1..pg3 / t1..t3 and in bytes 32..61.
// Leaf i is taken only when t_i < t(k), which proves k > sep_i; on a tie the
// walk starts one leaf to the left and moves right (B-link, Tree.cpp:626-629).
// k lies inside the directory's key range (and is not kKeyMax)
__device__ __forceinline__ bool dir_covers(uint64_t dir_lo, uint32_t dir_shift, uint64_t dir_n,
                                           uint64_t k) {
  return k >= dir_lo && ((k - dir_lo) >> dir_shift) < dir_n && k != kKeyMax;
}
__device__ __forceinline__ uint64_t dir_start(const uint64_t* dir, uint64_t dir_lo,
                                              uint32_t dir_shift, uint64_t dir_n,
                                              uint16_t node, uint64_t k, uint64_t fallback) {
  const uint64_t p = (k - dir_lo) >> dir_shift;
  if (k < dir_lo || p >= dir_n || k == kKeyMax) return fallback;
  const u32x4* e = reinterpret_cast<const u32x4*>(dir + kDirWords * p);
  const u32x4 e0 = e[0], e1 = e[1];
  const uint64_t off = (k - dir_lo) - (p << dir_shift);
  const bool exact = dir_shift <= 32;
  const uint32_t tk = exact ? (uint32_t)off : (uint32_t)(off >> (dir_shift - 32));
  const uint32_t cnt = e1.w & 0xFFu;
  auto past = [&](uint32_t t) { return t < tk || (exact && t == tk); };
  const uint32_t i = (uint32_t)(cnt > 1 && past(e1.x)) + (uint32_t)(cnt > 2 && past(e1.y)) +
                     (uint32_t)(cnt > 3 && past(e1.z));
  const uint32_t pg = i == 0 ? e0.x : i == 1 ? e0.y : i == 2 ? e0.z : e0.w;
  return dir_page_ga(pg, node);
}

// dir_start reading the whole 64 B entry into e (one request): *fpform when
// it is in fingerprint form (its one leaf returned, candidates by dir_fp_cand).
// alt (nullable), round 4: on a tie (k's top 32 offset bits equal leaf i's
// split point's) the leaf i itself is returned and *alt = the safe start one
// leaf to the left, else *alt = 0.  The split points are keys (each leaf's
// lowest fence), so a lookup of the first key of a leaf is exactly such a
// tie: 2.7 % of C2's gets started left and moved right (a summary and a
// header read more).  A caller that finds k in the returned leaf is done (a
// key lives in one leaf); one that does not must walk again from *alt (k may
// lie below leaf i's lowest fence, in leaf i - 1).
__device__ __forceinline__ uint64_t dir_start_e(const uint64_t* dir, uint64_t dir_lo,
                                                uint32_t dir_shift, uint64_t dir_n, uint16_t node,
                                                uint64_t k, uint64_t fallback, u32x4 (&e)[4],
                                                bool& fpform, uint64_t* alt = nullptr) {
  fpform = false;
  if (alt) *alt = 0;
  const uint64_t p = (k - dir_lo) >> dir_shift;
  if (k < dir_lo || p >= dir_n || k == kKeyMax) {
    // no entry: a zero one (count 0, no form flag), so the callers' pair /
    // fingerprint decoding of e[] sees no candidates
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = u32x4{0u, 0u, 0u, 0u};
    return fallback;
  }
  const u32x4* ep = reinterpret_cast<const u32x4*>(dir + kDirWords * p);
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] = ep[j];
  const uint64_t off = (k - dir_lo) - (p << dir_shift);
  const bool exact = dir_shift <= 32;
  const uint32_t tk = exact ? (uint32_t)off : (uint32_t)(off >> (dir_shift - 32));
  const uint32_t cnt = e[1].w & 0xFFu;
  fpform = (e[1].w & kDirFp) != 0;
  auto past = [&](uint32_t t) { return t < tk || (exact && t == tk); };
  const uint32_t i = fpform ? 0u
                            : (uint32_t)(cnt > 1 && past(e[1].x)) +
                                  (uint32_t)(cnt > 2 && past(e[1].y)) +
                                  (uint32_t)(cnt > 3 && past(e[1].z));
  auto page_of = [&](uint32_t j) {
    return j == 0 ? e[0].x : j == 1 ? e[0].y : j == 2 ? e[0].z : e[0].w;
  };
  if (alt && !fpform && !exact && i + 1 < cnt) {
    const uint32_t tn = i == 0 ? e[1].x : i == 1 ? e[1].y : e[1].z;  // leaf i + 1's split
    if (tn == tk) {
      *alt = dir_page_ga(page_of(i), node);
      return dir_page_ga(page_of(i + 1), node);
    }
  }
  return dir_page_ga(page_of(i), node);
}

// A directory entry in fingerprint form (count == 1 | kDirFp, layout.h):
// the candidate slots of its one leaf for key k, from the copy of the leaf's
// summary fingerprints taken when the directory was built: fp[s] at bytes
// 4..27 (s < 24) and 32..61 (s >= 24) of the entry.  The copy may be stale
// (the leaf got keys or split since): a candidate is only a slot to read,
// and a get that finds no valid entry with its key there walks the summary
// path (never a wrong answer, a stale copy only costs that fallback).
__device__ __forceinline__ uint64_t dir_fp_cand(const u32x4 (&e)[4], uint64_t k) {
  const uint32_t fq = key_fp(k);
  uint64_t cand = 0;
#pragma unroll
  for (int s = 0; s < kLeafCardinality; ++s) {
    const int b = s < 24 ? 4 + s : 8 + s;  // 24 fps at 4..27, 30 at 32..61
    const u32x4 v = e[b >> 4];
    const int d = (b >> 2) & 3;
    const uint32_t x = d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w;
    cand |= (uint64_t)(((x >> (8 * (b & 3))) & 0xFFu) == fq) << s;
  }
  return cand;
}

// A directory entry in pair form (layout.h kDirPairs): usable when its build
// finished clean (no kDirPairsBad, at most kDirPairMax pairs); the pairs
// whose fingerprint equals k's (bit j: pair j), each naming a slot of one of
// the entry's leaves (dir_pair_slot).  Like the fingerprint form's, a
// candidate is only a slot to read (a stale pair costs the summary walk).
__device__ __forceinline__ uint32_t dir_pair_cand(const u32x4 (&e)[4], uint64_t k, bool& usable) {
  const uint32_t cw = e[1].w;
  const uint32_t np = (cw >> 16) & 0xFFu;
  usable = (cw & kDirPairs) && !(cw & kDirPairsBad) && np <= kDirPairMax;
  if (!usable) return 0;
  const uint32_t fq = key_fp(k);
  const uint32_t w[8] = {e[2].x, e[2].y, e[2].z, e[2].w, e[3].x, e[3].y, e[3].z, e[3].w};
  uint32_t cand = 0;
#pragma unroll
  for (int j = 0; j < (int)kDirPairMax; ++j) {
    const uint32_t pr = (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
    cand |= (uint32_t)((uint32_t)j < np && (pr & 0xFFu) == fq) << j;
  }
  return cand;
}
// pair j's leaf (page index from the entry's list) and slot
__device__ __forceinline__ void dir_pair_slot(const u32x4 (&e)[4], int j, uint32_t& pg, int& slot) {
  const uint32_t w = (j < 8 ? (j < 4 ? (j < 2 ? e[2].x : e[2].y) : (j < 6 ? e[2].z : e[2].w))
                            : (j < 12 ? (j < 10 ? e[3].x : e[3].y) : (j < 14 ? e[3].z : e[3].w)));
  const uint32_t pr = (w >> (16 * (j & 1))) & 0xFFFFu;
  const uint32_t leaf = (pr >> 14) & 3u;
  slot = (int)((pr >> 8) & 63u);
  pg = leaf == 0 ? e[0].x : leaf == 1 ? e[0].y : leaf == 2 ? e[0].z : e[0].w;
}

}  // namespace dev
}  // namespace shm
