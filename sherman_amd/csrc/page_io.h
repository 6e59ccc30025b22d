// page_io.h — a page's bytes on the device: whole pages as one 16 B slice per
// lane, and single fields and entries per lane.
//
// A 1 KB Sherman page is moved as ONE global_load_dwordx4 per lane: lane l
// holds bytes [16l, 16l+16) in a u32x4.  Header fields come out with
// v_readlane (they live in lanes 0..2 and 63; parse_hdr), internal records
// are lane aligned (record j = lane j+3 after a one-lane shift), and the
// 18-byte leaf entries (2-byte aligned) are staged through a per-wave 1 KB LDS
// slot.  A lane that walks alone reads single entries straight from global
// memory (entry_load / entry_decode).  Which dword holds which field is
// page_fields.h's.
#pragma once
#include "device_common.h"
#include "page_fields.h"

namespace shm {
namespace dev {

__device__ __forceinline__ u32x4 load_page_slice(const uint8_t* arena,
                                                  uint64_t off) {
  return *reinterpret_cast<const u32x4*>(arena + off + 16 * lane_id());
}

// Header (page_fields.h) + both rear versions, wave-uniform: dword d of the
// page is component d & 3 of lane d >> 2's slice.
struct Hdr : PageHdr {
  uint32_t rver_internal, rver_leaf;
};
template <int D>
__device__ __forceinline__ uint32_t slice_dw(const u32x4 w) {
  constexpr int c = D & 3;
  return rl32(c == 0 ? w.x : c == 1 ? w.y : c == 2 ? w.z : w.w, D >> 2);
}
__device__ __forceinline__ Hdr parse_hdr(const u32x4 w) {
  const uint32_t d2 = slice_dw<2>(w), d3 = slice_dw<3>(w), d4 = slice_dw<4>(w),
                 d5 = slice_dw<5>(w), d6 = slice_dw<6>(w), d7 = slice_dw<7>(w),
                 d8 = slice_dw<8>(w), d9 = slice_dw<9>(w), d10 = slice_dw<10>(w);
  const uint32_t zl = slice_dw<kDwLeafRear>(w), zi = slice_dw<kDwInternalRear>(w);
  Hdr h;
  static_cast<PageHdr&>(h) = hdr_fields(d2, d3, d4, d5, d6, d7, d8, d9, d10);
  h.rver_internal = zi & 0xFF;
  h.rver_leaf = zl & 0xFF;
  return h;
}

// both rear versions' dwords of a page (or an LDS slot) with one 8 B load
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x2 rear_dwords(const uint32_t* p) {
  return *reinterpret_cast<const u32x2*>(p + kDwLeafRear);
}

// Internal record j = lane - 3 (Tree.h:163-172): key straddles lanes j+2/j+3.
struct IntRec {
  uint64_t key, ptr;
};
__device__ __forceinline__ IntRec internal_record(const u32x4 w) {
  const uint32_t prev_w3 = (uint32_t)__shfl_up((int)w.w, 1);
  IntRec r;
  r.key = ((uint64_t)w.x << 32) | prev_w3;
  r.ptr = (uint64_t)w.y | ((uint64_t)w.z << 32);
  return r;
}

// Leaf entry i = lane (Tree.h:174-187), read from the wave's LDS page image.
struct LeafEnt {
  uint64_t key, val;
  uint32_t fraw, rraw;  // full bytes; versions are the low nibbles
};
__device__ __forceinline__ void stage_page(uint32_t* lp, const u32x4 w) {
  *reinterpret_cast<u32x4*>(lp + 4 * lane_id()) = w;
}
// An 18 B entry's fields from its own five dwords (q0's byte 0 is the entry's
// byte 0; the funnel shift that aligns them is the caller's): f, key, value
// and r at bytes 0, 1, 9 and 17 (Tree.h:174-187).  The one decode of a single
// entry (leaf_chunk.h unpacks a lane's chunk with compile-time offsets).
__device__ __forceinline__ void leaf_fields(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3,
                                            uint32_t q4, uint64_t& key, uint64_t& val,
                                            uint32_t& f, uint32_t& r) {
  f = q0 & 0xFF;
  key = u64_b1(q0, q1, q2);
  val = u64_b1(q2, q3, q4);
  r = (q4 >> 8) & 0xFF;
}
__device__ __forceinline__ LeafEnt leaf_entry(const uint32_t* lp, int i) {
  const int s = kOffRecords + kLeafEntry * i;
  const int d = s >> 2;
  const uint32_t sh = (uint32_t)(s & 3);
  const uint32_t a0 = lp[d], a1 = lp[d + 1], a2 = lp[d + 2], a3 = lp[d + 3],
                 a4 = lp[d + 4];
  LeafEnt e;
  leaf_fields(__builtin_amdgcn_alignbyte(a1, a0, sh), __builtin_amdgcn_alignbyte(a2, a1, sh),
              __builtin_amdgcn_alignbyte(a3, a2, sh), __builtin_amdgcn_alignbyte(a4, a3, sh),
              __builtin_amdgcn_alignbyte(0u, a4, sh), e.key, e.val, e.fraw, e.rraw);
  return e;
}
// write an 18 B entry at its 2-byte aligned slot: an even slot starts on a
// dword (4 dword stores + 1 halfword), an odd one 2 bytes past (1 halfword +
// 4 dword stores)
__device__ __forceinline__ void put_leaf_entry(uint32_t* lp, int i,
                                               uint64_t key, uint64_t val,
                                               uint32_t fraw, uint32_t rraw) {
  uint8_t* b = reinterpret_cast<uint8_t*>(lp) + kOffRecords + kLeafEntry * i;
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  const uint32_t v0 = (uint32_t)val, v1 = (uint32_t)(val >> 32);
  const uint32_t f = fraw & 0xFF, r = rraw & 0xFF;
  if ((i & 1) == 0) {  // f k0..k2 | k3..k6 | k7 v0..v2 | v3..v6 | v7 r
    uint32_t* d = reinterpret_cast<uint32_t*>(b);
    d[0] = f | (k0 << 8);
    d[1] = (k0 >> 24) | (k1 << 8);
    d[2] = (k1 >> 24) | (v0 << 8);
    d[3] = (v0 >> 24) | (v1 << 8);
    *reinterpret_cast<uint16_t*>(b + 16) = (uint16_t)((v1 >> 24) | (r << 8));
  } else {  // f k0 | k1..k4 | k5..k7 v0 | v1..v4 | v5..v7 r
    *reinterpret_cast<uint16_t*>(b) = (uint16_t)(f | ((k0 & 0xFF) << 8));
    uint32_t* d = reinterpret_cast<uint32_t*>(b + 2);
    d[0] = (k0 >> 8) | (k1 << 24);
    d[1] = (k1 >> 8) | (v0 << 24);
    d[2] = (v0 >> 8) | (v1 << 24);
    d[3] = (v1 >> 8) | (r << 24);
  }
}

// Header dword d (0..10) of a page image (bytes 0..43); lock word = 0.
__device__ __forceinline__ uint32_t header_dword(int d, uint32_t fver,
                                                 uint64_t leftmost,
                                                 uint64_t sibling,
                                                 uint32_t level,
                                                 int32_t last_index,
                                                 uint64_t lowest,
                                                 uint64_t highest) {
  switch (d) {
    case 2: return (fver & 0xFF) | (uint32_t)((leftmost & 0xFFFFFF) << 8);
    case 3: return (uint32_t)(leftmost >> 24);
    case 4: return (uint32_t)(leftmost >> 56) | (uint32_t)((sibling & 0xFFFFFF) << 8);
    case 5: return (uint32_t)(sibling >> 24);
    case 6:
      return (uint32_t)(sibling >> 56) | ((level & 0xFF) << 8) |
             ((uint32_t)(last_index & 0xFFFF) << 16);
    case 7: return (uint32_t)lowest;
    case 8: return (uint32_t)(lowest >> 32);
    case 9: return (uint32_t)highest;
    case 10: return (uint32_t)(highest >> 32);
    default: return 0;
  }
}

// zero the slot and write a fresh header (all lanes call)
__device__ __forceinline__ void init_page_image(uint32_t* lp, uint32_t fver,
                                                uint64_t leftmost,
                                                uint64_t sibling,
                                                uint32_t level,
                                                int32_t last_index,
                                                uint64_t lowest,
                                                uint64_t highest) {
  const int l = lane_id();
  *reinterpret_cast<u32x4*>(lp + 4 * l) = u32x4{0, 0, 0, 0};
  wave_lds_sync();
  if (l < 11)
    lp[l] = header_dword(l, fver, leftmost, sibling, level, last_index, lowest,
                         highest);
}

__device__ __forceinline__ void store_page(uint8_t* arena, uint64_t off,
                                           const uint32_t* lp) {
  wave_lds_sync();
  const u32x4 w = *reinterpret_cast<const u32x4*>(lp + 4 * lane_id());
  *reinterpret_cast<u32x4*>(arena + off + 16 * lane_id()) = w;
}

// ---- per-lane leaf access (the summary walk, the update matcher) --------------

// Leaf entry s of a page (18 B at 44 + 18 s, 2-byte aligned) in two halves,
// so several entries (and a summary line) can be requested before any is
// decoded: the raw dwords of entry s, then its fields
struct RawEntry {
  uint32_t d[5];
  uint32_t sh;
};
__device__ __forceinline__ void entry_load(const uint8_t* page, int s, RawEntry& r) {
  const uint32_t off = (uint32_t)(kOffRecords + kLeafEntry * s);
  const uint32_t* d = reinterpret_cast<const uint32_t*>(page + (off & ~3u));
#pragma unroll
  for (int j = 0; j < 5; ++j) r.d[j] = d[j];
  r.sh = off & 3u;  // 0 or 2
}
__device__ __forceinline__ void entry_decode(const RawEntry& e, uint64_t& key, uint64_t& val,
                                             uint32_t& f, uint32_t& r) {
  leaf_fields(__builtin_amdgcn_alignbyte(e.d[1], e.d[0], e.sh),
              __builtin_amdgcn_alignbyte(e.d[2], e.d[1], e.sh),
              __builtin_amdgcn_alignbyte(e.d[3], e.d[2], e.sh),
              __builtin_amdgcn_alignbyte(e.d[4], e.d[3], e.sh), e.d[4] >> (8 * e.sh), key, val, f,
              r);
}
// ... and both at once
__device__ __forceinline__ void lane_entry(const uint8_t* page, int s, uint64_t& key,
                                           uint64_t& val, uint32_t& f, uint32_t& r) {
  RawEntry e;
  entry_load(page, s, e);
  entry_decode(e, key, val, f, r);
}

__device__ __forceinline__ bool entry_hit(uint64_t key, uint64_t val, uint32_t f, uint32_t r,
                                          uint64_t k) {
  return key == k && val != kValueNull && ((f ^ r) & 0xF) == 0;
}

// a page's sibling pointer from its header (one 16 B load): the right turn
// of a summary walk
__device__ __forceinline__ uint64_t page_sibling(const uint8_t* page) {
  const u32x4 B = *reinterpret_cast<const u32x4*>(page + 4 * kDwSibling);
  return u64_b1(B.x, B.y, B.z);
}

}  // namespace dev
}  // namespace shm
