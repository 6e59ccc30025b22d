// page_fields.h — the reference page's fields as dwords: the one place that
// turns layout.h's byte offsets into what a kernel (or the host) reads from a
// page held as uint32_t[256], in global memory, in LDS or in registers.
//
// The header's two pointers start at byte 1 of a dword (front_version takes
// byte 0 of dword 2), so each spans three dwords (u64_b1); level and
// last_index share dword 6 with the sibling pointer's last byte; the fences
// and the internal records are dword aligned (u64_at).  The 18 B leaf entries
// are 2-byte aligned and have readers of their own (leaf_chunk.h for a lane's
// chunk of a staged page, page_io.h's leaf_fields for one entry).
//
// Host and device, plain C++: tests/native/page_fields_test.cpp checks every
// reader here against byte-wise reads at layout.h's offsets.
#pragma once
#include "layout.h"

namespace shm {

constexpr int kDwFrontVer = kOffFrontVer / 4;          // byte 0: front_version
constexpr int kDwLeftmost = kOffLeftmost / 4;          // from byte 1, three dwords
constexpr int kDwSibling = kOffSibling / 4;            // from byte 1, three dwords
constexpr int kDwLevel = kOffLevel / 4;                // byte 1: level, bytes 2..3: last_index
constexpr int kDwLowest = kOffLowest / 4;
constexpr int kDwHighest = kOffHighest / 4;
constexpr int kDwRecords = kOffRecords / 4;            // the header is dwords [0, kDwRecords)
constexpr int kDwLeafRear = kOffLeafRear / 4;          // byte 0: a leaf's rear_version
constexpr int kDwInternalRear = kOffInternalRear / 4;  // byte 0: an internal page's
constexpr int kRecDwords = kInternalEntry / 4;         // {key, ptr}
static_assert(kOffFrontVer % 4 == 0 && kOffLeftmost == kOffFrontVer + 1, "front_version, leftmost");
static_assert(kOffSibling % 4 == 1 && kOffSibling == kOffLeftmost + 8, "sibling from byte 1");
static_assert(kOffLevel == kOffSibling + 8 && kOffLastIndex == kOffLevel + 1 &&
                  kOffLastIndex % 4 == 2,
              "level and last_index in the sibling's last dword");
static_assert(kOffLowest % 4 == 0 && kOffHighest == kOffLowest + 8 &&
                  kOffRecords == kOffHighest + 8,
              "dword aligned fences, then the records");
static_assert(kDwInternalRear == kDwLeafRear + 1, "one 8 B read takes both rear versions");
static_assert(kInternalEntry == 16 && kOffLeafRear % 4 == 0 && kOffInternalRear % 4 == 0,
              "dword aligned records and rear versions");

// record j of an internal page: its key's and its pointer's first dword
SHM_HD constexpr int rec_key_dw(int j) { return kDwRecords + kRecDwords * j; }
SHM_HD constexpr int rec_ptr_dw(int j) { return kDwRecords + kRecDwords * j + 2; }

// a page (1 KB aligned in its arena) as dwords
SHM_HD const uint32_t* page_dw(const uint8_t* page) {
  return reinterpret_cast<const uint32_t*>(page);
}

// the u64 that starts at byte 1 of dword a and ends with byte 0 of dword c
SHM_HD uint64_t u64_b1(uint32_t a, uint32_t b, uint32_t c) {
  return (uint64_t)((a >> 8) | (b << 24)) | ((uint64_t)((b >> 8) | (c << 24)) << 32);
}
SHM_HD uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }
// the dword aligned u64 at dword d of p
SHM_HD uint64_t u64_at(const uint32_t* p, int d) { return u64_of(p[d], p[d + 1]); }

// Header (Tree.h:130-160) and front version
struct PageHdr {
  uint64_t leftmost, sibling, lowest, highest;
  uint32_t level;
  int32_t last_index;
  uint32_t fver;
  SHM_HD int count() const { return last_index + 1; }  // records / entries in use
  SHM_HD bool is_leaf() const { return leftmost == 0; }
};
// from dwords kDwFrontVer .. kDwRecords - 1 (2 .. 10), however they were read
SHM_HD PageHdr hdr_fields(uint32_t d2, uint32_t d3, uint32_t d4, uint32_t d5, uint32_t d6,
                          uint32_t d7, uint32_t d8, uint32_t d9, uint32_t d10) {
  PageHdr h;
  h.fver = d2 & 0xFF;
  h.leftmost = u64_b1(d2, d3, d4);
  h.sibling = u64_b1(d4, d5, d6);
  h.level = (d6 >> 8) & 0xFF;
  h.last_index = (int32_t)(int16_t)(d6 >> 16);
  h.lowest = u64_of(d7, d8);
  h.highest = u64_of(d9, d10);
  return h;
}
// one lane (or the host) reading a page's header, dword by dword
SHM_HD PageHdr read_hdr(const uint32_t* p) {
  return hdr_fields(p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10]);
}
static_assert(kDwFrontVer == 2 && kDwRecords == 11, "hdr_fields takes dwords 2..10");

// single fields, for a reader that needs no more
SHM_HD uint64_t hdr_leftmost(const uint32_t* p) {
  return u64_b1(p[kDwLeftmost], p[kDwLeftmost + 1], p[kDwLeftmost + 2]);
}
SHM_HD uint64_t hdr_sibling(const uint32_t* p) {
  return u64_b1(p[kDwSibling], p[kDwSibling + 1], p[kDwSibling + 2]);
}
SHM_HD uint32_t hdr_level(const uint32_t* p) { return (p[kDwLevel] >> 8) & 0xFF; }
SHM_HD int hdr_last_index(const uint32_t* p) { return (int)(int16_t)(p[kDwLevel] >> 16); }
SHM_HD uint64_t hdr_lowest(const uint32_t* p) { return u64_at(p, kDwLowest); }
SHM_HD uint64_t hdr_highest(const uint32_t* p) { return u64_at(p, kDwHighest); }

// internal record j (Tree.h:163-172)
SHM_HD uint64_t rec_key(const uint32_t* p, int j) { return u64_at(p, rec_key_dw(j)); }
SHM_HD uint64_t rec_ptr(const uint32_t* p, int j) { return u64_at(p, rec_ptr_dw(j)); }

}  // namespace shm
