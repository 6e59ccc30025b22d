// page_fields_test.cpp — the shared page readers of
// sherman_amd/csrc/page_fields.h against byte-wise reads at layout.h's
// offsets.  1 KB internal and leaf pages are written byte by byte, with field
// values whose eight bytes all differ (a reader that takes a byte from the
// wrong place, or in the wrong order, gives another number), for last_index
// -1, 0 and 60, level 0 and 7, versions 0 and 0xFF; records 0 and 60 are
// read back from the internal pages.  Expected values are memcpy reads at the
// byte offsets.  Pure host code: no GPU, no library.  `make -C tests/native
// sanitize` builds and runs it with the address and undefined-behaviour
// sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../../sherman_amd/csrc/page_fields.h"

using namespace shm;

static int fails = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++fails;                                              \
    }                                                       \
  } while (0)

struct alignas(16) Page {
  uint8_t b[kPageSize];
};

// eight different bytes, different for every seed below
static uint64_t distinct(uint8_t seed) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= (uint64_t)(uint8_t)(seed + 0x11 * i + 1) << (8 * i);
  return v;
}
static void put64(Page& p, int off, uint64_t v) {
  for (int i = 0; i < 8; ++i) p.b[off + i] = (uint8_t)(v >> (8 * i));
}
static uint64_t get64(const Page& p, int off) {
  uint64_t v;
  memcpy(&v, p.b + off, 8);  // the host is little-endian, like the device
  return v;
}
static int16_t get16(const Page& p, int off) {
  int16_t v;
  memcpy(&v, p.b + off, 2);
  return v;
}

struct Fields {
  uint64_t leftmost, sibling, lowest, highest;
  uint8_t level, fver, rver;
  int16_t last_index;
};

// every byte of the page is first set to a filler that no field holds, so a
// reader that strays off its field is seen
static void write_page(Page& p, const Fields& f, bool leaf) {
  memset(p.b, 0xEE, sizeof(p.b));
  put64(p, kOffLock, distinct(0xC0));
  p.b[kOffFrontVer] = f.fver;
  put64(p, kOffLeftmost, f.leftmost);
  put64(p, kOffSibling, f.sibling);
  p.b[kOffLevel] = f.level;
  p.b[kOffLastIndex] = (uint8_t)((uint16_t)f.last_index & 0xFF);
  p.b[kOffLastIndex + 1] = (uint8_t)((uint16_t)f.last_index >> 8);
  put64(p, kOffLowest, f.lowest);
  put64(p, kOffHighest, f.highest);
  if (!leaf) {
    for (int j = 0; j < kInternalCardinality; ++j) {
      put64(p, kOffRecords + kInternalEntry * j, distinct((uint8_t)(2 * j)));
      put64(p, kOffRecords + kInternalEntry * j + 8, distinct((uint8_t)(2 * j + 1)));
    }
  }
  // the rear byte of the page's kind: a leaf's other one (padding) gets
  // another value, an internal page's other one lies in record 60's pointer,
  // whose byte there is neither 0x5A nor 0xA5
  if (leaf) {
    p.b[kOffLeafRear] = f.rver;
    p.b[kOffInternalRear] = (uint8_t)~f.rver;
  } else {
    p.b[kOffInternalRear] = f.rver;
  }
}

static void check_page(const Page& p, const Fields& f, bool leaf) {
  const uint32_t* d = page_dw(p.b);
  // the expected values: bytes at layout.h's offsets
  const uint64_t leftmost = get64(p, kOffLeftmost), sibling = get64(p, kOffSibling);
  const uint64_t lowest = get64(p, kOffLowest), highest = get64(p, kOffHighest);
  const uint32_t level = p.b[kOffLevel], fver = p.b[kOffFrontVer];
  const int last = get16(p, kOffLastIndex);
  CHECK(leftmost == f.leftmost && sibling == f.sibling && last == f.last_index);

  const PageHdr h = read_hdr(d);
  CHECK(h.leftmost == leftmost);
  CHECK(h.sibling == sibling);
  CHECK(h.lowest == lowest);
  CHECK(h.highest == highest);
  CHECK(h.level == level);
  CHECK(h.last_index == last);
  CHECK(h.count() == last + 1);
  CHECK(h.fver == fver);
  CHECK(h.is_leaf() == leaf);
  // hdr_fields from the dwords by their names
  const PageHdr g = hdr_fields(d[kDwFrontVer], d[kDwLeftmost + 1], d[kDwSibling], d[kDwSibling + 1],
                               d[kDwLevel], d[kDwLowest], d[kDwLowest + 1], d[kDwHighest],
                               d[kDwHighest + 1]);
  CHECK(g.leftmost == leftmost && g.sibling == sibling && g.lowest == lowest &&
        g.highest == highest && g.level == level && g.last_index == last && g.fver == fver);
  // the single-field readers
  CHECK(hdr_leftmost(d) == leftmost);
  CHECK(hdr_sibling(d) == sibling);
  CHECK(hdr_lowest(d) == lowest);
  CHECK(hdr_highest(d) == highest);
  CHECK(hdr_level(d) == level);
  CHECK(hdr_last_index(d) == last);
  // u64_b1 and u64_at on their own
  CHECK(u64_b1(d[kDwLeftmost], d[kDwLeftmost + 1], d[kDwLeftmost + 2]) == leftmost);
  CHECK(u64_b1(d[kDwSibling], d[kDwSibling + 1], d[kDwSibling + 2]) == sibling);
  CHECK(u64_at(d, kDwLowest) == lowest && u64_at(d, kDwHighest) == highest);
  // the rear version of the page's kind: byte 0 of its dword
  CHECK((d[leaf ? kDwLeafRear : kDwInternalRear] & 0xFF) ==
        p.b[leaf ? kOffLeafRear : kOffInternalRear]);
  CHECK((d[leaf ? kDwLeafRear : kDwInternalRear] & 0xFF) == f.rver);
  if (!leaf) {
    for (int j : {0, 1, 59, kInternalCardinality - 1}) {
      CHECK(rec_key(d, j) == get64(p, kOffRecords + kInternalEntry * j));
      CHECK(rec_ptr(d, j) == get64(p, kOffRecords + kInternalEntry * j + 8));
      CHECK(4 * rec_key_dw(j) == kOffRecords + kInternalEntry * j);
      CHECK(4 * rec_ptr_dw(j) == kOffRecords + kInternalEntry * j + 8);
    }
    CHECK(rec_key(d, 0) == distinct(0) && rec_ptr(d, 0) == distinct(1));
    CHECK(rec_key(d, 60) == distinct(120) && rec_ptr(d, 60) == distinct(121));
  }
}

int main() {
  static_assert(kInternalCardinality - 1 == 60, "record 60 is the last");
  int pages = 0;
  Page p;
  for (int leaf = 0; leaf < 2; ++leaf)
    for (int16_t last : {(int16_t)-1, (int16_t)0, (int16_t)60})
      for (uint8_t level : {(uint8_t)0, (uint8_t)7})
        for (uint8_t ver : {(uint8_t)0, (uint8_t)0xFF}) {
          Fields f;
          f.leftmost = leaf ? 0 : distinct(0x20);
          f.sibling = distinct(0x30);
          f.lowest = distinct(0x40);
          f.highest = distinct(0x50);
          f.level = level;
          f.fver = ver;
          f.rver = (uint8_t)(ver ^ 0x5A);  // front and rear are told apart
          f.last_index = last;
          write_page(p, f, leaf != 0);
          check_page(p, f, leaf != 0);
          ++pages;
        }
  // a sibling of all ones and of zero beside non-zero neighbours: no bit of
  // the bytes around a field leaks into it
  for (uint64_t sib : {0ull, ~0ull}) {
    Fields f = {distinct(0x20), sib, distinct(0x40), distinct(0x50), 7, 0xFF, 0, 60};
    write_page(p, f, false);
    check_page(p, f, false);
    ++pages;
  }
  if (fails) {
    printf("page_fields_test: %d failures\n", fails);
    return 1;
  }
  printf("page_fields_test ok: %d pages\n", pages);
  return 0;
}
