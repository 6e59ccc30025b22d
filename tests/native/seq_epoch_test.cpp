// seq_epoch_test.cpp — the host arithmetic behind the counters' periods
// (sherman_amd/csrc/seq_epoch.h) against step-by-step models of the real
// streams: a jump of the chunk counter or the scan counter must report exactly
// the clears that issuing every skipped chunk or scan would have performed,
// and leave the counter where that stream would have left it.  Pure host
// code: no GPU, no library.  `make -C tests/native sanitize` builds and runs
// it with the address and undefined-behaviour sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../sherman_amd/csrc/seq_epoch.h"

using namespace shm::seq;

static int fails = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++fails;                                              \
    }                                                       \
  } while (0)

// insert_begin / insert_apply, one chunk: the tag it gets and the clears its
// apply makes (tree_insert.cpp: new_mark(tag) == 1, the fan tag's low 29 bits zero)
struct ChunkModel {
  uint32_t chunks;
  bool marks = false, fan = false, epoch = false;
  void step() {
    if (chunks == 0xFFFFFFFFu) {  // epoch_reset
      chunks = 0;
      epoch = true;
    }
    const uint32_t tag = ++chunks;
    if ((uint8_t)(tag % 255u + 1u) == 1) marks = true;
    if ((uint32_t)((uint64_t)tag << 3) == 0) fan = true;
  }
};

// scan_tag, one scan
struct ScanModel {
  uint32_t seq;
  bool clear = false;
  uint32_t step() {
    uint32_t tag = ++seq & 0xFFFFu;
    if (tag == 0) {
      clear = true;
      tag = ++seq & 0xFFFFu;
    }
    return tag;
  }
};

static void chunk_window(uint32_t from, uint32_t len) {
  for (uint32_t a = 0; a < len; ++a) {
    ChunkModel m{from + a};
    for (uint32_t d = 0; a + d < len; ++d) {
      // m has issued chunks from + a + 1 .. from + a + d
      const uint32_t to = from + a + d;
      const ChunkJump j = chunk_jump(from + a, to);
      CHECK(m.chunks == to);
      CHECK(j.marks == m.marks);
      CHECK(j.fan == m.fan);
      CHECK(!m.epoch);
      if (to == 0xFFFFFFFFu) break;
      m.step();
    }
  }
}

static void scan_window(uint32_t from, uint32_t len) {
  for (uint32_t a = 0; a < len; ++a) {
    if (((from + a) & 0xFFFFu) == 0 && from + a != 0) continue;  // scan_seq never rests there
    ScanModel m{from + a};
    for (uint32_t n = 0; n < len; ++n) {
      // m has run n scans: a jump to where it rests reports its clears
      const uint32_t want = m.seq;
      const ScanJump j = scan_jump(from + a, want);
      CHECK(j.seq == want && j.clear == m.clear);
      // ... and a jump onto the multiple of 2^16 the stream stepped over
      // steps over it the same way
      if ((want & 0xFFFFu) == 1 && want - 1 > from + a) {
        const ScanJump k = scan_jump(from + a, want - 1);
        CHECK(k.seq == want && k.clear && m.clear);
      }
      if (m.seq >= 0xFFFFFFF0u) break;
      const uint32_t tag = m.step();
      CHECK(tag != 0 && tag == (m.seq & 0xFFFFu));
    }
  }
}

int main() {
  CHECK(kMarkPeriod == 255u && kFanPeriod == (1u << 29) && kScanPeriod == 65536u);
  CHECK(kLastTag == 0xFFFFFFFFu && epoch_ends(kLastTag) && !epoch_ends(0) && !epoch_ends(kLastTag - 1));
  // nothing is crossed by standing still, at any value
  for (uint32_t v : {0u, 1u, 254u, 255u, 256u, 65535u, 65536u, (1u << 29) - 1, 1u << 29, 0xFFFFFFFFu}) {
    CHECK(!crosses_multiple(v, v, 255u) && !crosses_multiple(v, v, 1u << 29));
    CHECK(!chunk_jump(v, v).marks && !chunk_jump(v, v).fan);
    if ((v & 0xFFFFu) != 0 || v == 0) CHECK(!scan_jump(v, v).clear && scan_jump(v, v).seq == v);
  }
  // every pair of counters in windows around each period's multiples, the
  // start and the end of the counter
  for (uint32_t c : {0u, 255u, 510u, 65535u - 255u, 65536u, 2u * 65536u, (1u << 29), 3u * (1u << 29),
                     0xFFFFFFFFu - 149u}) {
    const uint32_t from = c >= 150 ? c - 150 : 0;
    chunk_window(from, 300);
    scan_window(from, 300);
  }
  // long jumps: the multiples between are found without stepping
  CHECK(chunk_jump(10, (1u << 29) - 1).marks && !chunk_jump(10, (1u << 29) - 1).fan);
  CHECK(chunk_jump(10, 1u << 29).fan && chunk_jump((1u << 29) - 1, 1u << 29).fan);
  CHECK(!chunk_jump(1u << 29, 10 + (1u << 29) - 1).fan);
  CHECK(chunk_jump((1u << 29) + 10, 10 + (2u << 29) - 1).fan);
  CHECK(chunk_jump(0, 0xFFFFFFFFu).marks && chunk_jump(0, 0xFFFFFFFFu).fan);
  CHECK(chunk_jump(0xFFFFFFFEu, 0xFFFFFFFFu).marks);  // 2^32 - 1 = 255 * 16843009
  CHECK(!chunk_jump(0xFFFFFFFEu, 0xFFFFFFFFu).fan);
  CHECK(scan_jump(0, 0xFFFFu).seq == 0xFFFFu && !scan_jump(0, 0xFFFFu).clear);
  CHECK(scan_jump(0, 0x10000u).seq == 0x10001u && scan_jump(0, 0x10000u).clear);
  CHECK(scan_jump(0xFFF0u, 0x1FFF0u).clear && scan_jump(0x10005u, 0x1FFFFu).clear == false);
  // the epoch's end in the step model: the chunk after 2^32 - 1 is 1, never 0
  {
    ChunkModel m{0xFFFFFFFEu};
    m.step();
    CHECK(m.chunks == 0xFFFFFFFFu && !m.epoch && m.marks);
    m.step();
    CHECK(m.chunks == 1u && m.epoch);
  }
  if (fails) {
    printf("seq_epoch_test: %d checks failed\n", fails);
    return 1;
  }
  printf("seq_epoch_test ok\n");
  return 0;
}
