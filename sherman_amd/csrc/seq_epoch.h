// seq_epoch.h — the periods of the tree's counter-derived tags and the host
// arithmetic that guards them (tree.cpp: insert_begin, insert_apply,
// scan_tag, shm__seq_jump).  Pure host code without a HIP type, so a
// stand-alone program can exercise it (tests/native/seq_epoch_test.cpp).
//
// A tag derived from a counter recurs after its period; a word that still
// carries it then reads as fresh.  Each period below has one host-side clear
// that runs when the counter reaches a multiple of it (DESIGN.md "Counters
// and their periods").
#pragma once
#include <stdint.h>

namespace shm {
namespace seq {

// per-page byte marks (kernels.h new_mark: tag % 255 + 1): cleared by the
// chunk whose tag is a multiple of 255
constexpr uint32_t kMarkPeriod = 255u;
// fan-in words (split_wave.h fan_tag: (uint32_t)(tag << 3) | level): cleared
// by the chunk whose tag is a multiple of 2^29
constexpr uint32_t kFanPeriod = 1u << 29;
// 16-bit tags of launch_scan_u64_total's tile words: scan_seq never rests on
// a multiple of 2^16 (scan_tag clears the words there and steps on)
constexpr uint32_t kScanPeriod = 1u << 16;
// the last chunk tag of an epoch: the chunk after it is tag 1 of the next
// epoch (tree.cpp epoch_reset), so no caller and no device word sees tag 0
constexpr uint32_t kLastTag = 0xFFFFFFFFu;

// a multiple of `period` (> 0) lies in (cur, to], cur <= to
inline bool crosses_multiple(uint32_t cur, uint32_t to, uint32_t period) {
  return to / period != cur / period;
}

// the chunk counter is at the end of its epoch: the next chunk starts a new one
inline bool epoch_ends(uint32_t chunks) { return chunks == kLastTag; }

// the clears a stream of chunks cur + 1 .. to performs on the host
struct ChunkJump {
  bool marks;  // the page marks (a tag that is a multiple of 255)
  bool fan;    // the fan-in words (a tag that is a multiple of 2^29)
};
inline ChunkJump chunk_jump(uint32_t cur, uint32_t to) {
  return ChunkJump{crosses_multiple(cur, to, kMarkPeriod), crosses_multiple(cur, to, kFanPeriod)};
}

// scans cur + 1 .. to: whether scan_tag clears the tile words on the way, and
// where the counter rests afterwards (a multiple of 2^16 is stepped over, as
// scan_tag does)
struct ScanJump {
  bool clear;
  uint32_t seq;
};
inline ScanJump scan_jump(uint32_t cur, uint32_t to) {
  ScanJump j{crosses_multiple(cur, to, kScanPeriod), to};
  if ((to & (kScanPeriod - 1)) == 0 && to != cur) j.seq = to + 1;
  return j;
}

}  // namespace seq
}  // namespace shm
