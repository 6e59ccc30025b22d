// page_group.h — the 16-lane "page group" that reads one 1 KB page: what
// k_range, k_scan / k_rscan, k_export_leaf and k_rank / k_count / k_select
// share (range.hip, scan.hip, export.hip, order.hip).
//
// A wave is four groups of 16 lanes, one scan / unit / query per group, so
// four independent chains of dependent page reads are in flight per wave
// (range.hip's header gives the reasons).  Lane li of a group holds four 16 B
// chunks of the group's page: chunks li, li + 16, li + 32 and li + 48 (RPage;
// 256 B coalesced per group per load).  The page goes through those registers
// into the group's 1 KB LDS slot (rstage), where the header fields are read
// (page_fields.h: hdr_*, rec_key, rec_ptr) and each lane takes its four
// consecutive 18 B entries (leaf_chunk.h).  Chunk 3, the page's last 256 B, is read only when the
// leaf's occupancy bound says a valid slot may lie there (rload3 +
// rload_last, leaf_load); rload reads the whole page.
//
// Not here: the descent to a key's leaf.  range.hip (range_walk) and scan.hip
// (leaf_descend) each have their own; DESIGN.md §3.4.1 says why.
#pragma once
#include "device_common.h"
#include "kernels.h"
#include "page_fields.h"

namespace shm {
namespace dev {

namespace {
constexpr int kRG = 4;                        // groups per wave
constexpr int kRL = kWave / kRG;              // lanes per group
constexpr int kRE = 4;                        // leaf entries per lane
constexpr int kRCD = kLeafEntry * kRE / 4;    // dwords of a lane's entry chunk
constexpr int kRChunks = kPageSize / 16 / kRL;  // 16 B page chunks per lane
static_assert(kRL * kRE >= kLeafCardinality, "entries per group");
// the hit keys of one leaf, padded to a pair (u64x2), fit the page slot
static_assert((kLeafCardinality + 1) * 8 <= (int)kPageSize, "key list");

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

struct RPage {
  u32x4 c[kRChunks];
};

__device__ __forceinline__ void rload(const uint8_t* arena, uint64_t p, int li, RPage& w) {
  const uint8_t* b = arena + ga_offset(p) + 16 * li;
#pragma unroll
  for (int k = 0; k < kRChunks; ++k) w.c[k] = *reinterpret_cast<const u32x4*>(b + 16 * kRL * k);
}
// chunks 0..2 (bytes 0..767: the header and slots 0..39); chunk 3 (slots
// 40..53 and the rear version) only when the leaf's occupancy bound says a
// valid slot may lie there (layout.h leaf_hw: every slot >= hw is empty)
constexpr uint32_t kChunk3Hw = 41;  // slot 40 ends past byte 767
__device__ __forceinline__ void rload3(const uint8_t* arena, uint64_t p, int li, RPage& w) {
  const uint8_t* b = arena + ga_offset(p) + 16 * li;
#pragma unroll
  for (int k = 0; k < kRChunks - 1; ++k)
    w.c[k] = *reinterpret_cast<const u32x4*>(b + 16 * kRL * k);
}
__device__ __forceinline__ void rload_last(const uint8_t* arena, uint64_t p, int li, RPage& w) {
  w.c[kRChunks - 1] =
      *reinterpret_cast<const u32x4*>(arena + ga_offset(p) + 16 * li + 16 * kRL * (kRChunks - 1));
}
__device__ __forceinline__ void rstage(uint32_t* lp, int li, const RPage& w) {
#pragma unroll
  for (int k = 0; k < kRChunks; ++k) *reinterpret_cast<u32x4*>(lp + 4 * (li + kRL * k)) = w.c[k];
}
// exclusive prefix of v over the 16 lanes of each group; *tot = group sum
__device__ __forceinline__ uint32_t group_scan(uint32_t v, int li, uint32_t* tot) {
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < kRL; off <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)incl, off, kRL);
    if (li >= off) incl += y;
  }
  *tot = (uint32_t)__shfl((int)incl, kRL - 1, kRL);
  return incl - v;
}
// a leaf's bytes into w: its last 256 B only when its occupancy bound reaches
// slot 40 (pages of a loaded image: kLeafHwFull, read whole).  Args: any
// argument struct with arena and leaf_hw (ExportArgs, OrderArgs)
template <class Args>
__device__ __forceinline__ void leaf_load(const Args& a, uint64_t p, int li, RPage& w,
                                          uint32_t& hw) {
  const uint32_t h = a.leaf_hw ? a.leaf_hw[ga_offset(p) >> 10] : kLeafHwFull;
  rload3(a.arena, p, li, w);
  if (h >= kChunk3Hw) rload_last(a.arena, p, li, w);
  hw = h < (uint32_t)kLeafCardinality ? h : (uint32_t)kLeafCardinality;
}
}  // namespace

}  // namespace dev
}  // namespace shm
