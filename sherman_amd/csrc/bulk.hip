// bulk.hip — bulk load (shm_bulk_load): the tree of a sorted run of pairs
// written in one streaming pass.  The shape is known before anything runs
// (tree.cpp bulk_plan: P0 = ceil(n / leaf_fill) leaves, ceil(P / (internal_fill
// + 1)) pages per level above, items dealt out evenly, level 0 at pages 2..,
// each level after the one below, the root at page 1), so every page's
// contents, address and neighbours are arithmetic on its index: no kernel
// takes a lock or an allocation, looks back or spins on another block.
//
//   k_bulk_check   the input is strictly ascending, no kKeyMax, no kValueNull
//   k_bulk_leaves  one wave per leaf: page, summary line, occupancy byte
//   k_bulk_level   one launch per internal level, one wave per page; a page's
//                  separators are its children's lowest fences, which level 1
//                  reads from keys[] and each level above from the array the
//                  level below wrote (stream order between the launches)
//
// Pages are built as 1 KB images in the wave's LDS and leave as one plain 16 B
// store per lane (store_page): the kernel boundary publishes them, nothing in
// the launch reads them back.  16 B read per pair by the check and again by
// the leaves, 1088 B written per leaf: bound by HBM traffic, a third to a half
// of it reads (DESIGN.md §3.3.1 has the measured rates).
#include "device_common.h"
#include "page_io.h"
#include "kernels.h"

namespace shm {
namespace dev {

namespace {

// first item of page p when C items are dealt over pages as q = C / P each and
// one more for the first r = C % P (p * q <= C: no overflow)
__device__ __forceinline__ uint64_t deal_first(uint64_t p, uint64_t q, uint64_t r) {
  return p * q + (p < r ? p : r);
}

__device__ __forceinline__ uint64_t page_ga(uint16_t node, uint64_t page) {
  return ga_make(node, page * kPageSize);
}

__global__ __launch_bounds__(kBlock) void k_bulk_check(const uint64_t* __restrict__ keys,
                                                       const uint64_t* __restrict__ vals,
                                                       uint64_t n, uint32_t* status) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint64_t k = keys[i];
    const uint64_t v = vals[i];
    const uint64_t k1 = i + 1 < n ? keys[i + 1] : kKeyMax;
    // k >= k1 also rejects kKeyMax anywhere (nothing is larger)
    bad |= k >= k1 || v == kValueNull;
  }
  if (ballot(bad) != 0 && lane_id() == 0) atomicOr(status, 1u);
}

__global__ __launch_bounds__(kBlock) void k_bulk_leaves(BulkLeafArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_page[kWavesPerBlock][kPageDwords + 8];
  __shared__ __attribute__((aligned(16))) uint32_t s_sum[kWavesPerBlock][kSumBytes / 4];
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t p = (uint64_t)blockIdx.x * kWavesPerBlock + (uint64_t)w;
  if (p >= a.pages) return;  // wave-uniform; no block barrier below
  uint32_t* lp = s_page[w];
  uint32_t* sl = s_sum[w];
  const uint64_t first = deal_first(p, a.q, a.r);
  const uint32_t cnt = (uint32_t)a.q + (p < a.r ? 1u : 0u);
  const bool has_next = p + 1 < a.pages;
  // lane e < cnt: its pair; lane cnt (<= 53): the next leaf's first key
  uint64_t key = 0, val = 0;
  if ((uint32_t)lane < cnt) {
    key = a.keys[first + lane];
    val = a.vals[first + lane];
  } else if ((uint32_t)lane == cnt && has_next) {
    key = a.keys[first + cnt];
  }
  const uint64_t lowest = p == 0 ? kKeyMin : rl64(key, 0);
  const uint64_t highest = has_next ? shfl64(key, (int)cnt) : kKeyMax;
  const uint64_t page = a.page0 + p;
  const uint64_t sibling = has_next ? page_ga(a.node, page + 1) : 0ull;
  init_page_image(lp, 1, 0, sibling, 0, -1, lowest, highest);
  if (lane < (int)(kSumBytes / 4)) sl[lane] = 0;
  wave_lds_sync();
  if ((uint32_t)lane < cnt) {
    put_leaf_entry(lp, lane, key, val, 1, 1);
    reinterpret_cast<uint8_t*>(sl)[kSumOffFp + lane] = (uint8_t)key_fp(key);
  }
  if (lane == 0) {
    lp[kOffLeafRear / 4] = 1;  // rear_version, byte 1016
    sl[0] = (uint32_t)highest;
    sl[1] = (uint32_t)(highest >> 32);
    reinterpret_cast<uint8_t*>(sl)[kSumOffTag] = kSumLeaf;
  }
  store_page(a.arena, page * kPageSize, lp);  // orders the LDS writes first
  if (lane < (int)(kSumBytes / 16))
    *reinterpret_cast<u32x4*>(a.sum + page * kSumBytes + 16 * lane) =
        *reinterpret_cast<const u32x4*>(sl + 4 * lane);
  if (lane == 0) a.leaf_hw[page] = (uint8_t)cnt;
}

__global__ __launch_bounds__(kBlock) void k_bulk_level(BulkLevelArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_page[kWavesPerBlock][kPageDwords + 8];
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t p = (uint64_t)blockIdx.x * kWavesPerBlock + (uint64_t)w;
  if (p >= a.pages) return;
  uint32_t* lp = s_page[w];
  const uint64_t c0 = deal_first(p, a.q, a.r);
  const uint32_t ch = (uint32_t)a.q + (p < a.r ? 1u : 0u);  // 2 .. 61 children
  const bool has_next = p + 1 < a.pages;
  // lane c < ch: the lowest fence of child c; lane ch: of the next page's first
  uint64_t low = 0;
  if ((uint32_t)lane < ch || ((uint32_t)lane == ch && has_next)) {
    const uint64_t c = c0 + (uint64_t)lane;
    if (c != 0) low = a.low_in ? a.low_in[c] : a.keys[deal_first(c, a.leaf_q, a.leaf_r)];
  }
  const uint64_t lowest = rl64(low, 0);
  const uint64_t highest = has_next ? shfl64(low, (int)ch) : kKeyMax;
  if (a.low_out && lane == 0) a.low_out[p] = lowest;
  const uint64_t page = a.page0 + p;
  const uint64_t sibling = has_next ? page_ga(a.node, page + 1) : 0ull;
  init_page_image(lp, 1, page_ga(a.node, a.child0 + c0), sibling, a.level, (int32_t)ch - 2, lowest,
                  highest);
  wave_lds_sync();
  if (lane >= 1 && (uint32_t)lane < ch) {  // record lane - 1 names child `lane`
    const uint64_t ptr = page_ga(a.node, a.child0 + c0 + (uint64_t)lane);
    uint32_t* d = lp + (kOffRecords + kInternalEntry * (lane - 1)) / 4;
    d[0] = (uint32_t)low;
    d[1] = (uint32_t)(low >> 32);
    d[2] = (uint32_t)ptr;
    d[3] = (uint32_t)(ptr >> 32);
  }
  if (lane == 0) lp[kOffInternalRear / 4] = 1;  // rear_version, byte 1020
  store_page(a.arena, page * kPageSize, lp);
  // not a leaf: no summary tag (an earlier tree's leaf may have sat here)
  if (lane < (int)(kSumBytes / 16))
    *reinterpret_cast<u32x4*>(a.sum + page * kSumBytes + 16 * lane) = u32x4{0, 0, 0, 0};
  if (lane == 0) a.leaf_hw[page] = kLeafHwFull;
}

unsigned wave_blocks(uint64_t waves) {
  return (unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
}

}  // namespace

void launch_bulk_check(const uint64_t* keys, const uint64_t* vals, uint64_t n, uint32_t* status,
                       hipStream_t s) {
  if (n == 0) return;
  const uint64_t blocks = (n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_bulk_check, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kBlock),
                     0, s, keys, vals, n, status);
}

void launch_bulk_leaves(const BulkLeafArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bulk_leaves, dim3(wave_blocks(a.pages)), dim3(kBlock), 0, s, a);
}

void launch_bulk_level(const BulkLevelArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bulk_level, dim3(wave_blocks(a.pages)), dim3(kBlock), 0, s, a);
}

}  // namespace dev
}  // namespace shm
