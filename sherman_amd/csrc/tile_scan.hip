// tile_scan.hip — the one-launch look-back kernels over 1024-element tiles: the
// insert pipeline's segmentation (k_seg_fill, its tile in seg_tile.h) and the
// exclusive scan of u64 counts (k_scan_u64), plus k_add_u64.
#include "device_common.h"
#include "kernels.h"
#include "upper_quick.h"
#include "seg_tile.h"

namespace shm {
namespace dev {

namespace {
constexpr int kT = 256;
// A tile is kSegTile = 1024 elements, 4 consecutive per thread of a 256-thread
// block (seg_tile.h has the block scan).
constexpr int kScanPer = (int)kSegTile / kT;
static_assert(kScanPer * kT == (int)kSegTile, "tile shape");
static_assert(kT == segt::kT, "segt::block_scan's block");
}  // namespace

// n_dev (nullable): the device-side op count, n its upper bound
__device__ __forceinline__ uint64_t dev_n(const uint64_t* n_dev, uint64_t n) {
  return n_dev ? *n_dev : n;
}

// One launch: every 1024-op tile counts its staged heads, publishes the
// count in its tagged word (chunk tag << 32 | count), sums the words of the
// tiles before it (tile index = blockIdx, or a ticket when the tree passes a
// counter, lookback_index; tree.cpp lb_ctr says which and why), and fills its
// segments: seg_start / seg_page at each staged head, seg_end at its run's
// last op (the count of staged heads up to and including that op is the
// segment's position + 1).

__global__ __launch_bounds__(kT) void k_seg_fill(const uint64_t* page, uint64_t n,
                                                 const uint64_t* n_dev, uint64_t* lbw,
                                                 uint32_t* seg_start, uint32_t* seg_end,
                                                 uint64_t* seg_page, uint32_t* num_seg,
                                                 const uint8_t* pnew, uint32_t tag,
                                                 const uint32_t* any_new, uint32_t* err,
                                                 UpperArgs q, int has_q, uint32_t* ids,
                                                 uint32_t self_after, const uint64_t* ndel_src,
                                                 uint64_t* ndel_dst) {
  // the chunk's delete count into UpperCtl (k_upper's copy), before anything
  // of this chunk publishes its op buffers free (below, or k_upper)
  if (ndel_dst && blockIdx.x == 0 && threadIdx.x == 0) *ndel_dst = *ndel_src;
  if (any_new && *any_new != tag) {  // no op of this chunk marked a page (every block)
    if (blockIdx.x == 0) {
      if (threadIdx.x == 0) *num_seg = 0;
      if (has_q) seg_complete_unchanged(q);
    }
    return;
  }
  // the look-back's tile: a ticket, taken by every block past the check above
  const uint32_t b = lookback_index(ids);
  const uint64_t nv = dev_n(n_dev, n);
  if ((uint64_t)b * kSegTile >= nv) {  // past the device count (the grid covers n)
    if (nv == 0 && b == 0 && threadIdx.x == 0) *num_seg = 0;
    return;
  }
  segt::seg_tile(page, nv, b, lbw, seg_start, seg_end, seg_page, num_seg, pnew, tag, self_after);
}

void launch_segment(const uint64_t* page, uint64_t n, const uint64_t* n_dev, uint64_t* lbw,
                    uint32_t* seg_start, uint32_t* seg_end, uint64_t* seg_page,
                    uint32_t* num_seg, const uint8_t* pnew, uint32_t tag,
                    const uint32_t* any_new, uint32_t* err, hipStream_t s,
                    const UpperArgs* quick, uint32_t* ids, uint32_t self_after,
                    const uint64_t* ndel_src, uint64_t* ndel_dst) {
  const UpperArgs q = quick ? *quick : UpperArgs{};
  const int has_q = quick && any_new ? 1 : 0;
  // at least one block: block 0 copies the delete count even for no ops
  const uint64_t tiles = n ? seg_tiles(n) : 1;
  hipLaunchKernelGGL(k_seg_fill, dim3((unsigned)tiles), dim3(kT), 0, s, page, n, n_dev, lbw,
                     seg_start, seg_end, seg_page, num_seg, pnew, tag, any_new, err, q, has_q, ids,
                     self_after, ndel_src, ndel_dst);
}

// Exclusive scan of u64 counts in one launch: every 1024-element tile
// publishes its sum in a tagged word (tag << 48 | sum: a range scan's
// counts total < 2^48), sums the words of the tiles before it (as
// k_seg_fill) and writes its offsets; the thread holding n - 1 writes
// tot = {total, *err} (nullable).
__global__ __launch_bounds__(kT) void k_scan_u64(const uint64_t* in, uint64_t n, uint64_t* lbw,
                                                 uint32_t tag, uint64_t* out,
                                                 const uint32_t* err, uint64_t* tot,
                                                 uint32_t* err_out, uint32_t* ids) {
  __shared__ uint64_t s_pre[kT / kWave];
  const uint32_t b = lookback_index(ids);  // the tile
  const uint64_t i0 = (uint64_t)b * kSegTile + (uint64_t)threadIdx.x * kScanPer;
  uint64_t v[kScanPer], c = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    v[j] = i0 + j < n ? in[i0 + j] : 0;
    c += v[j];
  }
  uint64_t total;
  const uint64_t local = segt::block_scan<uint64_t>(c, &total);
  constexpr uint64_t kMask = (1ull << 48) - 1;
  const uint64_t tg = (uint64_t)(tag & 0xFFFFu) << 48;
  if (threadIdx.x == 0)
    __hip_atomic_store(lbw + b, tg | (total & kMask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint64_t pre = 0;
  for (uint32_t x = threadIdx.x; x < b; x += kT) {
    uint64_t w = 0;
    for (uint32_t spin = 0;; ++spin) {
      w = __hip_atomic_load(lbw + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((w & ~kMask) == tg) break;
      if (spin > (1u << 24)) {
        atomicOr(err_out, kErrScanSpin);
        w = tg;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    pre += w & kMask;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) pre += __shfl_xor(pre, o);
  if (lane_id() == 0) s_pre[threadIdx.x / kWave] = pre;
  __syncthreads();
  uint64_t pos = local;
#pragma unroll
  for (int w = 0; w < kT / kWave; ++w) pos += s_pre[w];
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    if (i0 + j < n) out[i0 + j] = pos;
    pos += v[j];
    if (tot && i0 + j + 1 == n) {
      tot[0] = pos;
      tot[1] = *err;
    }
  }
}

void launch_scan_u64_total(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* lbw,
                           uint32_t tag, const uint32_t* err, uint64_t* tot, uint32_t* err_out,
                           uint32_t* ids, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_scan_u64, dim3((unsigned)seg_tiles(n)), dim3(kT), 0, s, in, n, lbw, tag, out,
                     err, tot, err_out, ids);
}

__global__ void k_add_u64(uint64_t* x, uint64_t n, uint64_t c) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] += c;
}

void launch_add_u64(uint64_t* x, uint64_t n, uint64_t c, hipStream_t s) {
  if (n && c) hipLaunchKernelGGL(k_add_u64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                                 x, n, c);
}

}  // namespace dev
}  // namespace shm
