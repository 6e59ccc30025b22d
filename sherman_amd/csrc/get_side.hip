// get_side.hip — what the gets read beside the pages, rebuilt from the pages:
// the top of the tree for k_get_sum's LDS replica (k_top) and the summary
// lines of a loaded image (k_sum_rebuild).
#include "device_common.h"
#include "page_fields.h"
#include "page_io.h"
#include "sum_line.h"

#include "kernels.h"

namespace shm {
namespace dev {

// ---- the top of the tree for the LDS replica ---------------------------------
// One block, breadth first from the root: level by level, every page's
// children (leftmost, then the records' pointers) and their lowest fences
// (the parent's lowest for leftmost, the record key otherwise,
// Tree.cpp:665-685), in key order, until the next level would not fit max_n
// pages or the leaves are next.  scratch: 4 x max_n u64.
__global__ __launch_bounds__(1024) void k_top(const uint8_t* arena, uint64_t arena_bytes,
                                              uint16_t node, uint64_t root, uint32_t max_n,
                                              uint64_t* keys, uint32_t* pages,
                                              uint64_t* scratch, uint32_t* n_out,
                                              uint32_t* err) {
  __shared__ uint32_t s_n, s_ws[16], s_stop;
  const int t = threadIdx.x;
  uint64_t* cur_p = scratch;
  uint64_t* cur_k = scratch + max_n;
  uint64_t* nxt_p = scratch + 2 * (uint64_t)max_n;
  uint64_t* nxt_k = scratch + 3 * (uint64_t)max_n;
  if (t == 0) {
    cur_p[0] = root;
    cur_k[0] = kKeyMin;
    s_n = 1;
    s_stop = 0;
  }
  __syncthreads();
  for (int level = 0; level < kMaxLevelOfTree; ++level) {
    const uint32_t n = s_n;
    // children per page of the current level (0: a leaf level; stop)
    uint32_t total = 0;
    for (uint32_t base = 0; base < n; base += 1024) {
      const uint32_t j = base + t;
      uint32_t c = 0;
      if (j < n) {
        const uint64_t p = cur_p[j];
        if (!ptr_ok(p, node, arena_bytes)) {
          atomicOr(err, kErrBadPtr);
          atomicOr(&s_stop, 1u);
        } else {
          const uint8_t* pg = arena + ga_offset(p);
          const uint64_t leftmost = hdr_leftmost(page_dw(pg));
          const int cnt = hdr_last_index(page_dw(pg)) + 1;
          c = leftmost ? 1u + (uint32_t)(cnt < 0 ? 0 : cnt) : 0u;
          if (!leftmost || pg[kOffLevel] <= 1) atomicOr(&s_stop, 1u);  // children are leaves
        }
      }
      total += c;
    }
    // block total of children
    uint32_t v = total;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    if ((t & 63) == 0) s_ws[t >> 6] = v;
    __syncthreads();
    uint32_t all = 0;
    for (int w = 0; w < 16; ++w) all += s_ws[w];
    const bool stop = s_stop != 0 || all > max_n || all == 0;
    __syncthreads();
    if (stop) break;
    // children in order: one pass per 1024 pages, an exclusive scan of counts
    uint32_t run = 0;
    for (uint32_t base = 0; base < n; base += 1024) {
      const uint32_t j = base + t;
      uint32_t c = 0;
      uint64_t leftmost = 0, lowest = 0;
      const uint8_t* pg = nullptr;
      if (j < n) {
        pg = arena + ga_offset(cur_p[j]);
        leftmost = hdr_leftmost(page_dw(pg));
        const int cnt = hdr_last_index(page_dw(pg)) + 1;
        c = 1u + (uint32_t)(cnt < 0 ? 0 : cnt);
        lowest = cur_k[j];
      }
      uint32_t incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, o);
        if ((t & 63) >= o) incl += y;
      }
      if ((t & 63) == 63) s_ws[t >> 6] = incl;
      __syncthreads();
      uint32_t wb = 0, bt = 0;
      for (int w = 0; w < 16; ++w) {
        wb += w < (t >> 6) ? s_ws[w] : 0u;
        bt += s_ws[w];
      }
      const uint32_t pos = run + wb + incl - c;
      if (c) {
        nxt_p[pos] = leftmost;
        nxt_k[pos] = lowest;
        for (uint32_t r = 0; r + 1 < c; ++r) {
          nxt_k[pos + 1 + r] = rec_key(page_dw(pg), (int)r);
          nxt_p[pos + 1 + r] = rec_ptr(page_dw(pg), (int)r);
        }
      }
      run += bt;
      __syncthreads();
    }
    // swap
    uint64_t* x = cur_p;
    cur_p = nxt_p;
    nxt_p = x;
    x = cur_k;
    cur_k = nxt_k;
    nxt_k = x;
    if (t == 0) s_n = all;
    __syncthreads();
  }
  const uint32_t n = s_n;
  for (uint32_t j = t; j < n; j += 1024) {
    keys[j] = cur_k[j];
    pages[j] = dir_page_index(cur_p[j]);
  }
  if (t == 0) *n_out = n;
}

void launch_top(const uint8_t* arena, uint64_t arena_bytes, uint16_t node, uint64_t root,
                uint32_t max_n, uint64_t* keys, uint32_t* pages, uint64_t* scratch,
                uint32_t* n_out, uint32_t* err, hipStream_t s) {
  hipLaunchKernelGGL(k_top, dim3(1), dim3(1024), 0, s, arena, arena_bytes, node, root, max_n,
                     keys, pages, scratch, n_out, err);
}

// summaries of a loaded image: one wave per page.  Only the leaves the image
// reaches from its root (leaf[pg] != 0, the host's walk in shm_load_image) get
// a line: the tag says "a current leaf of the tree" to the page sweeps
// (leafdir.hip swept_leaf), and a page the tree does not reach is none,
// whatever its bytes look like.  The host zeroed every line before.
__global__ __launch_bounds__(256) void k_sum_rebuild(const uint8_t* arena, uint64_t pages,
                                                     const uint8_t* __restrict__ leaf,
                                                     uint8_t* sum) {
  const uint64_t pg = 1 + ((uint64_t)blockIdx.x * 256 + threadIdx.x) / kWave;
  if (pg >= pages || !leaf[pg]) return;  // wave-uniform
  const int lane = lane_id();
  const uint8_t* page = arena + pg * kPageSize;
  const PageHdr h = read_hdr(page_dw(page));
  const uint64_t leftmost = h.leftmost, highest = h.highest;
  if (leftmost != 0) {  // internal page: no summary
    if (lane == 0) clear_leaf_sum(sum, pg * kPageSize);
    return;
  }
  uint32_t fp = 0;
  if (lane < kLeafCardinality) {
    uint64_t ek, ev;
    uint32_t ef, er;
    lane_entry(page, lane, ek, ev, ef, er);
    fp = ev != kValueNull ? key_fp(ek) : 0u;
  }
  put_leaf_sum(sum, pg * kPageSize, highest, fp);
}

void launch_sum_rebuild(const uint8_t* arena, uint64_t pages, const uint8_t* leaf, uint8_t* sum,
                        hipStream_t s) {
  if (pages <= 1) return;
  const uint64_t waves = pages - 1;
  hipLaunchKernelGGL(k_sum_rebuild, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, arena,
                     pages, leaf, sum);
}

}  // namespace dev
}  // namespace shm
