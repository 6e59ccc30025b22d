// scan.hip — batched ordered scans with a count limit (shm_scan_batch): the
// first `limit` valid entries with from <= key <= to in ascending unsigned
// key order, keys and values, into a fixed row per scan.  The traversal and
// the validity rule are Tree::range_query's (src/Tree.cpp:461-540: the leaf
// holding `from`, then the sibling chain; value != kValueNull and front ==
// rear entry version); the order inside a leaf, the keys in the output and
// the early stop are new.
//
// The kernel has k_range's shape (range.hip's header gives the reasons): four
// scans per wave, 16 lanes per scan and four 18 B entries per lane, the page
// moved through registers into the group's 1 KB LDS slot, the start leaf from
// the leaf directory (or a descent from the covering internal page / the
// root), B-link right turns on a stale start, leaf_hw bounding the page read.
// The page helpers are page_group.h's.  leaf_descend is a copy of the descent
// inside range.hip's range_walk: called from there, it changes the register
// assignment of k_range, the benchmark's C5 kernel.
//
// Order.  Leaves are ordered against each other by their fences; inside a
// leaf the valid slots are not (updates land in place, inserts take the first
// empty slot).  So each leaf's hits are ranked and appended: once every lane
// has its entries in registers the group's page slot is dead, and the hit
// keys are compacted into it (54 x 8 B; the values stay in registers).  Each
// lane then counts, for each of its hits, the listed keys below it (two keys
// per broadcast 16 B LDS read) and stores its (key, value) at row position
// cnt + rank when that is below the limit.  A leaf's valid keys are unique,
// so the ranks are a permutation; the group checks their sum and reports
// kErrInconsistent otherwise (two equal keys would share a position).
//
// Early stop.  The walk ends when cnt >= limit, when highest > to, or with
// the chain.  The hit count is known only after the compare, and the sibling
// is loaded after it: loaded as soon as the header says the range continues
// (k_range's order) its latency overlaps the compare and the rank, but a scan
// that the limit ends has then read 768 B in vain, and that form measured
// 3-5 % slower at limits 1, 10 and 100 (DESIGN.md "Ordered scans").
//
// k_rscan (shm_rscan_batch), below k_scan, reads the same order downwards with
// the same helpers: its comment gives the step to the left.
#include "device_common.h"
#include "dir_entry.h"
#include "kernels.h"
#include "leaf_chunk.h"
#include "page_group.h"

namespace shm {
namespace dev {

namespace {
constexpr int kScanWaves = 4;

// Descends each group's scan (act: the group has one) from the leaf
// directory / the root to the leaf whose fences hold lo; on return w holds
// that leaf, whose slots >= hw are empty.  A bad pointer ends the scan (act =
// false, kErrBadPtr).  Wave-uniform call (ballot loop).
__device__ __forceinline__ void leaf_descend(const ScanArgs& a, bool& act, uint64_t lo,
                                             uint32_t* lp, int li, RPage& w, int& hops,
                                             uint32_t& hw, uint32_t& err) {
  uint64_t p = 0;
  if (act) {
    p = a.dir ? dir_start(a.dir, a.dir_lo, a.dir_shift, a.dir_n, a.node, lo, a.root) : a.root;
    if (!ptr_ok(p, a.node, a.arena_bytes)) {
      err |= kErrBadPtr;
      act = false;
    } else if (a.leaf_hw) {
      // the start page's last 256 B only if its occupancy bound reaches
      // slot 40 (internal pages: kLeafHwFull, read whole)
      const uint32_t h = a.leaf_hw[ga_offset(p) >> 10];
      rload3(a.arena, p, li, w);
      if (h >= kChunk3Hw) rload_last(a.arena, p, li, w);
      hw = h < (uint32_t)kLeafCardinality ? h : (uint32_t)kLeafCardinality;
    } else {
      rload(a.arena, p, li, w);
    }
  }
  bool desc = act;
  while (ballot(desc)) {
    if (desc) rstage(lp, li, w);
    wave_lds_sync();
    if (desc) {
      const uint64_t sibling = hdr_sibling(lp);
      const uint64_t highest = hdr_highest(lp);
      const uint64_t leftmost = hdr_leftmost(lp);
      uint64_t np = 0;
      if (lo >= highest && sibling) {
        np = sibling;
      } else if (leftmost != 0) {
        // internal page (Tree.cpp:665-685): child = number of keys <= lo
        const int last = hdr_last_index(lp);
        uint32_t c = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int j = li + kRL * m;
          c += (j <= last && j < kInternalCardinality && rec_key(lp, j) <= lo) ? 1u : 0u;
        }
        uint32_t tot;
        (void)group_scan(c, li, &tot);
        np = tot == 0 ? leftmost : rec_ptr(lp, (int)tot - 1);
      }
      if (np) {
        if (++hops > kMaxRounds || !ptr_ok(np, a.node, a.arena_bytes)) {
          err |= kErrBadPtr;
          act = false;
          desc = false;
        } else {
          p = np;
          hw = kLeafCardinality;  // read whole below
        }
      } else {
        desc = false;  // a leaf: w holds it
      }
    }
    wave_lds_sync();  // LDS reads done before the next stage
    if (desc) rload(a.arena, p, li, w);
  }
}
}  // namespace

__global__ __launch_bounds__(kScanWaves* kWave) void k_scan(ScanArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_page[kScanWaves][kRG * kPageDwords];
  const int lane = lane_id();
  const int wv = threadIdx.x >> 6;
  const int q = lane / kRL, li = lane % kRL;
  const uint64_t Q = ((uint64_t)blockIdx.x * kScanWaves + (uint64_t)wv) * kRG + (uint64_t)q;
  const bool has = Q < a.n;
  if (!ballot(has)) return;  // wave-uniform
  uint32_t* lp = s_page[wv] + q * kPageDwords;
  uint64_t* lk = reinterpret_cast<uint64_t*>(lp);  // the leaf's hit keys, once its page is unpacked
  const uint32_t limit = a.limit;
  uint64_t lo = 0, hi = kKeyMax;
  if (has) {
    lo = a.from[Q];
    if (a.to) hi = a.to[Q];
  }
  const uint64_t row = Q * (uint64_t)limit;  // the scan's row (written only for has, below limit)
  uint32_t err = 0;
  uint32_t cnt = 0;
  bool act = has && lo <= hi && lo != kKeyMax;  // no stored key equals kKeyMax

  RPage w;
  int hops = 0;
  uint32_t hw = kLeafCardinality;  // slots of the current leaf that may be valid
  leaf_descend(a, act, lo, lp, li, w, hops, hw, err);

  // ---- the leaf chain; w holds the current leaf -------------------------------
  const int ebase = chunk_base<kRE>(li);
  while (ballot(act)) {
    if (act) rstage(lp, li, w);
    wave_lds_sync();
    bool more = false;
    uint64_t sibling = 0;
    bool hit[kRE];
    uint64_t ek[kRE], ev[kRE];
#pragma unroll
    for (int j = 0; j < kRE; ++j) {
      hit[j] = false;
      ek[j] = 0;
      ev[j] = 0;
    }
    if (act) {
      sibling = hdr_sibling(lp);
      const uint64_t highest = hdr_highest(lp);
      more = sibling != 0 && highest <= hi;
      if (more && (++hops > (1 << 24) || !ptr_ok(sibling, a.node, a.arena_bytes))) {
        err |= kErrBadPtr;
        more = false;
      }
      uint32_t D[kRCD];
      const uint32_t* ep = lp + (kOffRecords + kLeafEntry * ebase) / 4;
#pragma unroll
      for (int i = 0; i < kRCD; ++i) D[i] = ep[i];
      uint32_t ef[kRE], er[kRE];
      chunk_entries<kRE>(D, ek, ev, ef, er);
#pragma unroll
      for (int j = 0; j < kRE; ++j)
        hit[j] = ebase + j >= li * kRE && (uint32_t)(ebase + j) < hw && ev[j] != kValueNull &&
                 ((ef[j] ^ er[j]) & 0xF) == 0 && ek[j] >= lo && ek[j] <= hi;
    }
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kRE; ++j) c += hit[j] ? 1u : 0u;
    uint32_t tot;  // <= kLeafCardinality: every slot has one owner lane
    uint32_t idx = group_scan(c, li, &tot);
    wave_lds_sync();  // the page is in registers: its slot becomes the key list
#pragma unroll
    for (int j = 0; j < kRE; ++j)
      if (hit[j]) lk[idx++] = ek[j];
    if (li == 0 && (tot & 1u)) lk[tot] = kKeyMax;  // pads the last pair: below no key
    wave_lds_sync();
    uint32_t r[kRE] = {0, 0, 0, 0};
#pragma unroll 1  // unrolled, its loads in flight cost 20 VGPRs and a wave per SIMD
    for (uint32_t m = 0; m < tot; m += 2) {
      const u64x2 km = *reinterpret_cast<const u64x2*>(lk + m);
#pragma unroll
      for (int j = 0; j < kRE; ++j)
        r[j] += (km.x < ek[j] ? 1u : 0u) + (km.y < ek[j] ? 1u : 0u);
    }
    uint32_t rs = 0;
#pragma unroll
    for (int j = 0; j < kRE; ++j) {
      if (hit[j]) {
        rs += r[j];
        const uint32_t pos = cnt + r[j];
        if (pos < limit) {
          a.keys[row + pos] = ek[j];
          a.vals[row + pos] = ev[j];
        }
      }
    }
    uint32_t rt;
    (void)group_scan(rs, li, &rt);
    if (rt * 2u != tot * (tot - 1u)) err |= kErrInconsistent;  // equal keys in one leaf
    cnt = cnt + tot < limit ? cnt + tot : limit;
    wave_lds_sync();  // LDS reads done before the next stage
    if (act) {
      if (more && cnt < limit) {
        // w is staged: its registers take the sibling's bytes
        const uint32_t hwn = a.leaf_hw ? a.leaf_hw[ga_offset(sibling) >> 10] : kLeafHwFull;
        rload3(a.arena, sibling, li, w);
        if (hwn >= kChunk3Hw) rload_last(a.arena, sibling, li, w);
        hw = hwn < (uint32_t)kLeafCardinality ? hwn : (uint32_t)kLeafCardinality;
      } else {
        act = false;
      }
    }
  }
  if (has && li == 0) a.counts[Q] = cnt;
  if (err) {
    atomicOr(a.err, err);
    if (a.status) atomicOr(reinterpret_cast<unsigned long long*>(a.status + 1), (unsigned long long)err);
  }
}

// Descending scans (shm_rscan_batch): scan i returns the first min(limit,
// matches) valid entries with to[i] <= key <= from[i] in descending key order.
// The leaf chain has no left links and needs none: a leaf's left neighbour is
// the leaf that holds lowest - 1 (B-link fences), so a step to the left is one
// leaf_descend(lowest - 1), a directory entry plus the page (a descent from
// the root without the directory).  One loop, one descent per iteration with a
// hop count of its own; the steps are bounded apart, and each step's leaf must
// lie strictly below the last one (a corrupt image must not loop).  Inside a
// leaf the hits are ranked by the listed keys above them; the pad word of an
// odd count is 0, which is above no key.
// The occupancy hint keeps k_scan's 6 waves per SIMD (80 VGPRs, no scratch):
// left alone the allocator takes 86 and the kernel, bound by occupancy over
// its dependent reads like k_scan, drops to 5.
__global__ __launch_bounds__(kScanWaves* kWave) __attribute__((amdgpu_waves_per_eu(6, 6))) void
k_rscan(ScanArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_page[kScanWaves][kRG * kPageDwords];
  const int lane = lane_id();
  const int wv = threadIdx.x >> 6;
  const int q = lane / kRL, li = lane % kRL;
  const uint64_t Q = ((uint64_t)blockIdx.x * kScanWaves + (uint64_t)wv) * kRG + (uint64_t)q;
  const bool has = Q < a.n;
  if (!ballot(has)) return;  // wave-uniform
  uint32_t* lp = s_page[wv] + q * kPageDwords;
  uint64_t* lk = reinterpret_cast<uint64_t*>(lp);  // the leaf's hit keys, once its page is unpacked
  const uint32_t limit = a.limit;
  uint64_t start = 0, stop = 0;
  if (has) {
    start = a.from[Q];
    if (a.to) stop = a.to[Q];
  }
  const uint64_t row = Q * (uint64_t)limit;  // the scan's row (written only for has, below limit)
  uint32_t err = 0;
  uint32_t cnt = 0;
  bool act = has && stop <= start;
  // the key whose leaf comes next, and the bound of that leaf's hits: the
  // start, then each leaf's lowest fence - 1.  No stored key equals kKeyMax,
  // and the last leaf holds kKeyMax - 1
  uint64_t cur = start == kKeyMax ? kKeyMax - 1 : start;

  const int ebase = chunk_base<kRE>(li);
  // every live scan of the wave takes one step per round, so the rounds
  // count each scan's steps: wave-uniform
  for (uint32_t steps = 0; ballot(act); ++steps) {
    uint32_t hw = kLeafCardinality;  // slots of this leaf that may be valid
    {
      // the descent's last round staged the leaf in the group's slot, so the
      // page registers end here
      RPage w;
      int hops = 0;  // per step: a long scan is not a long descent
      leaf_descend(a, act, cur, lp, li, w, hops, hw, err);
    }
    bool left = false;  // the scan goes on to the left, if the limit allows
    bool hit[kRE];
    uint64_t ek[kRE], ev[kRE];
#pragma unroll
    for (int j = 0; j < kRE; ++j) {
      hit[j] = false;
      ek[j] = 0;
      ev[j] = 0;
    }
    if (act) {
      const uint64_t lowest = hdr_lowest(lp);  // before the slot becomes the key list
      uint32_t D[kRCD];
      const uint32_t* ep = lp + (kOffRecords + kLeafEntry * ebase) / 4;
#pragma unroll
      for (int i = 0; i < kRCD; ++i) D[i] = ep[i];
      uint32_t ef[kRE], er[kRE];
      chunk_entries<kRE>(D, ek, ev, ef, er);
#pragma unroll
      for (int j = 0; j < kRE; ++j)
        hit[j] = ebase + j >= li * kRE && (uint32_t)(ebase + j) < hw && ev[j] != kValueNull &&
                 ((ef[j] ^ er[j]) & 0xF) == 0 && ek[j] >= stop && ek[j] <= cur;
      if (lowest > cur) {
        // cur is the last leaf's lowest fence - 1 (or the start): this leaf
        // does not lie at or below it, the step did not move left
        err |= kErrInconsistent;
      } else {
        left = lowest > stop && lowest != 0;
        cur = lowest - 1;
      }
    }
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kRE; ++j) c += hit[j] ? 1u : 0u;
    uint32_t tot;  // <= kLeafCardinality: every slot has one owner lane
    uint32_t idx = group_scan(c, li, &tot);
    wave_lds_sync();  // the page is in registers: its slot becomes the key list
#pragma unroll
    for (int j = 0; j < kRE; ++j)
      if (hit[j]) lk[idx++] = ek[j];
    if (li == 0 && (tot & 1u)) lk[tot] = 0;  // pads the last pair: above no key
    wave_lds_sync();
    uint32_t r[kRE] = {0, 0, 0, 0};
#pragma unroll 1  // as k_scan: unrolled, its loads in flight cost a wave per SIMD
    for (uint32_t m = 0; m < tot; m += 2) {
      const u64x2 km = *reinterpret_cast<const u64x2*>(lk + m);
#pragma unroll
      for (int j = 0; j < kRE; ++j)
        r[j] += (km.x > ek[j] ? 1u : 0u) + (km.y > ek[j] ? 1u : 0u);
    }
    uint32_t rs = 0;
#pragma unroll
    for (int j = 0; j < kRE; ++j) {
      if (hit[j]) {
        rs += r[j];
        const uint32_t pos = cnt + r[j];
        if (pos < limit) {
          a.keys[row + pos] = ek[j];
          a.vals[row + pos] = ev[j];
        }
      }
    }
    uint32_t rt;
    (void)group_scan(rs, li, &rt);
    if (rt * 2u != tot * (tot - 1u)) err |= kErrInconsistent;  // equal keys in one leaf
    cnt = cnt + tot < limit ? cnt + tot : limit;
    wave_lds_sync();  // LDS reads done before the next descent stages
    if (act && left && cnt < limit && steps >= (1u << 24)) {
      err |= kErrBadPtr;
      left = false;
    }
    act = act && left && cnt < limit;
  }
  if (has && li == 0) a.counts[Q] = cnt;
  if (err) {
    atomicOr(a.err, err);
    if (a.status) atomicOr(reinterpret_cast<unsigned long long*>(a.status + 1), (unsigned long long)err);
  }
}

namespace {
void launch_pieces(void (*kernel)(ScanArgs), const ScanArgs& a, hipStream_t s) {
  const uint64_t per = (uint64_t)kScanWaves * kRG;
  // a grid holds fewer than 2^31 blocks: longer batches in pieces
  const uint64_t piece = per << 26;
  for (uint64_t off = 0; off < a.n; off += piece) {
    ScanArgs b = a;
    b.n = a.n - off < piece ? a.n - off : piece;
    b.from = a.from + off;
    if (a.to) b.to = a.to + off;
    b.keys = a.keys + off * (uint64_t)a.limit;
    b.vals = a.vals + off * (uint64_t)a.limit;
    b.counts = a.counts + off;
    const dim3 grid((unsigned)((b.n + per - 1) / per)), block(kScanWaves * kWave);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, b);
  }
}
}  // namespace

void launch_scan(const ScanArgs& a, hipStream_t s) { launch_pieces(k_scan, a, s); }
void launch_rscan(const ScanArgs& a, hipStream_t s) { launch_pieces(k_rscan, a, s); }

}  // namespace dev
}  // namespace shm
