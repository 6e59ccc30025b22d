// range.hip — batched range scans: the intended Tree::range_query
// (src/Tree.cpp:461-540: every leaf overlapping [from, to] in key order via
// the sibling chain, valid entries in slot order, Tree.cpp:509-516).
//
// The count pass stages each scan's first stage_cap values; the fill pass
// then copies the scans that fit and walks only the longer ones again.
//
// Four scans per wave, 16 lanes per scan.  A scan is a chain of dependent
// page reads (start leaf, then its siblings), so a wave that walks one scan
// waits on one page at a time; four independent chains per wave put four
// times the page reads in flight at the same occupancy.  Lane li of scan
// group q reads 16 B chunks li, li + 16, li + 32, li + 48 of the group's
// page (256 B coalesced per group per load), stages them in the group's
// 1 KB LDS slot, and compares 4 consecutive 18 B entries (leaf_chunk.h).
// The start leaf comes from the leaf directory (or a descent from the
// covering internal page / the root: 4 separators per lane, the child is
// the count of separators <= from); B-link right turns fix a stale start.
// Along the leaf chain the sibling page is loaded into registers as soon as
// the current header says the scan continues, so its HBM latency overlaps
// the current leaf's compare and stores.  offsets == nullptr -> count only.
//
// The group's page helpers are page_group.h's.  The descent inside range_walk
// has a copy in scan.hip (leaf_descend): called from here instead, it changes
// k_range's register assignment, so it stays inline.
#include "device_common.h"
#include "dir_entry.h"
#include "kernels.h"
#include "leaf_chunk.h"
#include "page_group.h"

namespace shm {
namespace dev {

namespace {
constexpr int kRangeWaves = 4;
}  // namespace

// Walks one scan per group of the wave (act: the group has one) from the
// leaf directory / root down to lo's leaf and along the sibling chain to hi;
// its hit values in key order go to dst0[slot] for slot < cap0, then to
// dst1[slot - cap0] for the next cap1 slots (either nullable with cap 0).
// Returns the scan's value count.  Wave-uniform call (ballot loops); lp =
// the group's 1 KB LDS page slot.
__device__ __forceinline__ uint64_t range_walk(const RangeArgs& a, bool act, uint64_t lo,
                                               uint64_t hi, uint32_t* lp, int li, uint64_t* dst0,
                                               uint64_t cap0, uint64_t* dst1, uint64_t cap1,
                                               uint32_t& err) {
  uint64_t cnt = 0;
  // ---- descend to the leaf whose fences hold lo ------------------------------
  RPage w;
  uint64_t p = 0;
  int hops = 0;
  uint32_t hw = kLeafCardinality;  // slots of the current leaf that may be valid
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

  // ---- scan the leaf chain; w holds leaf p ------------------------------------
  // (a leaf's bytes past slot hw - 1 are not read)
  const int ebase = chunk_base<kRE>(li);
  while (ballot(act)) {
    if (act) rstage(lp, li, w);
    wave_lds_sync();
    bool more = false;
    uint64_t sibling = 0;
    uint32_t hwn = kLeafHwFull;
    // w is staged: its registers take the sibling's bytes (one page of
    // registers per lane, not two: 88 -> 77 VGPRs, 5 -> 6 waves per SIMD,
    // k_range 63.4 -> 62.7 us in the bench's profile pass.  Pages by LDS-DMA
    // instead, one slot per scan, measured 66.3: the slot refills only after
    // the page's compare, and the entry unpack still held 86 VGPRs)
    bool hit[kRE];
    uint64_t ev[kRE];
#pragma unroll
    for (int j = 0; j < kRE; ++j) {
      hit[j] = false;
      ev[j] = 0;
    }
    if (act) {
      sibling = hdr_sibling(lp);
      const uint64_t highest = hdr_highest(lp);
      more = sibling != 0 && highest <= hi;
      if (more) {
        if (++hops > (1 << 24) || !ptr_ok(sibling, a.node, a.arena_bytes)) {
          err |= kErrBadPtr;
          more = false;
        } else {
          // in flight: the sibling's bound (a 1.8 MB array, L2-resident) and
          // its first 768 bytes
          if (a.leaf_hw) hwn = a.leaf_hw[ga_offset(sibling) >> 10];
          rload3(a.arena, sibling, li, w);
        }
      }
      uint32_t D[kRCD];
      const uint32_t* ep = lp + (kOffRecords + kLeafEntry * ebase) / 4;
#pragma unroll
      for (int i = 0; i < kRCD; ++i) D[i] = ep[i];
      uint64_t ek[kRE];
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
    uint32_t tot;
    uint64_t slot = cnt + group_scan(c, li, &tot);
#pragma unroll
    for (int j = 0; j < kRE; ++j) {
      if (hit[j]) {
        if (slot < cap0)
          dst0[slot] = ev[j];
        else if (slot - cap0 < cap1)
          dst1[slot - cap0] = ev[j];
        ++slot;
      }
    }
    cnt += tot;
    wave_lds_sync();  // LDS reads done before the next stage
    if (act) {
      if (more) {
        if (hwn >= kChunk3Hw) rload_last(a.arena, sibling, li, w);
        hw = hwn < (uint32_t)kLeafCardinality ? hwn : (uint32_t)kLeafCardinality;
        p = sibling;
      } else {
        act = false;
      }
    }
  }
  return cnt;
}

__global__ __launch_bounds__(kRangeWaves* kWave) void k_range(RangeArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_page[kRangeWaves][kRG * kPageDwords];
  const int lane = lane_id();
  const int wv = threadIdx.x >> 6;
  const int q = lane / kRL, li = lane % kRL;
  const uint64_t Q = ((uint64_t)blockIdx.x * kRangeWaves + (uint64_t)wv) * kRG + (uint64_t)q;
  const bool has = Q < a.n;
  if (!ballot(has)) return;  // wave-uniform
  uint32_t* lp = s_page[wv] + q * kPageDwords;
  uint64_t lo = 0, hi = 0, out = 0;
  if (has) {
    lo = a.from[Q];
    hi = a.to[Q];
    if (a.offsets) out = a.offsets[Q];
  }
  uint32_t err = 0;
  uint64_t* stq = (a.stage && has) ? a.stage + Q * (uint64_t)a.stage_cap : nullptr;
  bool act = has && lo <= hi;
  bool copied = false;
  if (a.offsets && stq) {
    // fill pass, staged scan: copy its values out, no second walk
    const uint64_t c = a.counts[Q];
    copied = c <= a.stage_cap;
    if (copied) {
      for (uint64_t b = 0; b < c; b += kRL * 4) {
        uint64_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint64_t i = b + (uint64_t)(li + kRL * u);
          v[u] = i < c ? stq[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint64_t i = b + (uint64_t)(li + kRL * u);
          if (i < c && out + i < a.vals_cap) a.vals[out + i] = v[u];
        }
      }
      act = false;
    }
  }

  uint64_t* dst = stq;
  uint64_t cap = stq ? a.stage_cap : 0;
  if (a.offsets) {
    dst = a.vals + out;
    cap = out < a.vals_cap ? a.vals_cap - out : 0;
  }
  const uint64_t cnt = range_walk(a, act, lo, hi, lp, li, dst, cap, nullptr, 0, err);
  if (has && !copied && li == 0) {
    a.counts[Q] = cnt;
    if (a.status && cnt > a.stage_cap)
      atomicAdd(reinterpret_cast<unsigned long long*>(a.status), 1ull);
  }
  if (err) {
    atomicOr(a.err, err);
    if (a.status) atomicOr(reinterpret_cast<unsigned long long*>(a.status + 1), (unsigned long long)err);
  }
}

void launch_range(const RangeArgs& a, hipStream_t s) {
  if (!a.n) return;
  const uint64_t per = (uint64_t)kRangeWaves * kRG;
  hipLaunchKernelGGL(k_range, dim3((unsigned)((a.n + per - 1) / per)), dim3(kRangeWaves * kWave),
                     0, s, a);
}

}  // namespace dev
}  // namespace shm
