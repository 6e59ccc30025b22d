// order.hip — order statistics over the order index (shm_rank_batch,
// shm_count_batch, shm_select_batch): where a key stands in the key order,
// which pair stands at a position, and how many pairs a range holds, each from
// one search of the index and one read of a leaf (and of what hangs on it).
//
// The index (kernels.h OrderArgs; built by tree_order.cpp from the whole-tree
// count pass of the export) lists the tree's leaf units in key order: page[],
// bound[] (ascending, the last kKeyMax) and off[] (the valid pairs before the
// unit; off[units] = the total).  A key's rank is off[u] of the first unit
// whose bound is above it plus the valid keys below it in that unit; position
// r lives in the first unit with off[u + 1] > r, which skips empty units, whose
// off[u + 1] equals off[u], by the comparison itself.
//
// Search.  Both are "the first word above x" in an ascending array, answered
// through sampled levels (kOrdFan = 16: every 16th word, the last of each
// block, so a block's sample is its largest word).  From the one-block top
// level down, the query's 16 lanes read the block the level above chose, one
// word per lane (one 128 B line), and a ballot gives the first lane whose word
// is above x.  Every level is padded to whole blocks with ~0; a block index is
// clamped to the level's blocks, so an index that does not match itself cannot
// send a read outside the allocation.  The levels are plain HBM arrays: the
// upper ones are a few lines that every query reads and stay in L2.
//
// The leaf side has k_export_leaf's shape (export.hip: 16 lanes per query,
// four queries per wave, the page through registers into LDS, chunk_entries,
// leaf_hw ending the read at 768 B where it may, the compacted key list in the
// dead page slot and ranks from broadcast 16 B LDS reads) and its validity
// rule (value != kValueNull, front == rear entry version; src/Tree.cpp:461-540).
// The page helpers and leaf_load are page_group.h's.
//
// Bounds.  Every chain walk is bounded by the allocated pages (max_pages),
// every pointer by ptr_ok, a unit index by the unit count, and a page is read
// as a leaf only when its header says so.  Nothing here spins or waits for
// another block; the only atomics are the ORs into the error words.
#include "device_common.h"
#include "kernels.h"
#include "leaf_chunk.h"
#include "page_group.h"

namespace shm {
namespace dev {

namespace {
constexpr int kOWaves = 4;
static_assert(kOrdFan == kRL, "one index word per lane of a query's group");

// The index of the first word above x in level 0 of a pyramid, for the query
// of group q (x is the same in its 16 lanes); *ok = false when a block held no
// such word (the caller's x was not below the last word).  Every lane of the
// wave calls.
__device__ __forceinline__ uint64_t first_above(const uint64_t* const (&lv)[kOrdLevels],
                                                const OrderArgs& a, uint64_t x, int q, int li,
                                                bool* ok) {
  uint64_t idx = 0;
  bool good = true;
#pragma unroll
  for (int j = kOrdLevels - 1; j >= 0; --j) {
    if (j < (int)a.nlev) {  // wave-uniform
      const uint64_t blk = idx < a.nblk[j] ? idx : a.nblk[j] - 1;
      const uint64_t w = lv[j][blk * kOrdFan + (uint64_t)li];
      const uint32_t m = (uint32_t)(ballot(w > x) >> (kRL * q)) & 0xFFFFu;
      if (m == 0) good = false;
      idx = blk * kOrdFan + (uint64_t)(m ? __builtin_ctz(m) : 0);
    }
  }
  *ok = good;
  return idx;
}

// The valid keys below xa and below xb (xa <= xb) in the pages of unit
// (p, bound): the leaf, then its chain while the page's highest fence is below
// the unit's bound (the pages a missing separator left reachable through their
// left sibling alone) and below xb: a later page holds no key below its left
// neighbour's highest fence.  Every lane of the wave calls; act: the group has
// a unit to read.
__device__ __forceinline__ void walk_below(const OrderArgs& a, bool act, uint64_t p,
                                           uint64_t bound, uint64_t xa, uint64_t xb, uint32_t* lp,
                                           int li, uint64_t& ca, uint64_t& cb, uint32_t& err) {
  if (act && !ptr_ok(p, a.node, a.arena_bytes)) {
    err |= kErrBadPtr;
    act = false;
  }
  RPage w;
  uint32_t hw = kLeafCardinality;  // slots of the current leaf that may be valid
  if (act) leaf_load(a, p, li, w, hw);
  uint64_t hops = 0;
  const int ebase = chunk_base<kRE>(li);
  while (ballot(act)) {
    if (act) rstage(lp, li, w);
    wave_lds_sync();
    bool more = false;
    uint64_t sibling = 0;
    uint32_t c = 0;  // below xa in the low half, below xb in the high half
    if (act) {
      // read as a leaf only when its header says so
      if (hdr_leftmost(lp) != 0 || hdr_level(lp) != 0) {
        err |= kErrInconsistent;
        act = false;
      } else {
        sibling = hdr_sibling(lp);
        const uint64_t highest = hdr_highest(lp);
        more = sibling != 0 && highest < bound && highest < xb;
        if (more && (++hops >= a.max_pages || !ptr_ok(sibling, a.node, a.arena_bytes))) {
          err |= kErrBadPtr;
          more = false;
        }
        uint32_t D[kRCD];
        const uint32_t* ep = lp + (kOffRecords + kLeafEntry * ebase) / 4;
#pragma unroll
        for (int i = 0; i < kRCD; ++i) D[i] = ep[i];
        uint64_t ek[kRE], ev[kRE];
        uint32_t ef[kRE], er[kRE];
        chunk_entries<kRE>(D, ek, ev, ef, er);
#pragma unroll
        for (int j = 0; j < kRE; ++j) {
          const bool valid = ebase + j >= li * kRE && (uint32_t)(ebase + j) < hw &&
                             ev[j] != kValueNull && ((ef[j] ^ er[j]) & 0xF) == 0;
          c += (valid && ek[j] < xa ? 1u : 0u) + (valid && ek[j] < xb ? 0x10000u : 0u);
        }
      }
    }
    uint32_t tot;  // each half <= kLeafCardinality: every slot has one owner lane
    (void)group_scan(c, li, &tot);
    ca += (uint64_t)(tot & 0xFFFFu);
    cb += (uint64_t)(tot >> 16);
    wave_lds_sync();  // LDS reads done before the next stage
    if (act) {
      if (more) {
        // w is staged: its registers take the sibling's bytes
        leaf_load(a, sibling, li, w, hw);
      } else {
        act = false;
      }
    }
  }
}
}  // namespace

// out0[Q] = the valid pairs with key < in0[Q]
__global__ __launch_bounds__(kOWaves* kWave) void k_rank(OrderArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_page[kOWaves][kRG * kPageDwords];
  const int lane = lane_id();
  const int wv = threadIdx.x >> 6;
  const int q = lane / kRL, li = lane % kRL;
  const uint64_t Q = ((uint64_t)blockIdx.x * kOWaves + (uint64_t)wv) * kRG + (uint64_t)q;
  const bool has = Q < a.n;
  if (!ballot(has)) return;  // wave-uniform
  uint32_t* lp = s_page[wv] + q * kPageDwords;
  const uint64_t k = has ? a.in0[Q] : 0;
  uint32_t err = 0;
  // no stored key equals kKeyMax: every pair stands below it
  bool act = has && k != kKeyMax;
  bool ok;
  const uint64_t u = first_above(a.blv, a, act ? k : 0, q, li, &ok);
  if (act && (!ok || u >= a.units)) {
    err |= kErrInconsistent;  // the last bound is kKeyMax
    act = false;
  }
  uint64_t p = 0, bound = 0, base = 0;
  if (act) {
    p = a.page[u];
    bound = a.bound[u];
    base = a.off[u];
  }
  uint64_t ca = 0, cb = 0;
  walk_below(a, act, p, bound, k, k, lp, li, ca, cb, err);
  if (has && li == 0) a.out0[Q] = k == kKeyMax ? a.total : base + ca;
  if (err) {
    atomicOr(a.err, err);
    if (a.status) atomicOr(reinterpret_cast<unsigned long long*>(a.status + 1), (unsigned long long)err);
  }
}

// out0[Q] = the valid pairs with in0[Q] <= key <= in1[Q]: rank(to + 1) -
// rank(from), both ends by one group; ends inside one unit share its walk
__global__ __launch_bounds__(kOWaves* kWave) void k_count(OrderArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_page[kOWaves][kRG * kPageDwords];
  const int lane = lane_id();
  const int wv = threadIdx.x >> 6;
  const int q = lane / kRL, li = lane % kRL;
  const uint64_t Q = ((uint64_t)blockIdx.x * kOWaves + (uint64_t)wv) * kRG + (uint64_t)q;
  const bool has = Q < a.n;
  if (!ballot(has)) return;  // wave-uniform
  uint32_t* lp = s_page[wv] + q * kPageDwords;
  const uint64_t from = has ? a.in0[Q] : 0, to = has ? a.in1[Q] : 0;
  uint32_t err = 0;
  bool act = has && from <= to && from != kKeyMax;  // no stored key equals kKeyMax
  // the upper end is "below to + 1"; from to = kKeyMax - 1 on that is every pair
  const bool top = to >= kKeyMax - 1;
  const uint64_t x2 = top ? kKeyMax - 1 : to + 1;
  bool ok1, ok2;
  const uint64_t u1 = first_above(a.blv, a, act ? from : 0, q, li, &ok1);
  const uint64_t u2 = first_above(a.blv, a, act && !top ? x2 : 0, q, li, &ok2);
  if (act && (!ok1 || u1 >= a.units || (!top && (!ok2 || u2 >= a.units)))) {
    err |= kErrInconsistent;  // the last bound is kKeyMax
    act = false;
  }
  const bool same = !top && u1 == u2;
  uint64_t p = 0, bound = 0, base = 0;
  if (act) {
    p = a.page[u1];
    bound = a.bound[u1];
    base = a.off[u1];
  }
  uint64_t ca = 0, cb = 0;
  walk_below(a, act, p, bound, from, same ? x2 : from, lp, li, ca, cb, err);
  const uint64_t r1 = base + ca;
  uint64_t r2 = top ? a.total : base + cb;
  const bool two = act && !top && !same;
  if (two) {
    p = a.page[u2];
    bound = a.bound[u2];
    base = a.off[u2];
  }
  ca = cb = 0;
  walk_below(a, two, p, bound, x2, x2, lp, li, ca, cb, err);
  if (two) r2 = base + cb;
  if (has && li == 0) a.out0[Q] = act ? r2 - r1 : 0;
  if (err) {
    atomicOr(a.err, err);
    if (a.status) atomicOr(reinterpret_cast<unsigned long long*>(a.status + 1), (unsigned long long)err);
  }
}

// the pair at position in0[Q] of the key order: out0 = key, out1 = value,
// found = 1; past the end kKeyMax, 0 and 0 (each output nullable)
__global__ __launch_bounds__(kOWaves* kWave) void k_select(OrderArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_page[kOWaves][kRG * kPageDwords];
  const int lane = lane_id();
  const int wv = threadIdx.x >> 6;
  const int q = lane / kRL, li = lane % kRL;
  const uint64_t Q = ((uint64_t)blockIdx.x * kOWaves + (uint64_t)wv) * kRG + (uint64_t)q;
  const bool has = Q < a.n;
  if (!ballot(has)) return;  // wave-uniform
  uint32_t* lp = s_page[wv] + q * kPageDwords;
  uint64_t* lk = reinterpret_cast<uint64_t*>(lp);  // the leaf's valid keys, once its page is unpacked
  const uint64_t r = has ? a.in0[Q] : 0;
  uint32_t err = 0;
  bool act = has && r < a.total;
  bool ok;
  // the first unit with off[u + 1] > r: an empty unit's word equals its left
  // neighbour's and is never the first above r
  const uint64_t u = first_above(a.olv, a, act ? r : 0, q, li, &ok);
  if (act && (!ok || u >= a.units)) {
    err |= kErrInconsistent;  // r is below the total, the last word
    act = false;
  }
  uint64_t p = 0, bound = 0, rest = 0;
  if (act) {
    p = a.page[u];
    bound = a.bound[u];
    rest = r - a.off[u];
  }
  if (act && !ptr_ok(p, a.node, a.arena_bytes)) {
    err |= kErrBadPtr;
    act = false;
  }
  RPage w;
  uint32_t hw = kLeafCardinality;  // slots of the current leaf that may be valid
  if (act) leaf_load(a, p, li, w, hw);
  uint64_t hops = 0;
  bool done = false;
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
      // read as a leaf only when its header says so
      if (hdr_leftmost(lp) != 0 || hdr_level(lp) != 0) {
        err |= kErrInconsistent;
        act = false;
      } else {
        sibling = hdr_sibling(lp);
        const uint64_t highest = hdr_highest(lp);
        more = sibling != 0 && highest < bound;
        if (more && (++hops >= a.max_pages || !ptr_ok(sibling, a.node, a.arena_bytes))) {
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
                   ((ef[j] ^ er[j]) & 0xF) == 0;
      }
    }
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kRE; ++j) c += hit[j] ? 1u : 0u;
    uint32_t tot;  // <= kLeafCardinality: every slot has one owner lane
    uint32_t idx = group_scan(c, li, &tot);
    const bool here = act && rest < (uint64_t)tot;  // this page holds position r
    if (ballot(here)) {  // wave-uniform
      wave_lds_sync();  // the page is in registers: its slot becomes the key list
      if (here) {
#pragma unroll
        for (int j = 0; j < kRE; ++j)
          if (hit[j]) lk[idx++] = ek[j];
        if (li == 0 && (tot & 1u)) lk[tot] = kKeyMax;  // pads the last pair: below no key
      }
      wave_lds_sync();
      const uint32_t lim = here ? tot : 0u;
      uint32_t rk[kRE] = {0, 0, 0, 0};
#pragma unroll 1
      for (uint32_t m = 0; m < lim; m += 2) {
        const u64x2 km = *reinterpret_cast<const u64x2*>(lk + m);
#pragma unroll
        for (int j = 0; j < kRE; ++j)
          rk[j] += (km.x < ek[j] ? 1u : 0u) + (km.y < ek[j] ? 1u : 0u);
      }
      uint32_t rs = 0;
#pragma unroll
      for (int j = 0; j < kRE; ++j) {
        if (here && hit[j]) {
          rs += rk[j];
          if ((uint64_t)rk[j] == rest) {
            if (a.out0) a.out0[Q] = ek[j];
            if (a.out1) a.out1[Q] = ev[j];
            if (a.found) a.found[Q] = 1;
          }
        }
      }
      uint32_t rt;
      (void)group_scan(rs, li, &rt);
      if (here && rt * 2u != tot * (tot - 1u)) err |= kErrInconsistent;  // equal keys in one leaf
    }
    wave_lds_sync();  // LDS reads done before the next stage
    if (here) {
      done = true;
      act = false;
    } else if (act) {
      rest -= (uint64_t)tot;
      if (more) {
        // w is staged: its registers take the sibling's bytes
        leaf_load(a, sibling, li, w, hw);
      } else {
        err |= kErrInconsistent;  // the chain ended first: the index is not of these pages
        act = false;
      }
    }
  }
  if (has && !done && li == 0) {
    if (a.out0) a.out0[Q] = kKeyMax;
    if (a.out1) a.out1[Q] = 0;
    if (a.found) a.found[Q] = 0;
  }
  if (err) {
    atomicOr(a.err, err);
    if (a.status) atomicOr(reinterpret_cast<unsigned long long*>(a.status + 1), (unsigned long long)err);
  }
}

// one level of a pyramid from the level below: each block's last word
__global__ __launch_bounds__(256) void k_order_sample(const uint64_t* in, uint64_t n_in,
                                                      uint64_t* out, uint64_t n_out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_out) return;
  const uint64_t j = i * kOrdFan + (kOrdFan - 1);
  out[i] = in[j < n_in ? j : n_in - 1];
}

namespace {
void launch_pieces(void (*kernel)(OrderArgs), const OrderArgs& a, hipStream_t s) {
  const uint64_t per = (uint64_t)kOWaves * kRG;
  // a grid holds fewer than 2^31 blocks: longer batches in pieces
  const uint64_t piece = per << 26;
  for (uint64_t off = 0; off < a.n; off += piece) {
    OrderArgs b = a;
    b.n = a.n - off < piece ? a.n - off : piece;
    b.in0 = a.in0 + off;
    if (a.in1) b.in1 = a.in1 + off;
    if (a.out0) b.out0 = a.out0 + off;
    if (a.out1) b.out1 = a.out1 + off;
    if (a.found) b.found = a.found + off;
    const dim3 grid((unsigned)((b.n + per - 1) / per)), block(kOWaves * kWave);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, b);
  }
}
}  // namespace

void launch_order_rank(const OrderArgs& a, hipStream_t s) { launch_pieces(k_rank, a, s); }
void launch_order_count(const OrderArgs& a, hipStream_t s) { launch_pieces(k_count, a, s); }
void launch_order_select(const OrderArgs& a, hipStream_t s) { launch_pieces(k_select, a, s); }
void launch_order_sample(const uint64_t* in, uint64_t n_in, uint64_t* out, hipStream_t s) {
  if (n_in == 0) return;
  const uint64_t n_out = (n_in + kOrdFan - 1) / kOrdFan;
  hipLaunchKernelGGL(k_order_sample, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, in,
                     n_in, out, n_out);
}

}  // namespace dev
}  // namespace shm
