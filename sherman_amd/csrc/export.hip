// export.hip — every valid pair of a key range in ascending key order, in
// parallel passes (shm_export, shm_compact): what one shm_scan_batch(from = lo,
// to = hi) with an unbounded limit would return, without its serial walk over
// the sibling chain.  The traversal and the validity rule are
// Tree::range_query's (src/Tree.cpp:461-540: the leaf holding `lo`, then the
// sibling chain; value != kValueNull and front == rear entry version).
//
// The leaves of a grown tree lie in arbitrary page order and a leaf's slots are
// not sorted, so the passes are:
//
//  1. Top-down expansion, one level per step (k_export_expand).  A level's
//     work list holds units in key order; a unit is (page, upper bound of the
//     key range its parent gave it).  The root is the top level's only unit,
//     with bound kKeyMax.  One wave per unit reads the internal page, drops
//     the children whose range misses [lo, hi] and emits the others as units
//     of the level below: child i bounded by separator i + 1, the last child
//     by the page's highest fence.  Before it finishes, a unit follows its own
//     sibling chain while the page's highest fence is below the unit's bound:
//     those are the pages a missing separator left reachable through their
//     left sibling alone (the B-link state shm_insert_batch documents after
//     SHM_ENOMEM).  A count pass, an exclusive scan and an emit pass place the
//     children.
//  2. Leaf count pass (k_export_leaf<false>): per leaf unit, and per page of
//     its chain, the valid entries inside [lo, hi]; an exclusive scan over the
//     units; the host reads the grand total once.
//  3. Leaf write pass (k_export_leaf<true>): per leaf unit the hits are ranked
//     by key and (key, value) goes to offset + rank.
//
// The leaf kernel has k_scan's shape (scan.hip: 16 lanes per unit, four units
// per wave, the page through registers into LDS, chunk_entries, the hit keys
// compacted into the dead page slot, ranks from broadcast 16 B LDS reads); the
// page helpers and leaf_load are page_group.h's.
//
// The scan is three plain launches (per-tile sums, one block over the tile
// sums, per-tile offsets): no tile waits for another, so nothing here spins.
//
// Bounds.  Every chain walk is bounded by the allocated pages (max_pages),
// every emitted position by the list capacity (out_cap) or the counted total,
// every pointer by ptr_ok, and a page is read as a level-L page only when its
// header says so: a corrupt image ends with an error bit.
#include "device_common.h"
#include "page_io.h"
#include "kernels.h"
#include "leaf_chunk.h"
#include "page_group.h"

namespace shm {
namespace dev {

namespace {
constexpr int kXWaves = 4;
}  // namespace

// the top level's only unit
__global__ void k_export_seed(uint64_t root, uint64_t* page, uint64_t* bound) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    page[0] = root;
    bound[0] = kKeyMax;
  }
}

// One wave per unit of level a.level (>= 1).  EMIT = false: cnt[u] = the
// children of the unit's pages whose range meets [lo, hi]; EMIT = true: those
// children as units of the level below at out_page / out_bound [off[u] ...].
template <bool EMIT>
__global__ __launch_bounds__(kXWaves* kWave) void k_export_expand(ExportArgs a) {
  const int lane = lane_id();
  const uint64_t u = (uint64_t)blockIdx.x * kXWaves + (threadIdx.x >> 6);
  if (u >= a.n) return;  // wave-uniform
  uint64_t p = a.in_page[u];
  const uint64_t bound = a.in_bound[u];
  const uint64_t base = EMIT ? a.off[u] : 0;
  uint64_t count = 0;
  uint32_t err = 0;
  for (uint64_t hops = 0;; ++hops) {
    if (hops >= a.max_pages || !ptr_ok(p, a.node, a.arena_bytes)) {
      err |= kErrBadPtr;
      break;
    }
    const u32x4 w = load_page_slice(a.arena, ga_offset(p));
    const Hdr h = parse_hdr(w);
    // read as an internal page of this level only when its header says so
    if (h.leftmost == 0 || h.level != a.level || h.last_index < -1 ||
        h.last_index >= kInternalCardinality) {
      err |= kErrInconsistent;
      break;
    }
    const int nrec = h.last_index + 1;  // children 0 .. nrec
    const IntRec rec = internal_record(w);  // record j in lane j + 3
    // lane c takes child c: child 0 = leftmost from the lowest fence, child c
    // = record c - 1's pointer from its key; bounded by record c's key, the
    // last one by the highest fence
    const int c = lane;
    const uint64_t pk = shfl64(rec.key, (c + 2) & 63), pp = shfl64(rec.ptr, (c + 2) & 63);
    const uint64_t nk = shfl64(rec.key, (c + 3) & 63);
    const uint64_t cptr = c == 0 ? h.leftmost : pp;
    const uint64_t clow = c == 0 ? h.lowest : pk;
    const uint64_t cbound = c < nrec ? nk : h.highest;
    const bool keep = c <= nrec && cbound > a.lo && clow <= a.hi;
    const uint64_t mask = ballot(keep);
    if (EMIT && keep) {
      const uint64_t pos = base + count + (uint64_t)popc64(mask & lanemask_lt());
      if (pos < a.out_cap) {
        a.out_page[pos] = cptr;
        a.out_bound[pos] = cbound;
      } else {
        err |= kErrInconsistent;
      }
    }
    count += (uint64_t)popc64(mask);
    // pages a missing separator left reachable through this one alone
    if (h.sibling == 0 || h.highest >= bound || h.highest > a.hi) break;
    p = h.sibling;
  }
  if (!EMIT && lane == 0) a.cnt[u] = count;
  if (err) atomicOr(a.err, err);
}

// 16 lanes per leaf unit.  WRITE = false: cnt[u] = the valid entries inside
// [lo, hi] of the unit's leaf and of its chain; WRITE = true: those pairs in
// key order at keys / vals [off[u] ...] (either array nullable).
template <bool WRITE>
__global__ __launch_bounds__(kXWaves* kWave) void k_export_leaf(ExportArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_page[kXWaves][kRG * kPageDwords];
  const int lane = lane_id();
  const int wv = threadIdx.x >> 6;
  const int q = lane / kRL, li = lane % kRL;
  const uint64_t U = ((uint64_t)blockIdx.x * kXWaves + (uint64_t)wv) * kRG + (uint64_t)q;
  const bool has = U < a.n;
  if (!ballot(has)) return;  // wave-uniform
  uint32_t* lp = s_page[wv] + q * kPageDwords;
  uint64_t* lk = reinterpret_cast<uint64_t*>(lp);  // the leaf's hit keys, once its page is unpacked
  const uint64_t lo = a.lo, hi = a.hi;
  uint64_t p = 0, bound = 0, base = 0;
  if (has) {
    p = a.in_page[U];
    bound = a.in_bound[U];
    if (WRITE) base = a.off[U];
  }
  uint32_t err = 0;
  uint64_t cnt = 0;
  bool act = has;
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
        more = sibling != 0 && highest < bound && highest <= hi;
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
                   ((ef[j] ^ er[j]) & 0xF) == 0 && ek[j] >= lo && ek[j] <= hi;
      }
    }
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < kRE; ++j) c += hit[j] ? 1u : 0u;
    uint32_t tot;  // <= kLeafCardinality: every slot has one owner lane
    uint32_t idx = group_scan(c, li, &tot);
    if (WRITE) {
      wave_lds_sync();  // the page is in registers: its slot becomes the key list
#pragma unroll
      for (int j = 0; j < kRE; ++j)
        if (hit[j]) lk[idx++] = ek[j];
      if (li == 0 && (tot & 1u)) lk[tot] = kKeyMax;  // pads the last pair: below no key
      wave_lds_sync();
      uint32_t r[kRE] = {0, 0, 0, 0};
#pragma unroll 1
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
          const uint64_t pos = base + cnt + (uint64_t)r[j];
          if (pos < a.total) {  // the count pass's total: no store past the outputs
            if (a.keys) a.keys[pos] = ek[j];
            if (a.vals) a.vals[pos] = ev[j];
          } else {
            err |= kErrInconsistent;
          }
        }
      }
      uint32_t rt;
      (void)group_scan(rs, li, &rt);
      if (rt * 2u != tot * (tot - 1u)) err |= kErrInconsistent;  // equal keys in one leaf
    }
    cnt += (uint64_t)tot;
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
  if (!WRITE && has && li == 0) a.cnt[U] = cnt;
  if (err) atomicOr(a.err, err);
}

// ---- exclusive scan of u64 in three launches -------------------------------------
namespace {
constexpr int kXScanT = 256;                    // threads
constexpr int kXScanE = 4;                      // items per thread
constexpr uint64_t kXTile = kXScanT * kXScanE;  // items per block

// exclusive prefix of v over the block's threads (all call); *tot = block sum
__device__ __forceinline__ uint64_t block_scan_u64(uint64_t v, uint64_t* sh, uint64_t* tot) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < kXScanT; off <<= 1) {
    const uint64_t y = t >= off ? sh[t - off] : 0;
    __syncthreads();
    sh[t] += y;
    __syncthreads();
  }
  const uint64_t incl = sh[t];
  *tot = sh[kXScanT - 1];
  __syncthreads();  // sh may be reused
  return incl - v;
}
}  // namespace

__global__ __launch_bounds__(kXScanT) void k_export_sums(const uint64_t* in, uint64_t n,
                                                         uint64_t* bsum) {
  __shared__ uint64_t sh[kXScanT];
  const uint64_t i0 = (uint64_t)blockIdx.x * kXTile + (uint64_t)threadIdx.x * kXScanE;
  uint64_t v = 0;
#pragma unroll
  for (int j = 0; j < kXScanE; ++j)
    if (i0 + j < n) v += in[i0 + j];
  uint64_t tot;
  (void)block_scan_u64(v, sh, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
// one block: bsum[0, nb) becomes its exclusive scan; tot = {total, *err}
__global__ __launch_bounds__(kXScanT) void k_export_bscan(uint64_t* bsum, uint64_t nb,
                                                          uint64_t* tot, const uint32_t* err) {
  __shared__ uint64_t sh[kXScanT];
  uint64_t carry = 0;
  for (uint64_t b0 = 0; b0 < nb; b0 += kXScanT) {
    const uint64_t i = b0 + threadIdx.x;
    const uint64_t v = i < nb ? bsum[i] : 0;
    uint64_t t;
    const uint64_t ex = block_scan_u64(v, sh, &t);
    if (i < nb) bsum[i] = carry + ex;
    carry += t;
  }
  if (threadIdx.x == 0) {
    tot[0] = carry;
    tot[1] = (uint64_t)*err;
  }
}
__global__ __launch_bounds__(kXScanT) void k_export_offsets(const uint64_t* in, uint64_t n,
                                                            const uint64_t* bsum, uint64_t* out) {
  __shared__ uint64_t sh[kXScanT];
  const uint64_t i0 = (uint64_t)blockIdx.x * kXTile + (uint64_t)threadIdx.x * kXScanE;
  uint64_t x[kXScanE];
  uint64_t v = 0;
#pragma unroll
  for (int j = 0; j < kXScanE; ++j) {
    x[j] = i0 + j < n ? in[i0 + j] : 0;
    v += x[j];
  }
  uint64_t tot;
  uint64_t ex = bsum[blockIdx.x] + block_scan_u64(v, sh, &tot);
#pragma unroll
  for (int j = 0; j < kXScanE; ++j) {
    if (i0 + j < n) out[i0 + j] = ex;
    ex += x[j];
  }
}

uint64_t export_scan_tiles(uint64_t n) { return (n + kXTile - 1) / kXTile; }

void launch_export_seed(uint64_t root, uint64_t* page, uint64_t* bound, hipStream_t s) {
  hipLaunchKernelGGL(k_export_seed, dim3(1), dim3(kWave), 0, s, root, page, bound);
}
void launch_export_expand(const ExportArgs& a, bool emit, hipStream_t s) {
  if (a.n == 0) return;
  const dim3 grid((unsigned)((a.n + kXWaves - 1) / kXWaves)), block(kXWaves * kWave);
  if (emit)
    hipLaunchKernelGGL(k_export_expand<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(k_export_expand<false>, grid, block, 0, s, a);
}
void launch_export_leaf(const ExportArgs& a, bool write, hipStream_t s) {
  if (a.n == 0) return;
  const uint64_t per = (uint64_t)kXWaves * kRG;
  const dim3 grid((unsigned)((a.n + per - 1) / per)), block(kXWaves * kWave);
  if (write)
    hipLaunchKernelGGL(k_export_leaf<true>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(k_export_leaf<false>, grid, block, 0, s, a);
}
void launch_export_scan(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* bsum,
                        uint64_t* tot, const uint32_t* err, hipStream_t s) {
  const uint64_t nb = export_scan_tiles(n);
  if (nb) hipLaunchKernelGGL(k_export_sums, dim3((unsigned)nb), dim3(kXScanT), 0, s, in, n, bsum);
  hipLaunchKernelGGL(k_export_bscan, dim3(1), dim3(kXScanT), 0, s, bsum, nb, tot, err);
  if (nb)
    hipLaunchKernelGGL(k_export_offsets, dim3((unsigned)nb), dim3(kXScanT), 0, s, in, n, bsum, out);
}

}  // namespace dev
}  // namespace shm
