// route.hip — multi-GPU routing: what tree_route.cpp and shard*.cpp launch.
// A key's owning shard, stable bucketing by owner, the fixed-capacity get
// exchange, the routed insert's packing and the routed range scans' pieces,
// sums and assembly.
#include "device_common.h"
#include "kernels.h"
#include "seg_tile.h"  // segt::block_scan (k_range_sums)

namespace shm {
namespace dev {

namespace {
constexpr int kT = 256;
inline dim3 grid1(uint64_t n, int per = kT) {
  return dim3((unsigned)((n + per - 1) / per));
}
static_assert(kT == segt::kT, "segt::block_scan's block");
}  // namespace

// Equal slices (no splitters): shard s owns [s*2^64/P, (s+1)*2^64/P).
__device__ __forceinline__ uint32_t owner_of(uint64_t k, uint32_t shards) {
  return (uint32_t)__umul64hi(k, (uint64_t)shards);
}
constexpr int kRouteMaxShards = 64;
constexpr int kRoutePer = 4;  // keys per thread
constexpr int kRouteTile = kT * kRoutePer;

// Splitters (RouteSplit, kernels.h): shard p owns [s[p - 1], s[p]), so a key's
// owner is the number of splitters <= it.  The routing kernels are templates
// on how they find it; kOwnSlices is the code they were before splitters:
//   kOwnSlices : __umul64hi, no splitters anywhere
//   kOwnArgs   : P <= kRouteArgShards: compare-and-add over the splitters in
//                the kernel arguments (wave-uniform scalar loads, no LDS);
//                measured slower, kept selectable (own_mode)
//   kOwnLds    : the splitters copied to LDS once per block (padded with
//                kKeyMax to 64 words), a branchless binary search of
//                ceil(log2 P) steps: what every splitter launch uses
constexpr int kOwnSlices = 0, kOwnArgs = 1, kOwnLds = 2;
constexpr uint32_t kRouteArgShards = 16;

template <int M>
__device__ __forceinline__ uint64_t* split_lds() {
  if constexpr (M == kOwnLds) {
    __shared__ uint64_t s_split[kRouteMaxShards];
    return s_split;
  } else {
    return nullptr;
  }
}
// before the block's first __syncthreads (every routing kernel has one ahead
// of its first owner)
template <int M>
__device__ __forceinline__ void split_stage(uint64_t* lds, const RouteSplit& sp, uint32_t P) {
  if constexpr (M == kOwnLds) {
    if (threadIdx.x < (uint32_t)kRouteMaxShards)
      lds[threadIdx.x] = threadIdx.x + 1 < P ? sp.s[threadIdx.x] : kKeyMax;
  }
}
template <int M>
__device__ __forceinline__ uint32_t owner_by(uint64_t k, uint32_t P, const RouteSplit& sp,
                                             const uint64_t* lds) {
  if constexpr (M == kOwnSlices) {
    return owner_of(k, P);
  } else if constexpr (M == kOwnArgs) {
    uint32_t o = 0;
#pragma unroll
    for (uint32_t j = 0; j + 1 < kRouteArgShards; ++j) o += (j + 1 < P && sp.s[j] <= k) ? 1u : 0u;
    return o;
  } else {
    // the count of words <= k among the 2^nb - 1 first ones (ascending; the
    // padding counts only for k == kKeyMax, cut below)
    const int nb = P > 1 ? 32 - __clz((int)(P - 1)) : 0;
    uint32_t o = 0;
    for (uint32_t step = nb ? 1u << (nb - 1) : 0u; step; step >>= 1)
      o += lds[o + step - 1] <= k ? step : 0u;
    return o < P - 1 ? o : P - 1;
  }
}

// Stable bucketing by owner (keys_out keeps input order inside each shard,
// which insert routing needs for last-writer-in-batch-order semantics):
//   count   : per-tile shard counts            -> cm[tile][shard]
//   scan    : per shard, exclusive over tiles  -> cm = tile bases, counts_out
//   scatter : per tile, ranks in index order from wave ballots
//   (keymax, nullable: a routed insert's batch -- a kKeyMax key sets the
//   flag, and the scan then rejects the batch whole: every count 0, the
//   error bit kErrKeyMax, as a local insert rejects its chunk)
template <int M>
__device__ __forceinline__ void route_count(const uint64_t* __restrict__ keys, uint64_t n,
                                            uint32_t shards, uint32_t* __restrict__ cm,
                                            uint32_t* keymax, const RouteSplit& sp) {
  __shared__ uint32_t c[kRouteMaxShards];
  uint64_t* const sl = split_lds<M>();
  if (threadIdx.x < kRouteMaxShards) c[threadIdx.x] = 0;
  split_stage<M>(sl, sp, shards);
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kRouteTile;
  bool bad = false;
#pragma unroll
  for (int r = 0; r < kRoutePer; ++r) {
    const uint64_t i = base + (uint64_t)r * kT + threadIdx.x;
    if (i < n) {
      const uint64_t k = keys[i];
      bad |= k == kKeyMax;
      atomicAdd(&c[owner_by<M>(k, shards, sp, sl)], 1u);
    }
  }
  if (keymax && ballot(bad) && lane_id() == 0) atomicOr(keymax, 1u);
  __syncthreads();
  if (threadIdx.x < shards) cm[(uint64_t)blockIdx.x * shards + threadIdx.x] = c[threadIdx.x];
}
__global__ __launch_bounds__(kT) void k_route_count(const uint64_t* __restrict__ keys,
                                                    uint64_t n, uint32_t shards,
                                                    uint32_t* __restrict__ cm,
                                                    uint32_t* keymax) {
  route_count<kOwnSlices>(keys, n, shards, cm, keymax, RouteSplit{});
}
template <int M>
__global__ __launch_bounds__(kT) void k_route_count_b(const uint64_t* __restrict__ keys,
                                                      uint64_t n, uint32_t shards,
                                                      uint32_t* __restrict__ cm, uint32_t* keymax,
                                                      const RouteSplit sp) {
  route_count<M>(keys, n, shards, cm, keymax, sp);
}

__global__ __launch_bounds__(1024) void k_route_scan(uint32_t* __restrict__ cm, uint32_t tiles,
                                                     uint32_t shards,
                                                     uint64_t* __restrict__ counts_out,
                                                     uint32_t* keymax, uint32_t* err) {
  __shared__ uint32_t part[1024];
  __shared__ uint32_t off[kRouteMaxShards];
  const uint32_t t = threadIdx.x;
  const uint32_t Q = 1024 / shards;  // tile slices
  const uint32_t q = t / shards, sh = t % shards;
  const bool live = q < Q;
  const uint32_t b0 = live ? (uint32_t)(((uint64_t)tiles * q) / Q) : 0;
  const uint32_t b1 = live ? (uint32_t)(((uint64_t)tiles * (q + 1)) / Q) : 0;
  uint32_t sum = 0;
  for (uint32_t b = b0; b < b1; ++b) sum += cm[(uint64_t)b * shards + sh];
  if (live) part[q * shards + sh] = sum;
  __syncthreads();
  // per shard, inclusive scan of the slice sums over q (log2 Q steps)
  uint32_t incl = sum;
  for (uint32_t d = 1; d < Q; d <<= 1) {
    const uint32_t add = (live && q >= d) ? part[(q - d) * shards + sh] : 0u;
    __syncthreads();
    if (live) part[q * shards + sh] = (incl += add);
    __syncthreads();
  }
  if (live && q == Q - 1) off[sh] = incl;  // shard total for now
  __syncthreads();
  if (t == 0) {
    const bool reject = keymax && *keymax;
    if (reject) {
      *keymax = 0;
      atomicOr(err, kErrKeyMax);
    }
    uint32_t acc = 0;
    for (uint32_t x = 0; x < shards; ++x) {
      const uint32_t v = off[x];
      counts_out[x] = reject ? 0u : v;
      off[x] = acc;
      acc += v;
    }
  }
  __syncthreads();
  if (live) {
    uint32_t run = off[sh] + incl - sum;
    for (uint32_t b = b0; b < b1; ++b) {
      const uint64_t o = (uint64_t)b * shards + sh;
      const uint32_t v = cm[o];
      cm[o] = run;
      run += v;
    }
  }
}

template <int M>
__device__ __forceinline__ void route_scatter(const uint64_t* __restrict__ keys, uint64_t n,
                                              uint32_t shards, const uint32_t* __restrict__ cm,
                                              uint64_t* __restrict__ keys_out,
                                              uint32_t* __restrict__ perm, const RouteSplit& sp) {
  constexpr int kW = kT / kWave;
  __shared__ uint32_t wc[kRoutePer][kW][kRouteMaxShards];
  uint64_t* const sl = split_lds<M>();
  const int t = threadIdx.x, w = t >> 6, lane = lane_id();
  for (int j = t; j < kRoutePer * kW * kRouteMaxShards; j += kT) (&wc[0][0][0])[j] = 0;
  split_stage<M>(sl, sp, shards);
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kRouteTile;
  uint64_t kk[kRoutePer];
  uint32_t own[kRoutePer], rank[kRoutePer];
#pragma unroll
  for (int r = 0; r < kRoutePer; ++r) {
    const uint64_t i = base + (uint64_t)r * kT + t;
    const bool valid = i < n;
    kk[r] = valid ? keys[i] : 0;
    own[r] = valid ? owner_by<M>(kk[r], shards, sp, sl) : ~0u;
    rank[r] = 0;
    uint64_t pending = ballot(valid);
    while (pending) {  // one pass per distinct owner in this wave
      const uint32_t o = rl32(own[r], ctz64(pending));
      const uint64_t m = ballot(own[r] == o);
      if (own[r] == o) rank[r] = popc64(m & lanemask_lt());
      if (lane == 0) wc[r][w][o] = popc64(m);
      pending &= ~m;
    }
  }
  __syncthreads();
  if ((uint32_t)t < shards) {  // index order = (round, wave, lane)
    uint32_t run = cm[(uint64_t)blockIdx.x * shards + t];
    for (int r = 0; r < kRoutePer; ++r)
      for (int x = 0; x < kW; ++x) {
        const uint32_t v = wc[r][x][t];
        wc[r][x][t] = run;
        run += v;
      }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRoutePer; ++r) {
    if (own[r] == ~0u) continue;
    const uint32_t o = wc[r][w][own[r]] + rank[r];
    keys_out[o] = kk[r];
    perm[o] = (uint32_t)(base + (uint64_t)r * kT + t);
  }
}
__global__ __launch_bounds__(kT) void k_route_scatter(const uint64_t* __restrict__ keys,
                                                      uint64_t n, uint32_t shards,
                                                      const uint32_t* __restrict__ cm,
                                                      uint64_t* __restrict__ keys_out,
                                                      uint32_t* __restrict__ perm) {
  route_scatter<kOwnSlices>(keys, n, shards, cm, keys_out, perm, RouteSplit{});
}
template <int M>
__global__ __launch_bounds__(kT) void k_route_scatter_b(const uint64_t* __restrict__ keys,
                                                        uint64_t n, uint32_t shards,
                                                        const uint32_t* __restrict__ cm,
                                                        uint64_t* __restrict__ keys_out,
                                                        uint32_t* __restrict__ perm,
                                                        const RouteSplit sp) {
  route_scatter<M>(keys, n, shards, cm, keys_out, perm, sp);
}

uint64_t route_scratch_words(uint64_t n_max) {
  return ((n_max + kRouteTile - 1) / kRouteTile) * kRouteMaxShards;
}

// the form of the owner search for P shards with splitters: LDS unless the
// caller names the kernel-argument form (mode 1, P <= 16).  Placing 2^20 keys
// took 12.55 / 13.83 us from LDS against 13.08 / 14.12 us from the kernel
// arguments at P = 8 / 16 (equal slices: 12.0 / 13.1 us), and the bucketing
// 19.0 / 26.0 against 20.0 / 26.5 us (tools/route_bounds.py,
// profiles/route_bounds.json): the unrolled compares cost more issue slots
// than the three or four LDS reads they save
static int own_mode(uint32_t P, int mode) {
  return mode == kOwnArgs && P <= kRouteArgShards ? kOwnArgs : kOwnLds;
}

void launch_route_bucket(const uint64_t* keys, uint64_t n, uint32_t shards,
                         uint64_t* counts, uint64_t* keys_out, uint32_t* perm,
                         uint32_t* cm, uint32_t* keymax, uint32_t* err, hipStream_t s,
                         const RouteSplit* split, int mode) {
  const uint32_t tiles = (uint32_t)((n + kRouteTile - 1) / kRouteTile);
  const int m = split ? own_mode(shards, mode) : kOwnSlices;
  if (n) {
    if (m == kOwnSlices)
      hipLaunchKernelGGL(k_route_count, dim3(tiles), dim3(kT), 0, s, keys, n, shards, cm, keymax);
    else if (m == kOwnArgs)
      hipLaunchKernelGGL(k_route_count_b<kOwnArgs>, dim3(tiles), dim3(kT), 0, s, keys, n, shards,
                         cm, keymax, *split);
    else
      hipLaunchKernelGGL(k_route_count_b<kOwnLds>, dim3(tiles), dim3(kT), 0, s, keys, n, shards,
                         cm, keymax, *split);
  }
  hipLaunchKernelGGL(k_route_scan, dim3(1), dim3(1024), 0, s, cm, tiles, shards, counts, keymax,
                     err);
  if (n) {
    if (m == kOwnSlices)
      hipLaunchKernelGGL(k_route_scatter, dim3(tiles), dim3(kT), 0, s, keys, n, shards,
                         (const uint32_t*)cm, keys_out, perm);
    else if (m == kOwnArgs)
      hipLaunchKernelGGL(k_route_scatter_b<kOwnArgs>, dim3(tiles), dim3(kT), 0, s, keys, n, shards,
                         (const uint32_t*)cm, keys_out, perm, *split);
    else
      hipLaunchKernelGGL(k_route_scatter_b<kOwnLds>, dim3(tiles), dim3(kT), 0, s, keys, n, shards,
                         (const uint32_t*)cm, keys_out, perm, *split);
  }
}

// out[i] = in[perm[i]] (apply the bucket permutation to a companion array)
__global__ void k_permute(const uint64_t* in, const uint32_t* perm, uint64_t n,
                          uint64_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[perm[i]];
}
void launch_permute(const uint64_t* in, const uint32_t* perm, uint64_t n, uint64_t* out,
                    hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_permute, grid1(n), dim3(kT), 0, s, in, perm, n, out);
}

// found (nullable): found[perm[i]] = in[i] != kValueNull (Tree.cpp:445-448)
__global__ void k_unpermute(const uint64_t* in, const uint32_t* perm,
                            uint64_t n, uint64_t* out, uint8_t* found) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint64_t v = in[i];
    const uint32_t p = perm[i];
    out[p] = v;
    if (found) found[p] = v != kValueNull ? 1 : 0;
  }
}
void launch_unpermute(const uint64_t* in, const uint32_t* perm, uint64_t n,
                      uint64_t* out, uint8_t* found, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_unpermute, grid1(n), dim3(kT), 0, s, in, perm, n, out, found);
}

// ---- fixed-capacity get exchange (shard.cpp): no host-known counts ------------
// Peer p's keys go to slot run [p * cap, (p + 1) * cap) of the send buffer,
// the rest of the run kKeyMax (a get of kKeyMax finds nothing).  A key's
// place in its run comes from a per-peer cursor (one atomic per peer present
// in a block), so no bucketing pass, scan or pack is needed; the order inside
// a run does not matter, since spos[i] records where input i went and the
// results are gathered back from the same places.  cursor[p] ends as the
// number of keys routed to peer p (a run's overflow included), cursor[P] as
// the number of overflowed keys.
// kKeyMax padding of the P runs of cap slots (run `own` in own_out when
// non-null) and the cursors zeroed
__global__ __launch_bounds__(kT) void k_route_fill(uint64_t* out, uint64_t cap, uint32_t* cursor,
                                                   uint32_t P, uint32_t own, uint64_t* own_out) {
  const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
  if (i == 0)
    for (uint32_t p = 0; p <= P; ++p) cursor[p] = 0;
  if (i >= (uint64_t)P * cap) return;
  const uint32_t p = (uint32_t)(i / cap);
  if (own_out && p == own)
    own_out[i - (uint64_t)p * cap] = kKeyMax;
  else
    out[i] = kKeyMax;
}

// A block of 1024 threads places 4096 keys (4 per thread): per round and
// wave, ranks among the lanes of one owner by ballots (as k_route_scatter);
// per owner, ONE global claim for the whole block.  Sixteen waves per block,
// four per SIMD (round 5's 256-thread blocks of 16 keys per thread left one
// wave per SIMD waiting on its loads and its block's claim).  The claim words
// sit on lines of their own (ctr, kCtrStride words apart): a returning
// device-scope atomic on one word saturates at ~88 per us (MI355X_MICROARCH
// "dequeue"), and the 2048 claims of a 2^20-key batch at P = 8 on one line
// took ~20 us (tools/route_p8.py); per line they are 256.  The last block
// to finish copies the counts to cursor[0..P] (P runs, then the overflow
// count: what the exchange and the host read) and returns the claim words
// to zero, so no launch resets them.
// A key past its run's capacity goes to the overflow list (ovk[j] = key,
// ovi[j] = its input position; one claim per wave and round) and the
// shard's second round returns its value (shard.cpp); without an overflow
// list (ovk == nullptr) it finds nothing and kErrOverflow is reported.
constexpr int kSlotT = 1024;

template <int kSlotPer, int M>
__device__ __forceinline__ void route_slots(const uint64_t* __restrict__ keys, uint64_t n,
                                            uint32_t P, uint64_t cap,
                                            uint32_t* __restrict__ cursor,
                                            uint32_t* __restrict__ ctr, uint64_t* __restrict__ out,
                                            uint32_t* __restrict__ spos, uint64_t* ovk,
                                            uint32_t* ovi, uint32_t* err, uint32_t own_p,
                                            uint64_t* own_out, const RouteSplit& sp) {
  constexpr int kW = kSlotT / kWave;
  constexpr int kSlotTile = kSlotT * kSlotPer;
  __shared__ uint32_t wc[kSlotPer][kW][kRouteMaxShards];
  __shared__ uint32_t last;
  uint64_t* const sl = split_lds<M>();
  const int t = threadIdx.x, w = t >> 6, lane = lane_id();
  for (int j = t; j < kSlotPer * kW * kRouteMaxShards; j += kSlotT) (&wc[0][0][0])[j] = 0;
  split_stage<M>(sl, sp, P);
  const uint64_t base = (uint64_t)blockIdx.x * kSlotTile;
  uint64_t kk[kSlotPer];
#pragma unroll
  for (int r = 0; r < kSlotPer; ++r) {
    const uint64_t i = base + (uint64_t)r * kSlotT + t;
    kk[r] = i < n ? keys[i] : 0;
  }
  __syncthreads();
  // ranks among the wave's lanes of one owner from the owner's bit planes:
  // one ballot per bit (3 at P = 8), each lane keeping the lanes that agree
  // with its owner on every bit, and lane o < P the lanes whose owner is o
  // (its count).  A pass per owner present in the wave (readlane, ballot,
  // LDS store per pass) took 5-6 of the kernel's 12.4 us at P = 8
  // (tools/route_p8.py, the passes skipped: 6.8 us)
  const int nb = P > 1 ? 32 - __clz((int)(P - 1)) : 0;
  uint32_t own[kSlotPer], rank[kSlotPer];
#pragma unroll
  for (int r = 0; r < kSlotPer; ++r) {
    const bool valid = base + (uint64_t)r * kSlotT + t < n;
    own[r] = valid ? owner_by<M>(kk[r], P, sp, sl) : ~0u;
    const uint64_t vm = ballot(valid);
    uint64_t mine = vm, mine_o = vm;
    for (int b = 0; b < nb; ++b) {
      const uint64_t bb = ballot(valid && ((own[r] >> b) & 1u));
      mine &= ((own[r] >> b) & 1u) ? bb : ~bb;
      mine_o &= ((lane >> b) & 1) ? bb : ~bb;
    }
    rank[r] = valid ? popc64(mine & lanemask_lt()) : 0u;
    if ((uint32_t)lane < P) wc[r][w][lane] = popc64(mine_o);
  }
  __syncthreads();
  // one wave per owner: its 64 (round, wave) counts scanned across the
  // lanes, the block's one claim on the owner's run, the bases written back
  // (a thread per owner summing them in turn spent ~3 us in LDS latency)
  constexpr int kQ = kSlotPer * kW;  // (round, wave) counts per owner
  static_assert(kQ < kWave || kQ % kWave == 0, "whole lanes per (round, wave)");
  constexpr int kE = kQ >= kWave ? kQ / kWave : 1;  // per lane
  for (uint32_t p = (uint32_t)w; p < P; p += kW) {
    uint32_t v[kE], sum = 0;
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      const int q = lane * kE + e;
      v[e] = q < kQ ? wc[q / kW][q % kW][p] : 0u;
      sum += v[e];
    }
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)incl, off);
      if (lane >= off) incl += y;
    }
    const uint32_t tot = rl32(incl, kWave - 1);
    uint32_t run = 0;
    if (lane == 0 && tot) run = atomicAdd(ctr + p * kCtrStride, tot);
    run = rl32(run, 0) + incl - sum;
#pragma unroll
    for (int e = 0; e < kE; ++e) {
      const int q = lane * kE + e;
      if (q < kQ) wc[q / kW][q % kW][p] = run;
      run += v[e];
    }
  }
  __syncthreads();
  bool over = false;
#pragma unroll
  for (int r = 0; r < kSlotPer; ++r) {
    const uint64_t i = base + (uint64_t)r * kSlotT + t;
    bool ov = false;
    if (own[r] != ~0u) {
      const uint32_t pos = wc[r][w][own[r]] + rank[r];
      if (pos < cap) {
        const uint64_t x = (uint64_t)own[r] * cap + pos;
        if (own_out && own[r] == own_p)
          own_out[pos] = kk[r];  // this rank's run: straight to the local get
        else
          out[x] = kk[r];
        spos[i] = (uint32_t)x;
      } else {  // this peer's run is full
        spos[i] = ~0u;
        ov = true;
      }
    }
    const uint64_t om = ballot(ov);  // wave-uniform
    if (om && ovk) {
      uint32_t ob = 0;
      if (lane == 0) ob = atomicAdd(ctr + P * kCtrStride, (uint32_t)popc64(om));
      ob = rl32(ob, 0);
      if (ov) {
        const uint32_t j = ob + (uint32_t)popc64(om & lanemask_lt());
        ovk[j] = kk[r];
        ovi[j] = (uint32_t)i;
      }
    }
    over |= ov;
  }
  if (over && !ovk) atomicOr(err, kErrOverflow);
  // every claim of this block returned: the last block publishes the counts
  __syncthreads();
  if (t == 0) last = atomicAdd(ctr + (P + 1) * kCtrStride, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (last && (uint32_t)t <= P + 1) {
    // read and reset in one atomic, at the point every claim went through
    const uint32_t v = atomicExch(ctr + t * kCtrStride, 0u);
    if ((uint32_t)t <= P) cursor[t] = v;
  }
}
template <int kSlotPer>
__global__ __launch_bounds__(kSlotT) void k_route_slots(const uint64_t* __restrict__ keys,
                                                        uint64_t n, uint32_t P, uint64_t cap,
                                                        uint32_t* __restrict__ cursor,
                                                        uint32_t* __restrict__ ctr,
                                                        uint64_t* __restrict__ out,
                                                        uint32_t* __restrict__ spos, uint64_t* ovk,
                                                        uint32_t* ovi, uint32_t* err, uint32_t own_p,
                                                        uint64_t* own_out) {
  route_slots<kSlotPer, kOwnSlices>(keys, n, P, cap, cursor, ctr, out, spos, ovk, ovi, err, own_p,
                                    own_out, RouteSplit{});
}
template <int kSlotPer, int M>
__global__ __launch_bounds__(kSlotT) void k_route_slots_b(const uint64_t* __restrict__ keys,
                                                          uint64_t n, uint32_t P, uint64_t cap,
                                                          uint32_t* __restrict__ cursor,
                                                          uint32_t* __restrict__ ctr,
                                                          uint64_t* __restrict__ out,
                                                          uint32_t* __restrict__ spos,
                                                          uint64_t* ovk, uint32_t* ovi,
                                                          uint32_t* err, uint32_t own_p,
                                                          uint64_t* own_out, const RouteSplit sp) {
  route_slots<kSlotPer, M>(keys, n, P, cap, cursor, ctr, out, spos, ovk, ovi, err, own_p, own_out,
                           sp);
}

// fill: pad the runs with kKeyMax first (a slot's first batch, or one whose
// capacity changed); otherwise the runs' tails keep the keys an earlier
// batch placed there at the same capacity -- keys of the same owner's
// range, searched and never gathered, exactly as padding.  ctr: (P + 2) *
// kCtrStride words, zero at rest (route_ctr_words)
void launch_route_slots(const uint64_t* keys, uint64_t n, uint32_t P, uint64_t cap,
                        uint32_t* cursor, uint32_t* ctr, uint64_t* out, uint32_t* spos,
                        uint64_t* ovk, uint32_t* ovi, uint32_t* err, hipStream_t s, uint32_t own,
                        uint64_t* own_out, bool fill, const RouteSplit* split, int mode) {
  const uint64_t slots = (uint64_t)P * cap;
  if (fill)
    hipLaunchKernelGGL(k_route_fill, grid1(slots + 1), dim3(kT), 0, s, out, cap, cursor, P, own,
                       own_out);
  // four keys per thread: 256 blocks for 2^20 keys (one or two keys per
  // thread, or eight, measured no better at P = 8: tools/route_p8.py)
  const int m = split ? own_mode(P, mode) : kOwnSlices;
  if (n && m == kOwnSlices)
    hipLaunchKernelGGL(k_route_slots<4>, grid1(n, kSlotT * 4), dim3(kSlotT), 0, s, keys, n, P,
                       cap, cursor, ctr, out, spos, ovk, ovi, err, own, own_out);
  else if (n && m == kOwnArgs)
    hipLaunchKernelGGL((k_route_slots_b<4, kOwnArgs>), grid1(n, kSlotT * 4), dim3(kSlotT), 0, s,
                       keys, n, P, cap, cursor, ctr, out, spos, ovk, ovi, err, own, own_out, *split);
  else if (n)
    hipLaunchKernelGGL((k_route_slots_b<4, kOwnLds>), grid1(n, kSlotT * 4), dim3(kSlotT), 0, s,
                       keys, n, P, cap, cursor, ctr, out, spos, ovk, ovi, err, own, own_out, *split);
  else if (!fill)
    (void)hipMemsetAsync(cursor, 0, sizeof(uint32_t) * (P + 1), s);
}

// out[i] = in[spos[i]] (0 for a key cut by a full run: the overflow round
// fills it afterwards), found[i] = out[i] != 0 (Tree.cpp:445-448).  Four
// inputs per thread when the buffers allow 16 B accesses: one spos load, four
// gathers in flight, two 16 B value stores and one 4 B found store
__device__ __forceinline__ uint64_t gather_one(const uint64_t* in, uint32_t x, uint64_t own_lo,
                                               uint64_t cap, const uint64_t* own_src) {
  if (x == ~0u) return kValueNull;
  return own_src && x - own_lo < cap ? own_src[x] : in[x];
}
__global__ void k_route_gather(const uint64_t* in, const uint32_t* spos, uint64_t n,
                               uint64_t* out, uint8_t* found, uint64_t own_lo, uint64_t cap,
                               const uint64_t* own_src) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t v = gather_one(in, spos[i], own_lo, cap, own_src);
  out[i] = v;
  if (found) found[i] = v != kValueNull ? 1 : 0;
}
__global__ void k_route_gather4(const uint64_t* in, const uint32_t* spos, uint64_t n4,
                                uint64_t* out, uint8_t* found, uint64_t own_lo, uint64_t cap,
                                const uint64_t* own_src) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n4) return;
  const uint4 x = reinterpret_cast<const uint4*>(spos)[j];
  const uint64_t v0 = gather_one(in, x.x, own_lo, cap, own_src);
  const uint64_t v1 = gather_one(in, x.y, own_lo, cap, own_src);
  const uint64_t v2 = gather_one(in, x.z, own_lo, cap, own_src);
  const uint64_t v3 = gather_one(in, x.w, own_lo, cap, own_src);
  ulonglong2* o = reinterpret_cast<ulonglong2*>(out) + 2 * j;
  o[0] = make_ulonglong2(v0, v1);
  o[1] = make_ulonglong2(v2, v3);
  if (found)
    reinterpret_cast<uint32_t*>(found)[j] = (v0 != kValueNull ? 1u : 0u) |
                                            (v1 != kValueNull ? 1u << 8 : 0u) |
                                            (v2 != kValueNull ? 1u << 16 : 0u) |
                                            (v3 != kValueNull ? 1u << 24 : 0u);
}
void launch_route_gather(const uint64_t* in, const uint32_t* spos, uint64_t n, uint64_t* out,
                         uint8_t* found, hipStream_t s, uint32_t own, uint64_t cap,
                         const uint64_t* own_src) {
  if (!n) return;
  const uint64_t lo = (uint64_t)own * cap;
  const bool vec = ((reinterpret_cast<uintptr_t>(spos) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(found) & 3) == 0;
  const uint64_t n4 = vec ? n / 4 : 0;
  if (n4)
    hipLaunchKernelGGL(k_route_gather4, grid1(n4), dim3(kT), 0, s, in, spos, n4, out, found, lo,
                       cap, own_src);
  if (n > 4 * n4)
    hipLaunchKernelGGL(k_route_gather, grid1(n - 4 * n4), dim3(kT), 0, s, in, spos + 4 * n4,
                       n - 4 * n4, out + 4 * n4, found ? found + 4 * n4 : nullptr, lo, cap,
                       own_src);
}

// the overflow round's results: out[ovi[perm[j]]] = in[j] (perm: the
// overflow list's bucketing permutation), found likewise
__global__ void k_route_ov_scatter(const uint64_t* in, const uint32_t* perm, const uint32_t* ovi,
                                   uint64_t m, uint64_t* out, uint8_t* found) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const uint32_t i = ovi[perm[j]];
  const uint64_t v = in[j];
  out[i] = v;
  if (found) found[i] = v != kValueNull ? 1 : 0;
}
void launch_route_ov_scatter(const uint64_t* in, const uint32_t* perm, const uint32_t* ovi,
                             uint64_t m, uint64_t* out, uint8_t* found, hipStream_t s) {
  if (m)
    hipLaunchKernelGGL(k_route_ov_scatter, grid1(m), dim3(kT), 0, s, in, perm, ovi, m, out, found);
}

// Routed insert: the stably bucketed keys (and values) of peer p, run
// [sum(cnt[< p]), + cnt[p]), packed into slot run [p * cap, (p + 1) * cap):
// the first min(cnt[p], cap) in bucket (= input) order, the rest kKeyMax
// padding (the receiver's insert skips it).  The overflow (cnt[p] > cap)
// stays in kb / vb for the shard's second round.
__global__ __launch_bounds__(kT) void k_route_pack(const uint64_t* kb, const uint64_t* vb,
                                                   const uint64_t* cnt, uint32_t P, uint64_t cap,
                                                   uint64_t* pk, uint64_t* pv, uint32_t own,
                                                   uint64_t* own_k, uint64_t* own_v) {
  const uint64_t x = (uint64_t)blockIdx.x * kT + threadIdx.x;
  if (x >= (uint64_t)P * cap) return;
  const uint32_t p = (uint32_t)(x / cap);
  const uint64_t j = x - (uint64_t)p * cap;
  uint64_t off = 0;
  for (uint32_t q = 0; q < p; ++q) off += cnt[q];
  const bool real = j < cnt[p];
  const bool mine = own_k && p == own;  // this rank's run: straight to the local insert
  (mine ? own_k + j : pk + x)[0] = real ? kb[off + j] : kKeyMax;
  (mine ? own_v + j : pv + x)[0] = real ? vb[off + j] : kValueNull;
}
void launch_route_pack(const uint64_t* kb, const uint64_t* vb, const uint64_t* cnt, uint32_t P,
                       uint64_t cap, uint64_t* pk, uint64_t* pv, hipStream_t s, uint32_t own,
                       uint64_t* own_k, uint64_t* own_v) {
  const uint64_t slots = (uint64_t)P * cap;
  if (slots)
    hipLaunchKernelGGL(k_route_pack, grid1(slots), dim3(kT), 0, s, kb, vb, cnt, P, cap, pk, pv,
                       own, own_k, own_v);
}

// ---- routed range scans (shard.cpp shm_shard_range_query) -------------------
// Piece (p, j) of the P x cap piece matrix = scan j's overlap with shard p,
// [max(from, lo_p), min(to, hi_p)], or empty (1, 0) where it misses the shard
// (or j >= n); row p goes to rank p.  bnd: shard p owns [bnd[p], bnd[p + 1]),
// bnd[P] = 0 standing for 2^64.
__global__ __launch_bounds__(kT) void k_range_pieces(const uint64_t* from, const uint64_t* to,
                                                     uint64_t n, uint64_t cap, uint32_t P,
                                                     ShardBounds bnd, uint64_t* plo,
                                                     uint64_t* phi) {
  const uint64_t x = (uint64_t)blockIdx.x * kT + threadIdx.x;
  if (x >= (uint64_t)P * cap) return;
  const uint32_t p = (uint32_t)(x / cap);
  const uint64_t j = x - (uint64_t)p * cap;
  uint64_t lo = 1, hi = 0;
  if (j < n) {
    const uint64_t f = from[j], t = to[j];
    const uint64_t slo = bnd.b[p];
    const uint64_t shi = p + 1 < P ? bnd.b[p + 1] - 1 : kKeyMax;  // inclusive top
    // repeated splitters: shard [x, x) owns nothing (its top would wrap for x = 0)
    const bool none = p + 1 < P && bnd.b[p + 1] <= slo;
    if (!none && f <= t && f <= shi && t >= slo) {
      lo = f > slo ? f : slo;
      hi = t < shi ? t : shi;
    }
  }
  plo[x] = lo;
  phi[x] = hi;
}
void launch_range_pieces(const uint64_t* from, const uint64_t* to, uint64_t n, uint64_t cap,
                         uint32_t P, const ShardBounds& bnd, uint64_t* plo, uint64_t* phi,
                         hipStream_t s) {
  const uint64_t m = (uint64_t)P * cap;
  if (m) hipLaunchKernelGGL(k_range_pieces, grid1(m), dim3(kT), 0, s, from, to, n, cap, P, bnd, plo, phi);
}

// Sums after the counts came back: blocks [0, P) sum row r of rc (the values
// this rank, as scanner, sends rank r) into rw[r]; blocks [P, 2P) row p of
// bc (the values it receives from shard p) into rw[P + p]; the rest give
// counts[j] = sum over p of bc[p][j] for j < n (scan j's total).
__global__ __launch_bounds__(kT) void k_range_sums(const uint64_t* rc, const uint64_t* bc,
                                                   uint64_t n, uint64_t cap, uint32_t P,
                                                   uint64_t* rw, uint64_t* counts) {
  const uint32_t b = blockIdx.x;
  if (b < 2 * P) {
    const uint64_t* row = (b < P ? rc : bc) + (uint64_t)(b % P) * cap;
    uint64_t v = 0;
    for (uint64_t j = threadIdx.x; j < cap; j += kT) v += row[j];
    uint64_t tot;
    (void)segt::block_scan<uint64_t>(v, &tot);
    if (threadIdx.x == 0) rw[b] = tot;
    return;
  }
  const uint64_t j = (uint64_t)(b - 2 * P) * kT + threadIdx.x;
  if (j >= n) return;
  uint64_t c = 0;
  for (uint32_t p = 0; p < P; ++p) c += bc[(uint64_t)p * cap + j];
  counts[j] = c;
}
void launch_range_sums(const uint64_t* rc, const uint64_t* bc, uint64_t n, uint64_t cap,
                       uint32_t P, uint64_t* rw, uint64_t* counts, hipStream_t s) {
  const uint32_t blocks = 2 * P + (uint32_t)((n + kT - 1) / kT);
  hipLaunchKernelGGL(k_range_sums, dim3(blocks), dim3(kT), 0, s, rc, bc, n, cap, P, rw, counts);
}

// Scan j's values, in shard order (= key order across shards): piece (p, j)
// holds bc[p][j] values at bv[bsc[p][j]] (bsc: exclusive scan of bc in
// row-major order, the layout of the received value runs; pitch != 0: row
// p's run starts at bv[p * pitch] and holds at most pitch values, the
// exchange without a host read-back); they go to vals[offsets[j] + sum of
// its earlier pieces], values past vals_cap dropped.  One wave per scan.
__global__ __launch_bounds__(kT) void k_range_assemble(const uint64_t* bv, const uint64_t* bc,
                                                       const uint64_t* bsc, uint64_t n,
                                                       uint64_t cap, uint32_t P,
                                                       const uint64_t* offsets, uint64_t* vals,
                                                       uint64_t vals_cap, uint64_t pitch) {
  const uint64_t j = ((uint64_t)blockIdx.x * kT + threadIdx.x) / kWave;
  if (j >= n) return;
  const int lane = lane_id();
  uint64_t dst = offsets[j];
  for (uint32_t p = 0; p < P; ++p) {
    const uint64_t c = bc[(uint64_t)p * cap + j];
    const uint64_t x = bsc[(uint64_t)p * cap + j];
    // pitched: the piece's place inside row p's run, cut at the run's end
    const uint64_t rel = pitch ? x - bsc[(uint64_t)p * cap] : 0;
    const uint64_t src = pitch ? (uint64_t)p * pitch + rel : x;
    const uint64_t cc = pitch ? (rel >= pitch ? 0 : c < pitch - rel ? c : pitch - rel) : c;
    for (uint64_t k = (uint64_t)lane; k < cc; k += kWave)
      if (dst + k < vals_cap) vals[dst + k] = bv[src + k];
    dst += c;
  }
}
void launch_range_assemble(const uint64_t* bv, const uint64_t* bc, const uint64_t* bsc,
                           uint64_t n, uint64_t cap, uint32_t P, const uint64_t* offsets,
                           uint64_t* vals, uint64_t vals_cap, hipStream_t s, uint64_t pitch) {
  if (n)
    hipLaunchKernelGGL(k_range_assemble, grid1(n * kWave), dim3(kT), 0, s, bv, bc, bsc, n, cap, P,
                       offsets, vals, vals_cap, pitch);
}

// The routed scan's value exchange without a host read-back: the scanner's
// packed values (row p = the values for rank p's scans, rw[p] of them, rows
// in order) copied to fixed runs of pitch values per peer, sent whole.  Block
// 0 also writes the batch's status for the caller: status[0] = its scans'
// total (rw[2P + 2]), status[1] = flags (1: a run to or from a peer passed
// pitch, 2: the scan pass dropped values past its buffer, 4: total > vals_cap,
// 8: a device error word of the scans).  Grid-stride copy, rows by blockIdx.y.
__global__ __launch_bounds__(kT) void k_range_pitch(const uint64_t* rvals, const uint64_t* rw,
                                                    uint32_t P, uint64_t pitch, uint64_t* out,
                                                    uint64_t rvcap, uint64_t vals_cap,
                                                    uint64_t* status) {
  const uint32_t p = blockIdx.y;
  uint64_t off = 0;
  for (uint32_t q = 0; q < p; ++q) off += rw[q];
  const uint64_t c = rw[p] < pitch ? rw[p] : pitch;
  for (uint64_t k = (uint64_t)blockIdx.x * kT + threadIdx.x; k < c; k += (uint64_t)gridDim.x * kT)
    if (off + k < rvcap) out[(uint64_t)p * pitch + k] = rvals[off + k];
  if (p == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    uint64_t f = 0;
    for (uint32_t q = 0; q < P; ++q)
      if (rw[q] > pitch || rw[P + q] > pitch) f |= 1;
    if (rw[2 * P] > rvcap) f |= 2;
    if (rw[2 * P + 2] > vals_cap) f |= 4;
    if (rw[2 * P + 1] || rw[2 * P + 3] || rw[2 * P + 5]) f |= 8;
    status[0] = rw[2 * P + 2];
    status[1] = f;
  }
}
void launch_range_pitch(const uint64_t* rvals, const uint64_t* rw, uint32_t P, uint64_t pitch,
                        uint64_t* out, uint64_t rvcap, uint64_t vals_cap, uint64_t* status,
                        hipStream_t s) {
  uint64_t bx = (pitch + kT - 1) / kT;
  if (bx > 64) bx = 64;
  if (bx == 0) bx = 1;
  hipLaunchKernelGGL(k_range_pitch, dim3((unsigned)bx, P), dim3(kT), 0, s, rvals, rw, P, pitch,
                     out, rvcap, vals_cap, status);
}

}  // namespace dev
}  // namespace shm
