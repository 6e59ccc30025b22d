// get_sum.hip — the batched get, lane = query: the bucket table, the leaf
// directory entry and the summary walk (k_get_sum).
//
// Per get, three HBM lines instead of a 1 KB page: the leaf-directory entry,
// the leaf's 64 B summary line (layout.h: the highest fence, an 8-bit
// fingerprint per slot) and the entries whose fingerprint matches (false
// positives ~ 36 / 255 per get at C2's 36 keys per leaf).
// A stale directory is fixed by turning right on k >= highest from the
// summary (B-link).  Pages without a summary (internal pages: a directory
// miss, or no directory) are walked from their own bytes, lane by lane:
// check_consistent, fences, binary search of the records (Tree.cpp:593-685).
// The leaf search keeps Tree.cpp:687-697: the first slot (in slot order) with
// key == k, value != 0 and f == r.  Batches are serialised against inserts
// by the call order, so a page is never torn under a get; the entry-level
// f == r check stays.
//
// Without a directory the walk starts at the root, or — with the LDS
// replica of the top of the tree (a.top_n: every page of one upper level
// with its lowest fence, launch_top) — at the page of that level holding k,
// found by a binary search of the block's LDS copy (the north star's "upper
// tree levels replicated in LDS"; DESIGN §8 measures it against the
// directory).
#include <hip/hip_ext.h>

#include "device_common.h"
#include "dir_entry.h"
#include "kernels.h"
#include "page_fields.h"
#include "page_io.h"
#include "sum_line.h"
#include "valtab.h"

namespace shm {
namespace dev {

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}

// 5 waves per SIMD (95 VGPRs, no scratch).  Round 4 capped it at 6 waves
// (80 VGPRs: C2 +2 % against 5 then); with the pair form and the shared
// rounds the cap spilled 28-48 B per lane into scratch on the candidate
// rounds: same box C2 18623 / 18631 and C3 12750 / 12903 at 6 waves against
// 19572 / 19611 and 14828 / 14986 at 5.  With the bucket table's probe in
// front (valtab.h: 32 more registers live until the probe ends) still 95
// VGPRs, no scratch, 5 waves (PCHK, which has no probe: 96).
// COOP / PACK (WalkArgs get_coop / get_pack, chosen per launch, only with a
// table): the probe that loads each bucket line with one instruction, and
// the packing of the gets the table leaves over into the block's lowest
// waves.  Either or both: 95-96 VGPRs, no scratch, 5
// waves; PACK adds TPB x 12 + TPB / 16 B of static LDS (3088 B at 256).  The
// packed get's output index is kept as its 32-bit thread number: as a
// 64-bit index the COOP + PACK form spilled one register.
// PCHK (SHM_FLAG_PAGE_CHECK): the page-level version check on the fast
// path too -- a hit read from a page's entry also reads that page's
// front_version (byte 8) and rear_version (byte 1016) and reports a
// mismatch (kErrInconsistent: check_consistent, Tree.h:241-261, Tree.cpp:
// 616-618); two more lines per get (DESIGN §3.5 measures it)
template <int TPB, bool PCHK, bool COOP, bool PACK>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(5))) void k_get_sum(WalkArgs a) {
  static_assert(!PCHK || (!COOP && !PACK), "the page check has no probe");
  extern __shared__ __attribute__((aligned(16))) uint8_t s_top[];  // top_n x (8 + 4) B
  // the get's thread of the block: its key and its result are at block base + ti
  const uint64_t bbase = (uint64_t)blockIdx.x * TPB;
  uint32_t ti = threadIdx.x;
  const uint32_t tn = a.top_n;
  uint64_t* tk = reinterpret_cast<uint64_t*>(s_top);
  uint32_t* tpg = reinterpret_cast<uint32_t*>(s_top + 8 * (uint64_t)tn);
  if (tn) {  // block-uniform: the replica into LDS
    for (uint32_t j = threadIdx.x; j < tn; j += TPB) {
      tk[j] = a.top_keys[j];
      tpg[j] = a.top_pages[j];
    }
    __syncthreads();
  }
  if (a.clk && threadIdx.x == 0) a.clk[blockIdx.x] = wall_clock64();
  bool act = bbase + ti < a.n;
  uint64_t k = act ? a.keys[bbase + ti] : kKeyMax;
  uint64_t val = 0;
  uint32_t err = 0;
  uint32_t c_int = 0, c_right = 0, c_hops = 0, c_ent = 0;
  bool hit = false;
  uint32_t pv_f = 0, pv_r = 0;  // PCHK: the hit page's front / rear versions
  bool done = false;            // val is the answer
  // a get is counted where it enters the kernel (the packing below hands it
  // to another lane)
  uint32_t c_gets = act && k != kKeyMax ? 1u : 0u;
  auto add_stats = [&]() {  // wave-uniform; every lane of the wave is here
    const uint32_t v[kIdxStats] = {wave_sum32(c_gets), wave_sum32(c_int),
                                   wave_sum32(c_right), wave_sum32(c_hops), wave_sum32(c_ent),
                                   wave_sum32(act && val != kValueNull ? 1u : 0u),
                                   wave_sum32(hit ? 1u : 0u)};
    if (lane_id() == 0)
      for (int j = 0; j < kIdxStats; ++j)
        if (v[j]) atomicAdd(reinterpret_cast<unsigned long long*>(a.stats + j), v[j]);
  };
  // the bucket table (valtab.h) first: one 128 B line holds every key of
  // k's bucket, so a live bucket answers the get -- the key's value, or
  // absent -- with this one request; a dead bucket (more than 8 keys) goes
  // on below as before.  The 32 bucket registers are dead past this block.
  if (!PCHK && a.vt) {  // uniform over the launch
    uint64_t b;
    const bool hb = vt_bucket_of(a.vt_lo, a.vt_shift, a.vt_n, k, &b);  // never kKeyMax
    if (COOP) {
      // One load instruction per bucket line: in round r the eight lanes of
      // group g = lane >> 3 load the eight slots of the bucket of the get
      // that lane 8 r + g owns, so a wave instruction reads eight whole
      // lines and no later one touches them (a lane loading its own bucket
      // touches 64 lines per instruction, each of them eight times).  All
      // eight rounds are issued before the first compare.
      const int lane = lane_id(), g = lane >> 3, sl = lane & 7;
      u32x4 w[kVtSlots];
      uint64_t ok[kVtSlots];  // the owners' keys
#pragma unroll
      for (int r = 0; r < kVtSlots; ++r) {
        ok[r] = shfl64(k, 8 * r + g);
        uint64_t ob;
        w[r] = u32x4{0u, 0u, 0u, 0u};  // no bucket, no load: a free slot
        if (vt_bucket_of(a.vt_lo, a.vt_shift, a.vt_n, ok[r], &ob))
          w[r] = reinterpret_cast<const u32x4*>(a.vt + kVtBucketWords * ob)[sl];
      }
#pragma unroll
      for (int r = 0; r < kVtSlots; ++r) {
        uint64_t sv;
        const uint64_t M = ballot(vt_slot_match(w[r], ok[r], &sv));
        const uint64_t D = ballot(sl == 0 && vt_slot_dead(w[r]));
        // the owner of round r, lane 8 r + sl, was served by group sl:
        // vt_probe's answer from that group's eight predicates
        const uint32_t mg = (uint32_t)(M >> (8 * sl)) & 0xFFu;
        const bool dg = ((D >> (8 * sl)) & 1ull) != 0;
        const uint64_t v = shfl64(sv, 8 * sl + (mg ? 31 - __builtin_clz(mg) : 0));
        if (g == r && hb && !dg) {
          done = true;
          if (mg) {
            val = v;
            hit = true;
          }
        }
      }
    } else if (hb) {
      const u32x4* bp = reinterpret_cast<const u32x4*>(a.vt + kVtBucketWords * b);
      u32x4 w[kVtSlots];
#pragma unroll
      for (int j = 0; j < kVtSlots; ++j) w[j] = bp[j];
      const int r = vt_probe(w, k, &val);
      hit = r >= 0;
      done = r != kVtDead;
    }
    if (PACK) {
      // The gets the table did not answer (a dead bucket, key 0, a key
      // outside the table's range) are few per wave, and each would keep its
      // wave resident through the directory path's dependent rounds.  The
      // answered lanes store now; the block's other gets are packed, in
      // thread order, into its lowest waves, which alone go on.
      __shared__ uint64_t s_pk[TPB];           // the packed gets' keys
      __shared__ uint32_t s_pt[TPB];           // ... and the threads they came from
      __shared__ uint32_t s_pc[TPB / kWave];   // per wave
      const int lane = lane_id(), wv = (int)(threadIdx.x / kWave);
      const bool fall = c_gets && !done;
      if (act && !fall) {
        a.out_val[bbase + ti] = val;
        if (a.out_found) a.out_found[bbase + ti] = val != kValueNull ? 1 : 0;
      }
      if (a.stats) add_stats();
      // a wave's gets go to its own 64 slots, so one barrier is enough: the
      // readers find slot p of the packed order from the waves' counts
      const uint64_t fm = ballot(fall);
      if (fall) {
        const int at = wv * kWave + popc64(fm & lanemask_lt());
        s_pk[at] = k;
        s_pt[at] = threadIdx.x;
      }
      if (lane == 0) s_pc[wv] = (uint32_t)popc64(fm);
      __syncthreads();
      const uint32_t p = threadIdx.x;
      uint32_t base = 0;
      int src = -1;
#pragma unroll
      for (int j = 0; j < TPB / kWave; ++j) {
        const uint32_t c = s_pc[j];
        if (p >= base && p - base < c) src = j * kWave + (int)(p - base);
        base += c;
      }
      if ((uint32_t)(wv * kWave) >= base) {  // wave-uniform: nothing left for this wave
        if (a.clk && lane == 0)
          a.clk[gridDim.x + blockIdx.x * (TPB / kWave) + wv] = wall_clock64();
        return;
      }
      act = src >= 0;
      k = act ? s_pk[src] : kKeyMax;
      ti = act ? s_pt[src] : 0u;
      val = 0;
      hit = done = false;
      c_gets = 0;
    }
  }
  if (k != kKeyMax) {  // never stored (root highest is exclusive, Tree.h:150)
    uint64_t ptr = a.root;
    uint64_t alt = 0;  // a tie's safe start (dir_start_e)
    if (done) {
    } else if (a.dir) {
      u32x4 e[4];
      bool fpform;
      ptr = dir_start_e(a.dir, a.dir_lo, a.dir_shift, a.dir_n, a.node, k, ptr, e, fpform, &alt);
      // A wave's gets take their slowest lane's number of dependent rounds,
      // so the lanes share rounds: after the directory entry, a lane in
      // fingerprint form reads its lowest candidate entry (the prefix lies
      // in one leaf and the entry holds its fingerprints: Tree.cpp:687-697's
      // first valid slot with the key) while a lane that needs the summary
      // line reads it -- before, the summary lanes waited for the whole
      // wave's candidate loop -- and then every lane reads one candidate per
      // round, lowest first, the summary lanes' first beside the fingerprint
      // lanes' second.  A stale copy, an absent key, a right turn, a tie's
      // safe start, an internal page go on below.  C3 +5-7 %, C2 +0.5 %
      // (same box, first form); reading two candidates per round was C2
      // -2 % (speculative requests) for about the same C3.
      const bool pok = ptr_ok(ptr, a.node, a.arena_bytes);
      const uint64_t off = ga_offset(ptr);
      const uint8_t* page = a.arena + off;
      const bool fp = fpform && pok;
      // a read phase's pair form: the prefix's own keys, in up to four leaves
      bool pu = false;
      const uint32_t pc = !fpform && pok ? dir_pair_cand(e, k, pu) : 0u;
      const bool sm = !fpform && pok && !pu;
      // an exact directory (built, then kept by every insert chunk since):
      // a usable entry names every key of its prefix, so a key it does not
      // lead to is absent -- no summary walk for a miss (a tie at a split
      // point, or more matching pairs than the lane queues, walks anyway)
      const bool exact_miss = a.dir_exact && ((fpform && pok) || (pu && alt == 0 &&
                                                                  __builtin_popcount(pc) <= 8));
      // the value form (layout.h kDirVals): an exact directory's entry of a
      // prefix of at most two keys carries them whole, so the get ends with
      // its first request -- the key's value, or absent by the rule above.
      // Not with PCHK (no page read, no versions to check).
      if (!PCHK && a.dir_exact && pu && dir_vals_usable(e[1].w)) {
        const uint32_t np = (e[1].w >> 16) & 0xFFu;
        const uint64_t k0 = (uint64_t)e[0].z | ((uint64_t)e[0].w << 32);
        const uint64_t v0 = (uint64_t)e[1].y | ((uint64_t)e[1].z << 32);
        const uint64_t k1 = (uint64_t)e[3].x | ((uint64_t)e[3].y << 32);
        const uint64_t v1 = (uint64_t)e[3].z | ((uint64_t)e[3].w << 32);
        if (np > 0 && k0 == k && v0 != kValueNull) {
          val = v0;
          hit = done = true;
        } else if (np > 1 && k1 == k && v1 != kValueNull) {
          val = v1;
          hit = done = true;
        } else if (exact_miss) {
          done = true;
        }
      }
      // pend: the lane's candidate slots of its leaf still to read, lowest
      // first; a pair lane's candidates instead as up to 8 packed bytes
      // (leaf << 6 | slot) in plist, with the leaves' pages in lpg (the
      // directory entry itself is dead past this point: held through the
      // rounds it spilled registers, C3 -15 %)
      uint64_t pend = fp ? dir_fp_cand(e, k) : 0;
      uint64_t plist = 0;
      uint32_t pn = 0;
      const uint32_t lpg[4] = {e[0].x, e[0].y, e[0].z, e[0].w};
      if (pu && !done) {
#pragma unroll
        for (int j = 0; j < (int)kDirPairMax; ++j) {
          if (((pc >> j) & 1u) && pn < 8) {
            uint32_t pgi;
            int sl;
            dir_pair_slot(e, j, pgi, sl);
            const uint32_t leaf = pgi == lpg[0] ? 0u : pgi == lpg[1] ? 1u : pgi == lpg[2] ? 2u : 3u;
            plist |= (uint64_t)((leaf << 6) | (uint32_t)sl) << (8 * pn);
            ++pn;
          }
        }
      }
      // the next candidate -> its page and slot (false: a pair naming a bad
      // page); pops it
      const uint8_t* cp = page;
      int cs = 0;
      auto next = [&]() -> bool {
        if (pn == 0) {
          cp = page;
          cs = (int)ctz64(pend);
          pend &= pend - 1;
          return true;
        }
        const uint32_t b = (uint32_t)plist & 0xFFu;
        plist >>= 8;
        --pn;
        cs = (int)(b & 63u);
        const uint32_t li = b >> 6;
        const uint64_t ga = dir_page_ga(li == 0 ? lpg[0] : li == 1 ? lpg[1] : li == 2 ? lpg[2] : lpg[3],
                                        a.node);
        cp = a.arena + ga_offset(ga);
        return ptr_ok(ga, a.node, a.arena_bytes);
      };
      RawEntry r1;
      bool l1 = false;
      const bool any1 = !done && (pend || pn);
      if (any1) {
        l1 = next();
        if (l1) entry_load(cp, cs, r1);
      }
      u32x4 sraw[4];
      if (sm) sum_load(a.sum, off, sraw);
      uint64_t ek, ev;
      uint32_t ef, er;
      if (any1 && l1) {
        ++c_ent;
        entry_decode(r1, ek, ev, ef, er);
        if (entry_hit(ek, ev, ef, er, k)) {
          val = ev;
          hit = done = true;
          if (PCHK) {
            pv_f = cp[kOffFrontVer];
            pv_r = cp[kOffLeafRear];
          }
        }
      }
      // a summary lane in k's leaf (k >= highest turns right below) joins
      // the candidate rounds
      SumLine sl;
      const bool inleaf = sm && sum_decode(sraw, k, sl) && k < sl.highest;
      if (inleaf) pend = sl.cand;
      while (!done && (pend || pn)) {  // one candidate per lane and round, lowest first
        if (next()) {
          ++c_ent;
          lane_entry(cp, cs, ek, ev, ef, er);
          if (entry_hit(ek, ev, ef, er, k)) {
            val = ev;
            done = true;
            hit = fp || pu;
            if (PCHK) {
              pv_f = cp[kOffFrontVer];
              pv_r = cp[kOffLeafRear];
            }
          }
        }
      }
      if (!done && exact_miss) done = true;  // absent (val stays 0)
      // not found: a fingerprint or pair lane takes the summary walk below
      // (absent key or stale copy); a summary lane's leaf does not hold k,
      // unless this was a tie's optimistic leaf (k may lie below its lowest
      // fence: walk again from the safe start)
      if (!done && inleaf) {
        if (alt) {
          ptr = alt;
          alt = 0;
        } else {
          done = true;
        }
      }
    } else if (tn) {
      // the last page of the level whose lowest fence is <= k (tk[0] = kKeyMin)
      uint32_t lo = 0, hi = tn;
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tk[mid] <= k)
          lo = mid;
        else
          hi = mid;
      }
      ptr = dir_page_ga(tpg[lo], a.node);
    }
    int retries = 0;
    for (int hop = 0; !done; ++hop) {
      if (hop > kMaxRounds) {
        err |= kErrGetHops;
        break;
      }
      if (!ptr_ok(ptr, a.node, a.arena_bytes)) {
        err |= kErrBadPtr;
        break;
      }
      const uint64_t off = ga_offset(ptr);
      const uint8_t* page = a.arena + off;
      SumLine sl;
      if (sum_read(a.sum, off, k, sl)) {
        if (k >= sl.highest) {  // turn right (Tree.cpp:626-629)
          const uint64_t sib = page_sibling(a.arena + off);
          if (!sib) {
            err |= kErrFence;
            break;
          }
          ptr = sib;
          ++c_right;
          continue;
        }
        uint64_t cand = sl.cand;
        while (cand) {
          uint64_t ek, ev;
          uint32_t ef, er;
          ++c_ent;
          lane_entry(page, ctz64(cand), ek, ev, ef, er);
          if (entry_hit(ek, ev, ef, er, k)) {
            val = ev;
            if (PCHK) {
              pv_f = page[kOffFrontVer];
              pv_r = page[kOffLeafRear];
            }
            break;
          }
          cand &= cand - 1;
        }
        if (val == kValueNull && alt) {
          // a tie's optimistic leaf does not hold k: k may lie below its
          // lowest fence, so walk again from the safe start
          ptr = alt;
          alt = 0;
          continue;
        }
        break;
      }
      // no summary: the page's own bytes
      if (hop == 0) c_int = 1;
      ++c_hops;
      // page_fields.h's hdr_fields over dwords 2..10 (A.z .. C.z), restated
      // with its helpers: through the struct reader the kernel's register
      // allocation changes, and a kernel the bench times stays as it is
      const u32x4* pw = reinterpret_cast<const u32x4*>(page);
      const u32x4 A = pw[0], B = pw[1], C = pw[2];
      const uint64_t leftmost = u64_b1(A.z, A.w, B.x);
      const uint64_t sibling = u64_b1(B.x, B.y, B.z);
      const uint64_t lowest = u64_of(B.w, C.x);
      const uint64_t highest = u64_of(C.y, C.z);
      const int cnt = (int)(int16_t)(B.z >> 16) + 1;
      const bool leaf = leftmost == 0;
      const uint32_t* pd = page_dw(page);
      const uint32_t rver = (leaf ? pd[kDwLeafRear] : pd[kDwInternalRear]) & 0xFF;
      if ((A.z & 0xFF) != rver) {  // torn page: read it again (Tree.cpp:616-618)
        if (++retries > kMaxRetries) {
          err |= kErrInconsistent;
          break;
        }
        continue;
      }
      if (k >= highest && sibling) {
        ptr = sibling;
        ++c_right;
        continue;
      }
      if (k < lowest && alt) {  // a tie's optimistic leaf: k lies to its left
        ptr = alt;
        alt = 0;
        continue;
      }
      if (k < lowest || k >= highest) {
        err |= kErrFence;
        break;
      }
      if (leaf) {  // every slot
        for (int sl = 0; sl < kLeafCardinality; ++sl) {
          uint64_t ek, ev;
          uint32_t ef, er;
          lane_entry(page, sl, ek, ev, ef, er);
          if (entry_hit(ek, ev, ef, er, k)) {
            val = ev;
            break;
          }
        }
        break;  // k >= lowest: this leaf is k's, found or not
      }
      // internal_page_search (Tree.cpp:665-685): child = #keys <= k
      int lo = 0, hi = cnt < kInternalCardinality ? cnt : kInternalCardinality;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint64_t km = u64_of(pd[rec_key_dw(mid)], pd[rec_key_dw(mid) + 1]);
        if (km <= k)
          lo = mid + 1;
        else
          hi = mid;
      }
      ptr = lo == 0 ? leftmost : u64_of(pd[rec_ptr_dw(lo - 1)], pd[rec_ptr_dw(lo - 1) + 1]);
    }
  }
  if (a.stats) add_stats();
  if (PCHK && pv_f != pv_r) err |= kErrInconsistent;  // a torn page under a get
  if (err) atomicOr(a.err, err);
  if (act) {
    a.out_val[bbase + ti] = val;
    if (a.out_found) a.out_found[bbase + ti] = val != kValueNull ? 1 : 0;
  }
  if (a.clk && lane_id() == 0)
    a.clk[gridDim.x + blockIdx.x * (TPB / kWave) + (threadIdx.x / kWave)] = wall_clock64();
}

uint64_t get_sum_blocks(uint64_t n) { return (n + kGetSumTPB - 1) / kGetSumTPB; }

void launch_get_sum(const WalkArgs& a, uint64_t n, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
  if (n == 0) {
    // the profile's events still complete
    if (ev0) (void)hipEventRecord(ev0, s);
    if (ev1) (void)hipEventRecord(ev1, s);
    return;
  }
  constexpr int TPB = kGetSumTPB;
  const uint32_t lds = (uint32_t)a.top_n * 12;
  const dim3 grid((unsigned)((n + TPB - 1) / TPB));
  // the probe's forms matter only with a table: without one every launch is
  // the plain instantiation (no list in LDS, no barrier)
  const bool coop = a.vt && a.get_coop, pack = a.vt && a.get_pack;
  // ev0 / ev1 (the profile): the dispatch's own start and end
#define SHM_GET_SUM(P, C, K) \
  hipExtLaunchKernelGGL((k_get_sum<TPB, P, C, K>), grid, dim3(TPB), lds, s, ev0, ev1, 0u, a)
  if (a.page_check)
    SHM_GET_SUM(true, false, false);
  else if (coop && pack)
    SHM_GET_SUM(false, true, true);
  else if (coop)
    SHM_GET_SUM(false, true, false);
  else if (pack)
    SHM_GET_SUM(false, false, true);
  else
    SHM_GET_SUM(false, false, false);
#undef SHM_GET_SUM
}

}  // namespace dev
}  // namespace shm
