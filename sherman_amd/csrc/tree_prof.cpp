// tree_prof.cpp — profiling and diagnostics launches.
//
// The event records of the timed calls (prof_begin starts one, the issuing
// unit records its later events and pushes it, drain_profile folds the
// finished ones into the accumulator), the shm_profile_* and shm_index_stats
// calls, and the two diagnostic kernels a profiling run places on a stream
// (shm__hog, shm__mark).
#include "tree_internal.h"

namespace shm {
namespace host __attribute__((visibility("hidden"))) {

hipEvent_t take_event(shm_tree* t) {
  if (!t->prof.event_pool.empty()) {
    hipEvent_t e = t->prof.event_pool.back();
    t->prof.event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// start a ProfRec with `ne` events, e[0] recorded now on s
int prof_begin(shm_tree* t, hipStream_t s, int kind, uint64_t n, int ne,
               shm_tree::ProfRec& r) {
  r = shm_tree::ProfRec{{nullptr, nullptr, nullptr, nullptr}, n, kind, -1, 0};
  for (int i = 0; i < ne; ++i) {
    r.e[i] = take_event(t);
    if (!r.e[i]) return SHM_EIO;
  }
  HIP_OK(hipEventRecord(r.e[0], s));
  return SHM_OK;
}

// fold finished event records into the accumulator
int drain_profile(shm_tree* t) {
  for (auto& r : t->prof.pending) {
    const int ne = r.kind == shm_tree::kProfInsert ? 4 : r.kind == shm_tree::kProfGet ? 3 : 2;
    HIP_OK(hipEventSynchronize(r.e[ne - 1]));
    float d[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i + 1 < ne; ++i) HIP_OK(hipEventElapsedTime(&d[i], r.e[i], r.e[i + 1]));
    auto& a = t->prof.acc;
    if (r.kind == shm_tree::kProfGet) {
      a.calls += 1;
      a.queries += r.n;
      a.order_ms += d[0];
      a.walk_ms += d[1];
      if (r.clk >= 0) {
        // the walk's own span on the device clock: first block start to last
        // wave end (what a kernel trace reports, without the launch gap the
        // events include)
        std::vector<uint64_t> c(r.blocks * 5);
        HIP_OK(hipMemcpy(c.data(), t->prof.clk + (uint64_t)r.clk * t->prof.clk_words,
                         c.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        const uint64_t t0 = *std::min_element(c.begin(), c.begin() + r.blocks);
        const uint64_t t1 = *std::max_element(c.begin() + r.blocks, c.end());
        a.walk_kernel_ms += t1 > t0 ? (double)(t1 - t0) / t->prof.clk_khz : 0.0;
        --t->prof.clk_live;
      }
    } else if (r.kind == shm_tree::kProfInsert) {
      a.insert_calls += 1;
      a.insert_ops += r.n;
      a.insert_ms += d[0] + d[1] + d[2];
      a.upsert_ms += d[1];
    } else {
      a.range_calls += 1;
      a.range_queries += r.n;
      a.range_ms += d[0];
    }
    for (int i = 0; i < ne; ++i) t->prof.event_pool.push_back(r.e[i]);
  }
  t->prof.pending.clear();
  return SHM_OK;
}
}  // namespace host
}  // namespace shm

extern "C" {

int shm_profile_enable(shm_tree* t, int on) {
  if (!t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  t->prof.on = (on & 1) != 0;
  if (t->prof.on && !t->prof.ins) {
    if (dalloc(&t->prof.ins, 4)) return SHM_ENOMEM;
    HIP_OK(hipMemset(t->prof.ins, 0, sizeof(uint64_t) * 4));
  }
  if (t->prof.on && !t->prof.clk) {
    t->prof.clk_words = dev::get_sum_blocks(t->nmax) * 5;
    if (dalloc(&t->prof.clk, t->prof.clk_words * shm_tree::kClkSlots)) return SHM_ENOMEM;
    int khz = 0, dev_id = 0;
    HIP_OK(hipGetDevice(&dev_id));
    HIP_OK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev_id));
    t->prof.clk_khz = khz > 0 ? (double)khz : 1e5;  // 100 MHz on gfx950
  }
  const bool st = (on & 2) != 0;
  if (st && !t->prof.idx_stats) {
    if (dalloc(&t->prof.idx_stats, dev::kIdxStats)) return SHM_ENOMEM;
    HIP_OK(hipMemset(t->prof.idx_stats, 0, sizeof(uint64_t) * dev::kIdxStats));
  }
  t->prof.stats = st;
  return SHM_OK;
}

int shm_index_stats(shm_tree* t, shm_index_stats_t* out, int reset) {
  if (!t || !out) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  memset(out, 0, sizeof(*out));
  if (!t->prof.idx_stats) return SHM_OK;
  HIP_OK(hipDeviceSynchronize());
  uint64_t v[dev::kIdxStats];
  HIP_OK(hipMemcpy(v, t->prof.idx_stats, sizeof(v), hipMemcpyDeviceToHost));
  out->gets = v[dev::kIdxGets];
  out->start_internal = v[dev::kIdxStartInternal];
  out->right_moves = v[dev::kIdxRightMoves];
  out->page_hops = v[dev::kIdxPageHops];
  out->entry_reads = v[dev::kIdxEntryReads];
  out->hits = v[dev::kIdxHits];
  out->dir_fp_hits = v[dev::kIdxDirFp];
  if (reset) HIP_OK(hipMemset(t->prof.idx_stats, 0, sizeof(v)));
  return SHM_OK;
}

int shm_profile_read(shm_tree* t, shm_profile_t* out, int reset) {
  if (!t || !out) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  int rc = drain_profile(t);
  if (rc) return rc;
  if (t->prof.ins) {
    HIP_OK(hipDeviceSynchronize());
    uint64_t c[4];
    HIP_OK(hipMemcpy(c, t->prof.ins, sizeof(c), hipMemcpyDeviceToHost));
    t->prof.acc.insert_unique = c[0];
    t->prof.acc.insert_dels = c[1];
    t->prof.acc.insert_staged = c[2];
    if (reset) HIP_OK(hipMemset(t->prof.ins, 0, sizeof(c)));
  }
  *out = t->prof.acc;
  if (reset) t->prof.acc = shm_profile_t{};
  return SHM_OK;
}

// Diagnostics, not part of include/sherman_amd.h: `blocks` blocks that each
// hold a whole CU (all of its LDS) for `ticks` of the 100 MHz wall clock, on
// `stream`: other streams' kernels meanwhile get the remaining CUs only
int shm__hog(uint32_t blocks, uint64_t ticks, void* stream) {
  if (blocks > 4096 || ticks > 1000000000ull) return SHM_EINVAL;  // <= 10 s
  dev::launch_hog(blocks, ticks, pick(stream));
  HIP_OK(hipGetLastError());
  return SHM_OK;
}

// Diagnostics, not part of include/sherman_amd.h: an empty kernel on
// `stream` whose dispatch marks the edge of a profiling window (bench.py
// Region, tools/fold_roofline.py)
int shm__mark(uint32_t tag, void* stream) {
  dev::launch_mark(tag, pick(stream));
  HIP_OK(hipGetLastError());
  return SHM_OK;
}
}  // extern "C"
