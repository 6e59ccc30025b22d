// service.hip — small kernels around the tree's own: the zero-copy read-back
// every synchronising call uses, the benchmark's key generators, lock_bench,
// and two diagnostic kernels (a profile window marker, a CU hog).
#include "device_common.h"
#include "kernels.h"

namespace shm {
namespace dev {

namespace {
constexpr int kT = 256;
inline dim3 grid1(uint64_t n, int per = kT) {
  return dim3((unsigned)((n + per - 1) / per));
}
}  // namespace

// zero-copy read-back (tree.cpp readback): one wave copies the words into
// mapped host memory with vector stores, fences at system scope, then lane 0
// publishes the sequence number the host spins on.  clear: each word is
// taken by an atomic exchange with 0 (the error block: a bit another stream
// sets after the exchange stays for the next read)
__global__ void k_readback(uint32_t* dst, uint32_t* src, uint32_t nw, uint32_t* flag,
                           uint32_t seq, int clear) {
  for (uint32_t l = threadIdx.x; l < nw; l += blockDim.x)
    dst[l] = clear ? atomicExch(src + l, 0u) : src[l];
  const uint32_t l = threadIdx.x;
  __threadfence_system();
  // the fence's write-back performed before the flag (the returned exchanges
  // above let the compiler drop the fence's own wait: MI355X_MICROARCH.md
  // "Compiler hazard")
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (l == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

void launch_readback(uint32_t* dst, const uint32_t* src, uint32_t nw, uint32_t* flag,
                     uint32_t seq, int clear, hipStream_t s) {
  hipLaunchKernelGGL(k_readback, dim3(1), dim3(64), 0, s, dst, const_cast<uint32_t*>(src), nw,
                     flag, seq, clear);
}

// to_key without / with the modulus (test/benchmark.cpp:43-46)
__global__ void k_gen_keys(uint64_t first, uint64_t n, uint64_t keyspace,
                           uint64_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = cityhash64_u64(first + i) + 1;
  out[i] = keyspace ? h % keyspace : h;
}
void launch_gen_keys(uint64_t first, uint64_t n, uint64_t keyspace,
                     uint64_t* out, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_gen_keys, grid1(n), dim3(kT), 0, s, first, n, keyspace, out);
}

// keys[i] = to_key(ids[i]) for an arbitrary id array (zipf streams)
__global__ void k_hash_ids(const uint64_t* ids, uint64_t n, uint64_t keyspace,
                           uint64_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = cityhash64_u64(ids[i]) + 1;
  out[i] = keyspace ? h % keyspace : h;
}
void launch_hash_ids(const uint64_t* ids, uint64_t n, uint64_t keyspace, uint64_t* out,
                     hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_hash_ids, grid1(n), dim3(kT), 0, s, ids, n, keyspace, out);
}

// ---- Tree::lock_bench (src/Tree.cpp:310-321): take and release the lock word
// of each key, lock[CityHash64(key) % num_locks], as try_lock_addr /
// unlock_addr do (Tree.cpp:205-264) on the HBM lock table: a word is free
// when it holds <= tag (the epoch tags of the insert chunks, insert.hip),
// taken as tag | 1 by atomicCAS, released by storing tag.  Lanes of one wave
// that share a word take it in turn (a lane releases in the iteration it
// acquired, so the wave never waits on itself).  Spins are bounded.
__global__ __launch_bounds__(kT) void k_lock_bench(const uint64_t* keys, uint64_t n,
                                                   uint64_t* locks, uint32_t num_locks,
                                                   uint64_t tag, uint32_t* err) {
  const uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x;
  bool done = i >= n;
  unsigned long long* w = nullptr;
  if (!done)
    w = reinterpret_cast<unsigned long long*>(locks) + cityhash64_u64(keys[i]) % num_locks;
  const unsigned long long mine = (unsigned long long)(tag | 1ull);
  for (uint32_t spin = 0; spin < kMaxLockSpins; ++spin) {
    if (!done) {
      const unsigned long long cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur <= (unsigned long long)tag && atomicCAS(w, cur, mine) == cur) {
        __hip_atomic_store(w, (unsigned long long)tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        done = true;
      }
    }
    if (!ballot(!done)) return;
    __builtin_amdgcn_s_sleep(1);
  }
  if (!done) atomicOr(err, kErrLock);
}
void launch_lock_bench(const uint64_t* keys, uint64_t n, uint64_t* locks, uint32_t num_locks,
                       uint64_t tag, uint32_t* err, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_lock_bench, grid1(n), dim3(kT), 0, s, keys, n, locks, num_locks, tag, err);
}

// ---- diagnostics: a window marker for profiles (shm__mark) -------------------
// One empty wave whose dispatch names a window's edge in a kernel trace or a
// counter collection (tools/fold_roofline.py keeps the dispatches between
// tag 1 and tag 2).
__global__ void k_mark(uint32_t tag) { (void)tag; }
void launch_mark(uint32_t tag, hipStream_t s) {
  hipLaunchKernelGGL(k_mark, dim3(1), dim3(kWave), 0, s, tag);
}

// ---- diagnostics: a kernel that holds CUs (shm__hog) -----------------------------
// Each block declares a whole CU's LDS (160 KiB), so no other block that uses
// LDS fits its CU while it runs, and spins on the 100 MHz wall clock until
// `ticks` have passed since it started (bounded: every wave leaves).  n
// blocks therefore take n CUs away from the kernels of other streams for that
// long (tests/test_gpu_parity.py::test_split_insert_beside_cu_hog).
constexpr uint32_t kHogLdsWords = 160 * 1024 / 4;
__global__ __launch_bounds__(kWave) void k_hog(uint64_t ticks, uint32_t* sink) {
  __shared__ uint32_t s_pad[kHogLdsWords];
  s_pad[threadIdx.x] = threadIdx.x;
  const uint64_t t0 = wall_clock64();
  uint32_t spins = 0;
  while (wall_clock64() - t0 < ticks) {
    __builtin_amdgcn_s_sleep(8);
    ++spins;
  }
  // keep the LDS array alive; never true for a real run (spins > 0)
  if (spins == 0xFFFFFFFFu) sink[0] = s_pad[(threadIdx.x * 7) % kHogLdsWords];
}
void launch_hog(uint32_t n, uint64_t ticks, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_hog, dim3(n), dim3(kWave), 0, s, ticks, nullptr);
}

}  // namespace dev
}  // namespace shm
