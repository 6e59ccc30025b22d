// rebalance_plan_test.cpp — shm_rebalance_plan (host arithmetic: no handle, no
// GPU) against its own definition and invariants, over every world size and a
// sweep of count vectors (empty, fewer pairs than shards, everything on one
// rank, counts whose products pass 2^64).  Exit code 0 = pass.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/sherman_amd.h"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "FAIL %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

namespace {
// splitmix64
uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

void check_counts(const std::vector<uint64_t>& counts) {
  const uint32_t P = (uint32_t)counts.size();
  uint64_t N = 0;
  for (uint64_t c : counts) N += c;
  std::vector<std::vector<uint64_t>> send(P, std::vector<uint64_t>(P)), recv = send;
  std::vector<uint64_t> cut0(P + 1);
  uint64_t lo = ~0ull, hi = 0, total = 0;
  for (uint32_t r = 0; r < P; ++r) {
    std::vector<uint64_t> cut(P + 1, 77);
    CHECK(shm_rebalance_plan(counts.data(), P, r, cut.data(), send[r].data(), recv[r].data()) ==
          SHM_OK);
    if (r == 0) cut0 = cut;
    CHECK(cut == cut0);  // the same cuts on every rank
    CHECK(cut[0] == 0 && cut[P] == N);
    for (uint32_t p = 0; p < P; ++p) {
      CHECK(cut[p] <= cut[p + 1]);
      CHECK(cut[p] == (uint64_t)(((unsigned __int128)N * p) / P));
    }
    uint64_t s = 0, g = 0;
    for (uint32_t p = 0; p < P; ++p) {
      s += send[r][p];
      g += recv[r][p];
    }
    CHECK(s == counts[r]);
    CHECK(g == cut[r + 1] - cut[r]);
    lo = std::min(lo, g);
    hi = std::max(hi, g);
    total += g;
  }
  CHECK(total == N && hi - lo <= 1);
  for (uint32_t a = 0; a < P; ++a)
    for (uint32_t b = 0; b < P; ++b) CHECK(send[a][b] == recv[b][a]);
}
}  // namespace

int main() {
  uint64_t cases = 0;
  for (uint32_t P = 1; P <= 16; ++P) {
    std::vector<std::vector<uint64_t>> sets;
    sets.push_back(std::vector<uint64_t>(P, 0));
    sets.push_back(std::vector<uint64_t>(P, 7));
    sets.push_back(std::vector<uint64_t>(P, (1ull << 59) + 3));  // N p passes 2^64
    for (uint32_t one = 0; one < P; ++one) {
      std::vector<uint64_t> c(P, 0);
      c[one] = 1;
      sets.push_back(c);
      c[one] = 40000;
      sets.push_back(c);
      c[one] = P - 1;  // fewer pairs than shards
      sets.push_back(c);
    }
    for (uint64_t seed = 0; seed < 200; ++seed) {
      std::vector<uint64_t> c(P);
      for (uint32_t p = 0; p < P; ++p) {
        const uint64_t x = mix(seed * 64 + P * 1000 + p);
        c[p] = (x & 3) == 0 ? 0 : (x >> 8) % ((seed & 1) ? 5 : 100000);
      }
      sets.push_back(c);
    }
    for (const auto& c : sets) {
      check_counts(c);
      ++cases;
    }
  }
  uint64_t w[18] = {};
  CHECK(shm_rebalance_plan(w, 0, 0, w, w, w) == SHM_EINVAL);
  CHECK(shm_rebalance_plan(w, 17, 0, w, w, w) == SHM_EINVAL);
  CHECK(shm_rebalance_plan(w, 4, 4, w, w, w) == SHM_EINVAL);
  CHECK(shm_rebalance_plan(nullptr, 4, 0, w, w, w) == SHM_EINVAL);
  CHECK(shm_rebalance_plan(w, 4, 0, w, nullptr, w) == SHM_EINVAL);
  for (uint64_t x : w) CHECK(x == 0);
  std::printf("rebalance_plan_test ok: %llu count vectors\n", (unsigned long long)cases);
  return 0;
}
