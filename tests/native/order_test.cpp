// order_test.cpp — Tree::rank, count_range and select through the host C++
// facade (sherman_amd/csrc/Tree.hpp) on one MI355X, against a std::map holding
// the same pairs: the empty tree, a tree that grows by batches and single
// writes, shrinks by deletes, is compacted and grows again.  Every change is
// followed by queries, so each of them must rebuild the order index.  Exit
// code 0 = pass.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../../sherman_amd/csrc/Tree.hpp"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "FAIL %s (%s:%d)\n", #c, __FILE__, __LINE__); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

namespace {
constexpr uint64_t kKeyMax = ~0ull;

// splitmix64: keys on both sides of 2^63
uint64_t mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

using Map = std::map<uint64_t, uint64_t>;

// one batch of upserts (value 0 deletes) on the tree and on the map
void apply(shm::Tree& tree, Map& want, const std::vector<uint64_t>& k,
           const std::vector<uint64_t>& v) {
  uint64_t *dk = nullptr, *dv = nullptr;
  const size_t bytes = k.size() * sizeof(uint64_t);
  CHECK(hipMalloc(&dk, bytes) == hipSuccess && hipMalloc(&dv, bytes) == hipSuccess);
  CHECK(hipMemcpy(dk, k.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
  CHECK(hipMemcpy(dv, v.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
  tree.insert_batch(dk, dv, k.size());
  CHECK(hipFree(dk) == hipSuccess && hipFree(dv) == hipSuccess);
  for (size_t i = 0; i < k.size(); ++i) {
    if (v[i])
      want[k[i]] = v[i];
    else
      want.erase(k[i]);
  }
}

uint64_t builds(shm::Tree& tree) {
  shm_order_stats_t st;
  CHECK(shm_order_stats(tree.handle(), &st) == SHM_OK);
  return st.builds;
}

// the three calls on a sample of the stored pairs, their neighbours and the
// ends of the key space; `changed`: the tree changed since the last call
void check_all(shm::Tree& tree, const Map& want, bool changed) {
  const uint64_t b0 = builds(tree);
  std::vector<uint64_t> keys, vals;
  for (const auto& kv : want) {
    keys.push_back(kv.first);
    vals.push_back(kv.second);
  }
  const uint64_t n = keys.size();
  CHECK(tree.rank(kKeyMax) == n);
  CHECK(builds(tree) == b0 + (changed ? 1 : 0));
  CHECK(tree.rank(0) == 0 && tree.rank(kKeyMax - 1) == n);
  CHECK(tree.count_range(0, kKeyMax) == n && tree.count_range(0, kKeyMax - 1) == n);
  CHECK(tree.count_range(kKeyMax, kKeyMax) == 0 && tree.count_range(7, 3) == 0);
  uint64_t k = 1, v = 1;
  CHECK(!tree.select(n, k, v) && !tree.select(n + 1, k, v) && !tree.select(kKeyMax, k, v));
  CHECK(!tree.select(1ull << 63, k, v) && k == 1 && v == 1);
  const uint64_t step = n / 97 + 1;
  for (uint64_t i = 0; i < n; i += (i < 60 || i + 60 >= n) ? 1 : step) {
    CHECK(tree.rank(keys[i]) == i && tree.rank(keys[i] + 1) == i + 1);
    if (keys[i]) CHECK(tree.rank(keys[i] - 1) == i - (i && keys[i - 1] == keys[i] - 1 ? 1 : 0));
    CHECK(tree.select(i, k, v) && k == keys[i] && v == vals[i]);
    const uint64_t j = i + 1000 < n ? i + 1000 : n - 1;
    CHECK(tree.count_range(keys[i], keys[j]) == j - i + 1);
    CHECK(tree.count_range(keys[i] + 1, keys[j]) == j - i);
    CHECK(tree.count_range(keys[i], keys[i]) == 1);
    if (j > i) CHECK(tree.count_range(keys[j], keys[i]) == 0);
  }
  CHECK(builds(tree) == b0 + (changed ? 1 : 0));  // one build served all of them
}
}  // namespace

int main() {
  shm_config cfg = shm::Tree::default_config();
  cfg.arena_bytes = 64ull << 20;
  cfg.max_batch = 1 << 14;
  shm::Tree tree(cfg, /*tree_id=*/0);
  Map want;

  // the empty tree: one unit, no pair
  CHECK(builds(tree) == 0);
  check_all(tree, want, true);
  check_all(tree, want, false);

  // grown by batches: new keys, overwrites and deletes, so leaves split and
  // slots hold holes
  for (int round = 0; round < 4; ++round) {
    std::vector<uint64_t> k, v;
    for (uint64_t i = 0; i < 6000; ++i) {
      k.push_back(mix(round * 6000 + i));
      v.push_back(i * 2 + 1);
    }
    if (round) {
      uint64_t j = 0;
      for (const auto& kv : want) {
        if (j % 5 == 0) {
          k.push_back(kv.first);
          v.push_back(0);
        } else if (j % 5 == 1) {
          k.push_back(kv.first);
          v.push_back(kv.second + 2);
        }
        ++j;
      }
    }
    CHECK(k.size() <= cfg.max_batch);
    apply(tree, want, k, v);
    check_all(tree, want, true);
  }
  CHECK(want.begin()->first < (1ull << 63) && want.rbegin()->first >= (1ull << 63));
  // and by single ops
  for (uint64_t i = 100000; i < 100200; ++i) {
    tree.insert(mix(i), i);
    want[mix(i)] = i;
  }
  tree.del(want.begin()->first);
  want.erase(want.begin());
  check_all(tree, want, true);
  check_all(tree, want, false);
  shm::Value v = 0;
  CHECK(tree.search(want.begin()->first, v));  // a get leaves the index valid
  check_all(tree, want, false);

  // it shrinks: two of three keys deleted, whole leaves empty
  {
    std::vector<uint64_t> k, z;
    uint64_t j = 0;
    for (const auto& kv : want)
      if (j++ % 3) k.push_back(kv.first);
    for (size_t at = 0; at < k.size(); at += cfg.max_batch) {
      std::vector<uint64_t> part(k.begin() + at,
                                 k.begin() + std::min<size_t>(k.size(), at + cfg.max_batch));
      z.assign(part.size(), 0);
      apply(tree, want, part, z);
    }
  }
  check_all(tree, want, true);
  const uint64_t used = tree.stats().pages_used;
  CHECK(tree.compact());
  CHECK(tree.stats().pages_used < used);
  check_all(tree, want, true);
  // and grows again
  for (uint64_t i = 200000; i < 200300; ++i) {
    tree.insert(mix(i), i);
    want[mix(i)] = i;
  }
  check_all(tree, want, true);
  std::printf("order_test ok: %lu pairs, %lu index builds\n", (unsigned long)want.size(),
              (unsigned long)builds(tree));
  return 0;
}
