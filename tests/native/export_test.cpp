// export_test.cpp — Tree::export_sorted, count and compact through the host
// C++ facade (sherman_amd/csrc/Tree.hpp) on one MI355X, against a std::map
// holding the same pairs: a tree grown by single and batched writes, ranges,
// a buffer that is too small, compaction and writes after it.  Exit code 0 =
// pass.
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
constexpr uint64_t kSent = 0x5A5A5A5A5A5A5A5Aull;

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

// the export of [lo, hi] equals the map's pairs there, in order; the word
// past them stays
void check_range(shm::Tree& tree, const Map& want, uint64_t lo, uint64_t hi) {
  std::vector<uint64_t> wk, wv;
  if (lo <= hi)
    for (auto it = want.lower_bound(lo); it != want.end() && it->first <= hi; ++it) {
      wk.push_back(it->first);
      wv.push_back(it->second);
    }
  const uint64_t n = wk.size();
  CHECK(tree.count(lo, hi) == n);
  std::vector<uint64_t> k(n + 1, kSent), v(n + 1, kSent);
  CHECK(tree.export_sorted(k.data(), v.data(), n, lo, hi) == n);
  CHECK(k[n] == kSent && v[n] == kSent);
  for (uint64_t i = 0; i < n; ++i) CHECK(k[i] == wk[i] && v[i] == wv[i]);
  if (n) {  // too small: the count, nothing copied
    std::vector<uint64_t> k2(n, kSent), v2(n, kSent);
    CHECK(tree.export_sorted(k2.data(), v2.data(), n - 1, lo, hi) == n);
    for (uint64_t i = 0; i < n; ++i) CHECK(k2[i] == kSent && v2[i] == kSent);
    // keys only
    CHECK(tree.export_sorted(k2.data(), nullptr, n, lo, hi) == n);
    for (uint64_t i = 0; i < n; ++i) CHECK(k2[i] == wk[i]);
  }
}

void check_all(shm::Tree& tree, const Map& want) {
  check_range(tree, want, 0, kKeyMax);
  const uint64_t a = std::next(want.begin(), want.size() / 3)->first;
  const uint64_t b = std::next(want.begin(), 2 * want.size() / 3)->first;
  check_range(tree, want, a, b);
  check_range(tree, want, a + 1, b - 1);
  check_range(tree, want, a, a);
  check_range(tree, want, b, a);
  check_range(tree, want, 0, want.begin()->first);
  check_range(tree, want, want.rbegin()->first, kKeyMax);
  check_range(tree, want, kKeyMax, kKeyMax);
  CHECK(tree.count() == want.size());
}
}  // namespace

int main() {
  shm_config cfg = shm::Tree::default_config();
  cfg.arena_bytes = 64ull << 20;
  cfg.max_batch = 1 << 14;
  shm::Tree tree(cfg, /*tree_id=*/0);
  Map want;

  // the empty tree
  CHECK(tree.count() == 0);
  uint64_t one_k = kSent, one_v = kSent;
  CHECK(tree.export_sorted(&one_k, &one_v, 1) == 0 && one_k == kSent && one_v == kSent);

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
  }
  CHECK(want.begin()->first < (1ull << 63) && want.rbegin()->first >= (1ull << 63));
  // and by single ops
  for (uint64_t i = 100000; i < 100200; ++i) {
    tree.insert(mix(i), i);
    want[mix(i)] = i;
  }
  tree.del(want.begin()->first);
  want.erase(want.begin());
  check_all(tree, want);

  // compaction: the same pairs in the plan's pages
  const uint64_t used = tree.stats().pages_used;
  CHECK(!tree.compact(54, 0));  // rejected: the tree is as it was
  CHECK(!tree.compact(1, 2));   // too tall for these pairs
  CHECK(tree.stats().pages_used == used);
  check_all(tree, want);
  CHECK(tree.compact());
  shm_bulk_plan_t pl;
  CHECK(shm_bulk_plan(want.size(), 0, 0, &pl) == SHM_OK);
  shm_stats_t st = tree.stats();
  CHECK(st.pages_used == pl.pages && st.root_level == pl.root_level);
  uint64_t leaves = 0, internal = 0, keys = 0;
  tree.check_tree(&leaves, &internal, &keys);
  CHECK(leaves == pl.level_pages[0] && leaves + internal == pl.pages && keys == want.size());
  check_all(tree, want);
  shm::Value v = 0;
  for (const auto& kv : want) CHECK(tree.search(kv.first, v) && v == kv.second);

  // writes go on after it
  for (uint64_t i = 200000; i < 200300; ++i) {
    tree.insert(mix(i), i);
    want[mix(i)] = i;
  }
  check_all(tree, want);
  CHECK(tree.compact(53, 60));
  CHECK(shm_bulk_plan(want.size(), 53, 60, &pl) == SHM_OK);
  CHECK(tree.stats().pages_used == pl.pages && pl.pages < used);  // full leaves: fewer pages
  check_all(tree, want);
  std::printf("export_test ok: %lu pairs, %lu pages after compaction (%lu before)\n",
              (unsigned long)want.size(), (unsigned long)pl.pages, (unsigned long)used);
  return 0;
}
