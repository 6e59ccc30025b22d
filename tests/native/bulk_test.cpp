// bulk_test.cpp — Tree::bulk_load through the host C++ facade
// (sherman_amd/csrc/Tree.hpp) on one MI355X, against a std::map holding the
// same pairs: the load, then search, scan and insert on the loaded tree, a
// second load over it, and rejected inputs.  Exit code 0 = pass.
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

Map make(uint64_t first, uint64_t n, uint64_t mul) {
  Map m;
  for (uint64_t i = first; i < first + n; ++i) {
    const uint64_t k = mix(i);
    if (k != kKeyMax) m[k] = i * mul;
  }
  return m;
}

void load(shm::Tree& tree, const Map& m, uint32_t lf, uint32_t inf) {
  std::vector<shm::Key> k;
  std::vector<shm::Value> v;
  for (const auto& kv : m) {  // a map iterates in ascending key order
    k.push_back(kv.first);
    v.push_back(kv.second);
  }
  CHECK(tree.bulk_load(k.data(), v.data(), k.size(), lf, inf));
}

// every pair found, the keys beside them absent, scans in key order
void check_all(shm::Tree& tree, const Map& want) {
  shm::Value v = 0;
  for (const auto& kv : want) {
    CHECK(tree.search(kv.first, v) && v == kv.second);
    if (!want.count(kv.first + 1) && kv.first + 1 != kKeyMax) CHECK(!tree.search(kv.first + 1, v));
  }
  const uint64_t limit = 300;
  std::vector<shm::Key> ks(limit);
  std::vector<shm::Value> vs(limit);
  const uint64_t froms[] = {0, want.begin()->first, 1ull << 62, 1ull << 63, want.rbegin()->first};
  for (uint64_t from : froms) {
    const uint64_t n = tree.scan(from, limit, ks.data(), vs.data());
    auto it = want.lower_bound(from);
    uint64_t i = 0;
    for (; i < limit && it != want.end(); ++i, ++it)
      CHECK(i < n && ks[i] == it->first && vs[i] == it->second);
    CHECK(n == i);
  }
  uint64_t leaves = 0, internal = 0, keys = 0;
  tree.check_tree(&leaves, &internal, &keys);
  CHECK(keys == want.size());
}
}  // namespace

int main() {
  shm_config cfg = shm::Tree::default_config();
  cfg.arena_bytes = 64ull << 20;
  cfg.max_batch = 1 << 14;
  shm::Tree tree(cfg, /*tree_id=*/0);

  // the plan is host arithmetic
  shm_bulk_plan_t pl;
  CHECK(shm_bulk_plan(2187, 1, 2, &pl) == SHM_OK && pl.root_level == 7 && pl.pages == 3280);
  CHECK(shm_bulk_plan(2188, 1, 2, &pl) == SHM_EINVAL);

  Map want = make(1, 3000, 5);
  CHECK(want.begin()->first < (1ull << 63) && want.rbegin()->first >= (1ull << 63));
  load(tree, want, 0, 0);
  CHECK(shm_bulk_plan(want.size(), 0, 0, &pl) == SHM_OK);
  shm_stats_t st = tree.stats();
  CHECK(st.pages_used == pl.pages && st.root_level == pl.root_level && st.height == pl.root_level + 1);
  uint64_t leaves = 0, internal = 0, keys = 0;
  tree.check_tree(&leaves, &internal, &keys);
  CHECK(leaves == pl.level_pages[0] && leaves + internal == pl.pages);
  check_all(tree, want);

  // single-op writes on the loaded tree
  for (uint64_t i = 5000; i < 5400; ++i) {
    tree.insert(mix(i), i);
    want[mix(i)] = i;
  }
  for (auto it = want.begin(); it != want.end();) {  // every ninth: delete or overwrite
    const uint64_t k = it->first;
    if (k % 9 == 0) {
      tree.del(k);
      it = want.erase(it);
      continue;
    }
    if (k % 9 == 1) {
      tree.insert(k, k | 1);
      it->second = k | 1;
    }
    ++it;
  }
  check_all(tree, want);

  // a second load replaces all of it: full pages, three levels
  Map other = make(100000, 53 * 61 + 1, 3);
  load(tree, other, 53, 60);
  CHECK(shm_bulk_plan(other.size(), 53, 60, &pl) == SHM_OK && pl.root_level == 2);
  st = tree.stats();
  CHECK(st.pages_used == pl.pages && st.root_level == 2);
  shm::Value v = 0;
  for (const auto& kv : want)
    if (!other.count(kv.first)) CHECK(!tree.search(kv.first, v));
  check_all(tree, other);
  tree.insert(mix(7), 77);  // splits a full leaf
  other[mix(7)] = 77;
  check_all(tree, other);

  // rejected inputs leave the tree as it is
  std::vector<shm::Key> k = {10, 30, 20};
  std::vector<shm::Value> vals = {1, 2, 3};
  CHECK(!tree.bulk_load(k.data(), vals.data(), 3));       // not ascending
  k = {10, 20, 20};
  CHECK(!tree.bulk_load(k.data(), vals.data(), 3));       // equal keys
  k = {10, 20, kKeyMax};
  CHECK(!tree.bulk_load(k.data(), vals.data(), 3));       // kKeyMax
  k = {10, 20, 30};
  vals = {1, 0, 3};
  CHECK(!tree.bulk_load(k.data(), vals.data(), 3));       // kValueNull
  vals = {1, 2, 3};
  CHECK(!tree.bulk_load(k.data(), vals.data(), 3, 54));   // leaf_fill
  CHECK(!tree.bulk_load(k.data(), vals.data(), 3, 0, 1)); // internal_fill
  check_all(tree, other);

  // the empty load: the tree of shm_tree_create
  CHECK(tree.bulk_load(nullptr, nullptr, 0));
  st = tree.stats();
  CHECK(st.pages_used == 1 && st.root_level == 0);
  CHECK(!tree.search(other.begin()->first, v));
  tree.insert(42, 4242);
  CHECK(tree.search(42, v) && v == 4242);
  std::printf("bulk_test ok: %lu keys loaded, %lu pages\n", (unsigned long)other.size(),
              (unsigned long)pl.pages);
  return 0;
}
