// rscan_test.cpp — descending scans and floor through the host C++ facade
// (sherman_amd/csrc/Tree.hpp: rscan, floor) on one MI355X, against a std::map
// holding the same pairs.  Exit code 0 = pass.
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>

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

// the pairs of `want` at or below from, largest first, at most limit of them
void check_rscan(shm::Tree& tree, const std::map<uint64_t, uint64_t>& want, uint64_t from,
                 uint64_t limit) {
  std::vector<shm::Key> k(limit);
  std::vector<shm::Value> v(limit);
  const uint64_t n = tree.rscan(from, limit, k.data(), v.data());
  auto it = want.upper_bound(from);  // the first key above from
  uint64_t i = 0;
  while (i < limit && it != want.begin()) {
    --it;
    CHECK(i < n && k[i] == it->first && v[i] == it->second);
    ++i;
  }
  CHECK(n == i);
}
}  // namespace

int main() {
  shm_config cfg = shm::Tree::default_config();
  cfg.arena_bytes = 64ull << 20;
  cfg.max_batch = 1 << 14;
  shm::Tree tree(cfg, /*tree_id=*/0);
  std::map<uint64_t, uint64_t> want;
  const uint64_t N = 3000;
  for (uint64_t i = 1; i <= N; ++i) {
    const uint64_t k = mix(i);
    if (k == kKeyMax || k == 0) continue;
    tree.insert(k, i * 5);
    want[k] = i * 5;
  }
  for (uint64_t i = 3; i <= N; i += 7) {  // holes
    tree.del(mix(i));
    want.erase(mix(i));
  }
  CHECK(want.size() > 2000 && want.begin()->first < (1ull << 63) &&
        want.rbegin()->first >= (1ull << 63));

  shm::Key fk = 1;
  shm::Value fv = 1;
  // floor: below the minimum nothing, at and above the maximum the maximum
  CHECK(!tree.floor(want.begin()->first - 1, fk, fv));
  CHECK(!tree.floor(0, fk, fv));
  const uint64_t tops[] = {want.rbegin()->first, want.rbegin()->first + 1, kKeyMax - 1, kKeyMax};
  for (uint64_t top : tops) {
    CHECK(tree.floor(top, fk, fv));
    CHECK(fk == want.rbegin()->first && fv == want.rbegin()->second);
  }
  uint64_t n_probe = 0;
  for (auto it = want.begin(); it != want.end(); std::advance(it, 1), ++n_probe) {
    if (n_probe % 11) continue;
    // a stored key: itself; one above it: itself; one below it: its predecessor
    CHECK(tree.floor(it->first, fk, fv) && fk == it->first && fv == it->second);
    CHECK(tree.floor(it->first + 1, fk, fv) && fk == it->first && fv == it->second);
    const bool has = tree.floor(it->first - 1, fk, fv);
    if (it == want.begin()) {
      CHECK(!has);
    } else {
      auto p = std::prev(it);
      CHECK(has && fk == p->first && fv == p->second);
    }
    check_rscan(tree, want, it->first, 7);
    check_rscan(tree, want, it->first - 1, 100);
  }
  // from a deleted key: the live keys before it
  for (uint64_t i = 3; i <= N; i += 70) check_rscan(tree, want, mix(i), 3);
  // from kKeyMax: the whole tree, largest key first
  check_rscan(tree, want, kKeyMax, 1);
  check_rscan(tree, want, kKeyMax, want.size() + 1);
  check_rscan(tree, want, 1ull << 63, 200);  // across 2^63 downward
  bool refused = false;
  try {
    tree.rscan(100, 0, &fk, &fv);
  } catch (const shm::Error& e) {
    refused = e.status == SHM_EINVAL;
  }
  CHECK(refused);
  uint64_t leaves = 0, internal = 0, keys = 0;
  tree.check_tree(&leaves, &internal, &keys);
  CHECK(keys == want.size());
  std::printf("rscan_test ok: %lu keys, %lu leaves\n", (unsigned long)keys,
              (unsigned long)leaves);
  return 0;
}
