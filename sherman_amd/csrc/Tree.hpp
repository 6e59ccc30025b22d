// Tree.hpp — host C++ facade with the reference's Tree API
// (include/Tree.h:42-63) over the C-ABI (include/sherman_amd.h).
//
//   Reference                                   Here
//   Tree(DSM*, uint16_t tree_id)                Tree(const shm_config&, uint16_t tree_id = 0)
//   void insert(const Key&, const Value&, ...)  insert(k, v[, cxt, coro_id])
//   bool search(const Key&, Value&, ...)        search(k, v[, cxt, coro_id])
//   void del(const Key&, ...)                   del(k[, cxt, coro_id])
//   uint64_t range_query(from, to, Value* buf)  range_query(from, to, buf[, cxt, coro_id])
//   (new) ordered scan with a count limit       scan(from, limit, keys, vals)
//   (new) the same downwards, predecessor       rscan(from, limit, keys, vals), floor(k, key, val)
//   void print_and_check_tree(...)              print_and_check_tree([cxt, coro_id])
//   void lock_bench(const Key&, ...)            lock_bench(k[, cxt, coro_id])
//   void index_cache_statistics()               index_cache_statistics() (the leaf directory's)
//   void clear_statistics()                     clear_statistics()
//   (new) the tree of a sorted run, one pass    bulk_load(keys, vals, n[, leaf_fill, internal_fill])
//   (new) every pair of a range, in key order   export_sorted(keys, vals, cap[, lo, hi]), count([lo, hi])
//   (new) order statistics                      rank(k), count_range(from, to), select(r, key, val)
//   (new) the tree rebuilt from its own pairs   compact([leaf_fill, internal_fill])
//   (new) the key range hint of a live tree    set_key_range(key_lo, key_bits)
//   (new) batched forms on device pointers      search_batch / insert_batch / mixed_batch
//
// The coroutine arguments are accepted and ignored, so call sites of the
// reference's coroutine path (src/Tree.cpp:1088-1093) compile unchanged: a
// GPU batch hides latency with occupancy, not with coroutines.
//
// Single ops are batches of one, staged through small device buffers; the
// batched forms are the hot path.  Errors that the reference turns into
// assert()/infinite retries throw shm::Error here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sherman_amd.h"

namespace shm {

// the reference's coroutine context (include/Common.h); only its pointer is
// ever passed here
struct CoroContext;

using Key = uint64_t;    // include/Common.h:113
using Value = uint64_t;  // include/Common.h:114
constexpr Value kValueNull = 0;

struct Error : std::runtime_error {
  int status;
  Error(int s, const std::string& what)
      : std::runtime_error(what + ": " + shm_strerror(s)), status(s) {}
};

inline void check(int s, const char* what) {
  if (s != SHM_OK) throw Error(s, what);
}

class Tree {
 public:
  explicit Tree(const shm_config& cfg, uint16_t tree_id = 0) : tree_id(tree_id) {
    check(shm_tree_create(&cfg, &t_), "shm_tree_create");
    if (hipSetDevice(cfg.device) != hipSuccess ||
        hipMalloc(&d_keys_, 2 * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&d_vals_, 2 * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&d_found_, 8) != hipSuccess) {
      release();  // whichever of them were allocated
      throw Error(SHM_ENOMEM, "staging buffers");
    }
  }
  static shm_config default_config() {
    shm_config c;
    shm_config_init(&c);
    return c;
  }
  ~Tree() { release(); }
  Tree(const Tree&) = delete;
  Tree& operator=(const Tree&) = delete;

  // Tree::insert (Tree.cpp:353-403); v == kValueNull deletes
  void insert(const Key& k, const Value& v, CoroContext* cxt = nullptr, int coro_id = 0) {
    (void)cxt;
    (void)coro_id;
    stage(k, &v);
    check(shm_insert_batch(t_, d_keys_, d_vals_, 1, nullptr), "insert");
  }
  // Tree::search (Tree.cpp:405-459)
  bool search(const Key& k, Value& v, CoroContext* cxt = nullptr, int coro_id = 0) {
    (void)cxt;
    (void)coro_id;
    stage(k, nullptr);
    check(shm_search_batch(t_, d_keys_, 1, d_vals_, d_found_, nullptr), "search");
    uint8_t f = 0;
    if (hipMemcpy(&v, d_vals_, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&f, d_found_, 1, hipMemcpyDeviceToHost) != hipSuccess)
      throw Error(SHM_EIO, "search copy-back");
    return f != 0;
  }
  // Tree::del (Tree.cpp:542-591)
  void del(const Key& k, CoroContext* cxt = nullptr, int coro_id = 0) {
    (void)cxt;
    (void)coro_id;
    stage(k, nullptr);
    check(shm_del_batch(t_, d_keys_, 1, nullptr), "del");
  }
  // Tree::range_query (Tree.cpp:461-540), intended semantics: values of
  // [from, to] in leaf then slot order; `buffer` must hold every match.
  uint64_t range_query(const Key& from, const Key& to, Value* buffer,
                       CoroContext* cxt = nullptr, int coro_id = 0) {
    (void)cxt;
    (void)coro_id;
    uint64_t h[2] = {from, to};
    uint64_t *d_from = d_keys_, *d_to = d_keys_ + 1, *d_cnt = d_vals_;
    if (hipMemcpy(d_keys_, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess)
      throw Error(SHM_EIO, "range stage");
    check(shm_range_query(t_, d_from, d_to, 1, d_cnt, nullptr, nullptr, nullptr),
          "range count");
    uint64_t cnt = 0;
    if (hipMemcpy(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess)
      throw Error(SHM_EIO, "range count copy");
    if (cnt == 0) return 0;
    uint64_t *d_out = nullptr, *d_off = nullptr;
    if (hipMalloc(&d_out, cnt * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&d_off, sizeof(uint64_t)) != hipSuccess ||
        hipMemset(d_off, 0, sizeof(uint64_t)) != hipSuccess) {
      if (d_out) (void)hipFree(d_out);
      if (d_off) (void)hipFree(d_off);
      throw Error(SHM_ENOMEM, "range buffers");
    }
    int s = shm_range_query(t_, d_from, d_to, 1, d_cnt, d_off, d_out, nullptr);
    if (s == SHM_OK &&
        hipMemcpy(buffer, d_out, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
      s = SHM_EIO;
    (void)hipFree(d_out);
    (void)hipFree(d_off);
    check(s, "range_query");
    return cnt;
  }

  // The first `limit` valid entries with key >= from in ascending key order
  // (shm_scan_batch; the traversal of Tree::range_query, Tree.cpp:461-540):
  // keys[i] / vals[i] for i < the returned count (<= limit; == limit: there
  // may be more, keys[limit - 1] + 1 is the next from).  Host pointers.
  uint64_t scan(const Key& from, uint64_t limit, Key* keys, Value* vals) {
    return scan_dir(from, limit, keys, vals, false);
  }
  // The first `limit` valid entries with key <= from in descending key order
  // (shm_rscan_batch): as scan; from == kKeyMax starts at the largest stored
  // key, and keys[limit - 1] - 1 is the next from (unless that key is 0).
  uint64_t rscan(const Key& from, uint64_t limit, Key* keys, Value* vals) {
    return scan_dir(from, limit, keys, vals, true);
  }
  // The largest stored key <= k (an rscan of one): false when there is none.
  bool floor(const Key& k, Key& key_out, Value& val_out) {
    return rscan(k, 1, &key_out, &val_out) != 0;
  }

  // Replace the tree's contents with n pairs, keys strictly ascending
  // (shm_bulk_load; host pointers, copied to the device for the call).
  // leaf_fill entries per leaf (0: 36), internal_fill records per internal
  // page (0: 40).  False: the input was rejected (SHM_EINVAL: keys not
  // ascending, kKeyMax, a kValueNull value, fills out of range, a tree taller
  // than level 7) and the tree is as it was; other failures throw.
  bool bulk_load(const Key* keys, const Value* vals, uint64_t n, uint32_t leaf_fill = 0,
                 uint32_t internal_fill = 0) {
    uint64_t *d_k = nullptr, *d_v = nullptr;
    int s = SHM_OK;
    if (n) {
      if (!keys || !vals) return false;
      if (hipMalloc(&d_k, n * sizeof(uint64_t)) != hipSuccess ||
          hipMalloc(&d_v, n * sizeof(uint64_t)) != hipSuccess)
        s = SHM_ENOMEM;
      else if (hipMemcpy(d_k, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(d_v, vals, n * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess)
        s = SHM_EIO;
    }
    if (s == SHM_OK) s = shm_bulk_load(t_, d_k, d_v, n, leaf_fill, internal_fill, nullptr);
    if (d_k) (void)hipFree(d_k);
    if (d_v) (void)hipFree(d_v);
    if (s == SHM_EINVAL) return false;
    check(s, "bulk_load");
    return true;
  }

  // Every valid pair with lo <= key <= hi in ascending key order (shm_export;
  // host pointers, staged through device buffers like scan).  Returns the
  // count; when it is above cap nothing is copied.  keys or vals may be null
  // (that array is not exported); with both null the call only counts.
  uint64_t export_sorted(Key* keys, Value* vals, uint64_t cap, Key lo = 0, Key hi = ~0ull) {
    uint64_t n = 0;
    check(shm_export(t_, lo, hi, nullptr, nullptr, 0, &n, nullptr), "export count");
    if (n == 0 || n > cap || (!keys && !vals)) return n;
    uint64_t* d_out = nullptr;
    if (hipMalloc(&d_out, 2 * n * sizeof(uint64_t)) != hipSuccess)
      throw Error(SHM_ENOMEM, "export buffers");
    uint64_t m = 0;
    int s = shm_export(t_, lo, hi, keys ? d_out : nullptr, vals ? d_out + n : nullptr, n, &m,
                       nullptr);
    if (s == SHM_OK && m != n) s = SHM_EIO;  // the tree changed between the two calls
    if (s == SHM_OK &&
        ((keys && hipMemcpy(keys, d_out, n * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) ||
         (vals && hipMemcpy(vals, d_out + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost) !=
                      hipSuccess)))
      s = SHM_EIO;
    (void)hipFree(d_out);
    check(s, "export");
    return n;
  }
  // the number of valid pairs with lo <= key <= hi (shm_export's count pass)
  uint64_t count(Key lo = 0, Key hi = ~0ull) { return export_sorted(nullptr, nullptr, 0, lo, hi); }
  // Order statistics (shm_rank_batch / shm_count_batch / shm_select_batch as
  // batches of one; the first after a change of the tree rebuilds the order
  // index).  rank: the valid pairs with key < k, i.e. count(0, k - 1);
  // kKeyMax gives the total.
  uint64_t rank(const Key& k) {
    stage(k, nullptr);
    check(shm_rank_batch(t_, d_keys_, 1, d_vals_, nullptr, nullptr), "rank");
    return fetch(d_vals_, "rank copy-back");
  }
  // the valid pairs with from <= key <= to, what count(from, to) returns,
  // without reading the leaves between the two ends
  uint64_t count_range(const Key& from, const Key& to) {
    uint64_t h[2] = {from, to};
    if (hipMemcpy(d_keys_, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess)
      throw Error(SHM_EIO, "count stage");
    check(shm_count_batch(t_, d_keys_, d_keys_ + 1, 1, d_vals_, nullptr, nullptr), "count_range");
    return fetch(d_vals_, "count copy-back");
  }
  // the pair at position r (from 0) of the key order, element r of
  // export_sorted: false when r is not below the number of stored pairs
  bool select(uint64_t r, Key& key_out, Value& val_out) {
    stage(r, nullptr);
    check(shm_select_batch(t_, d_keys_, 1, d_vals_, d_vals_ + 1, d_found_, nullptr, nullptr),
          "select");
    uint8_t f = 0;
    if (hipMemcpy(&f, d_found_, 1, hipMemcpyDeviceToHost) != hipSuccess)
      throw Error(SHM_EIO, "select copy-back");
    if (!f) return false;
    key_out = fetch(d_vals_, "select copy-back");
    val_out = fetch(d_vals_ + 1, "select copy-back");
    return true;
  }
  // Rebuild the tree from its own valid pairs (shm_compact): the shape of
  // bulk_load(count(), leaf_fill, internal_fill), the pages deletes left behind
  // free again.  False: rejected before anything was written (SHM_EINVAL: fills
  // out of range, a tree taller than level 7; SHM_ENOMEM: the plan or the
  // temporary buffer does not fit) and the tree is as it was; other failures
  // throw.
  bool compact(uint32_t leaf_fill = 0, uint32_t internal_fill = 0) {
    const int s = shm_compact(t_, leaf_fill, internal_fill, nullptr);
    if (s == SHM_EINVAL || s == SHM_ENOMEM) return false;
    check(s, "compact");
    return true;
  }

  // Change the key range hint of the live tree (shm_tree_set_key_range): the
  // next reader rebuilds the directory over [key_lo, key_lo + 2^key_bits).
  // False: key_bits > 64 or an outstanding ordered chunk; other failures throw.
  bool set_key_range(Key key_lo, uint32_t key_bits) {
    const int s = shm_tree_set_key_range(t_, key_lo, key_bits);
    if (s == SHM_EINVAL) return false;
    check(s, "set_key_range");
    return true;
  }

  // batched hot path on device pointers (see include/sherman_amd.h)
  void search_batch(const Key* d_keys, uint64_t n, Value* d_vals,
                    uint8_t* d_found, hipStream_t s = nullptr) {
    check(shm_search_batch(t_, d_keys, n, d_vals, d_found, s), "search_batch");
  }
  void insert_batch(const Key* d_keys, const Value* d_vals, uint64_t n,
                    hipStream_t s = nullptr) {
    check(shm_insert_batch(t_, d_keys, d_vals, n, s), "insert_batch");
  }
  // one mixed batch: the gets see the tree before the batch's inserts
  void mixed_batch(const Key* d_get, uint64_t n_get, Value* d_vals, uint8_t* d_found,
                   const Key* d_ins, const Value* d_ins_vals, uint64_t n_ins,
                   hipStream_t s = nullptr) {
    check(shm_mixed_batch(t_, d_get, n_get, d_vals, d_found, d_ins, d_ins_vals, n_ins, s),
          "mixed_batch");
  }

  // Tree::print_and_check_tree (Tree.cpp:151-203) -> structural check
  void check_tree(uint64_t* leaves = nullptr, uint64_t* internal = nullptr,
                  uint64_t* keys = nullptr) {
    check(shm_check(t_, leaves, internal, keys), "check");
  }
  // the reference's name: checks the tree and prints its shape
  void print_and_check_tree(CoroContext* cxt = nullptr, int coro_id = 0) {
    (void)cxt;
    (void)coro_id;
    uint64_t leaves = 0, internal = 0, keys = 0;
    check_tree(&leaves, &internal, &keys);
    const shm_stats_t st = stats();
    printf("tree %u: height %u, %llu leaves, %llu internal pages, %llu keys\n",
           (unsigned)tree_id, st.height, (unsigned long long)leaves,
           (unsigned long long)internal, (unsigned long long)keys);
  }
  shm_stats_t stats() {
    shm_stats_t s;
    check(shm_stats(t_, &s), "stats");
    return s;
  }
  // Tree::lock_bench (Tree.cpp:310-321): take and release k's lock word
  void lock_bench(const Key& k, CoroContext* cxt = nullptr, int coro_id = 0) {
    (void)cxt;
    (void)coro_id;
    stage(k, nullptr);
    check(shm_lock_bench(t_, d_keys_, 1, nullptr), "lock_bench");
    check(shm_synchronize(t_), "lock_bench");
  }
  // Tree::index_cache_statistics / clear_statistics (Tree.cpp:1175-1185):
  // the index here is the leaf directory (or the LDS replica); its counters
  // are collected while enable_statistics(true)
  void enable_statistics(bool on) { check(shm_profile_enable(t_, on ? 2 : 0), "statistics"); }
  void index_cache_statistics() {
    shm_index_stats_t s;
    check(shm_index_stats(t_, &s, 0), "index statistics");
    const double g = s.gets ? (double)s.gets : 1.0;
    printf("index: %llu gets, %.4f start off a leaf, %.4f right moves, %.4f page hops, "
           "%.3f entry reads per get, %llu hits\n",
           (unsigned long long)s.gets, s.start_internal / g, s.right_moves / g, s.page_hops / g,
           s.entry_reads / g, (unsigned long long)s.hits);
  }
  void clear_statistics() {
    shm_index_stats_t s;
    check(shm_index_stats(t_, &s, 1), "clear statistics");
  }
  shm_tree* handle() { return t_; }

  const uint64_t tree_id;  // include/Tree.h:67 (one tree per handle here)

 private:
  uint64_t scan_dir(const Key& from, uint64_t limit, Key* keys, Value* vals, bool descending) {
    uint64_t *d_cnt = d_vals_, *d_out = nullptr;
    if (limit == 0 || limit >= (1ull << 31)) throw Error(SHM_EINVAL, "scan limit");
    if (hipMemcpy(d_keys_, &from, sizeof(from), hipMemcpyHostToDevice) != hipSuccess)
      throw Error(SHM_EIO, "scan stage");
    if (hipMalloc(&d_out, 2 * limit * sizeof(uint64_t)) != hipSuccess)
      throw Error(SHM_ENOMEM, "scan buffers");
    int s = (descending ? shm_rscan_batch : shm_scan_batch)(
        t_, d_keys_, nullptr, 1, limit, d_out, d_out + limit, d_cnt, nullptr, nullptr);
    uint64_t cnt = 0;
    if (s == SHM_OK && hipMemcpy(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess)
      s = SHM_EIO;
    if (s == SHM_OK && cnt &&
        (hipMemcpy(keys, d_out, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess ||
         hipMemcpy(vals, d_out + limit, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost) !=
             hipSuccess))
      s = SHM_EIO;
    (void)hipFree(d_out);
    check(s, descending ? "rscan" : "scan");
    return cnt;
  }
  void stage(const Key& k, const Value* v) {
    if (hipMemcpy(d_keys_, &k, sizeof(k), hipMemcpyHostToDevice) != hipSuccess)
      throw Error(SHM_EIO, "stage key");
    if (v && hipMemcpy(d_vals_, v, sizeof(*v), hipMemcpyHostToDevice) != hipSuccess)
      throw Error(SHM_EIO, "stage value");
  }
  // one result word back from the device (after the call that wrote it)
  uint64_t fetch(const uint64_t* d, const char* what) {
    uint64_t v = 0;
    if (hipMemcpy(&v, d, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) throw Error(SHM_EIO, what);
    return v;
  }
  void release() {
    if (d_keys_) (void)hipFree(d_keys_);
    if (d_vals_) (void)hipFree(d_vals_);
    if (d_found_) (void)hipFree(d_found_);
    d_keys_ = d_vals_ = nullptr;
    d_found_ = nullptr;
    if (t_) shm_tree_destroy(t_);
    t_ = nullptr;
  }
  shm_tree* t_ = nullptr;
  uint64_t* d_keys_ = nullptr;
  uint64_t* d_vals_ = nullptr;
  uint8_t* d_found_ = nullptr;
};

}  // namespace shm
