// tree_image.cpp — the tree as a whole: images, bulk load, export, key range.
//
// The calls that read or replace the whole tree on an idle device: the
// structural check of an image (check_image, shm_check), image dump and load,
// the bulk load of sorted pairs (bulk.hip), the sorted export of a key range
// and the compaction built from the two (export.hip), and the change of the
// shard's key range.  Each of those that replaces the tree's contents tells
// tree_dir.cpp (dir_invalidate) and rewrites the superblock.
#include "tree_internal.h"

namespace shm {
namespace host __attribute__((visibility("hidden"))) {

// host-side structural check of an image (same invariants as SURVEY App. A,
// and two the reference's check does not state: no key is valid in two slots
// of one leaf, -15, since a get answers from the first; and every child
// pointer of a level names a page the sibling walk of the level below
// visits, -16, since a stale copy of a page can carry the right lowest fence
// and level).  A page that hangs on its left sibling alone is visited, so the
// B-link state a failed take leaves passes.  tests/test_check_image.py pins
// every code.
int check_image(const uint8_t* img, uint64_t bytes, uint64_t root, uint16_t node,
                uint64_t* n_leaves, uint64_t* n_internal, uint64_t* n_keys) {
  auto rd64 = [&](uint64_t off) {
    uint64_t v;
    memcpy(&v, img + off, 8);
    return v;
  };
  auto page_off = [&](uint64_t ga) -> int64_t {
    if (ga == 0 || ga_node(ga) != node) return -1;
    const uint64_t o = ga_offset(ga);
    if (o < kPageSize || o + kPageSize > bytes || (o & (kPageSize - 1))) return -1;
    return (int64_t)o;
  };
  uint64_t leaves = 0, internals = 0, keys = 0;
  int64_t ro = page_off(root);
  if (ro < 0) return -1;
  int top = img[ro + kOffLevel];
  uint64_t head = root;
  // the children the level above named, then the pages this level's walk visits
  std::vector<uint64_t> named, kids, visited;
  for (int lvl = top; lvl >= 0; --lvl) {
    uint64_t p = head, expect_low = 0, next_head = 0;
    uint64_t guard = 0;
    kids.clear();
    visited.clear();
    while (p) {
      if (++guard > bytes / kPageSize + 1) return -20;
      const int64_t o = page_off(p);
      if (o < 0) return -2;
      const uint8_t* pg = img + o;
      const uint64_t leftmost = rd64(o + kOffLeftmost);
      const bool is_leaf = leftmost == 0;
      if (pg[kOffLevel] != lvl) return -3;
      if ((lvl == 0) != is_leaf) return -4;
      if (pg[kOffFrontVer] != pg[is_leaf ? kOffLeafRear : kOffInternalRear]) return -5;
      const uint64_t lo = rd64(o + kOffLowest), hi = rd64(o + kOffHighest);
      if (lo != expect_low || hi <= lo) return -6;
      visited.push_back((uint64_t)o);
      if (is_leaf) {
        int c = 0;
        uint64_t held[kLeafCardinality];
        for (int i = 0; i < kLeafCardinality; ++i) {
          const uint64_t e = o + kOffRecords + (uint64_t)kLeafEntry * i;
          if (rd64(e + 9) == kValueNull) continue;
          const uint64_t k = rd64(e + 1);
          if (k < lo || k >= hi) return -7;
          held[c++] = k;
        }
        if (c > kLeafCardinality - 1) return -8;
        std::sort(held, held + c);
        if (std::adjacent_find(held, held + c) != held + c) return -15;
        keys += (uint64_t)c;
        ++leaves;
      } else {
        int16_t li;
        memcpy(&li, pg + kOffLastIndex, 2);
        const int cnt = li + 1;
        if (cnt < 0 || cnt > kInternalCardinality - 1) return -9;
        if (!next_head) next_head = leftmost;
        int64_t co = page_off(leftmost);
        if (co < 0 || rd64(co + kOffLowest) != lo) return -10;
        kids.push_back((uint64_t)co);
        uint64_t prev = lo;
        for (int j = 0; j < cnt; ++j) {
          const uint64_t k = rd64(o + kOffRecords + 16ull * j);
          const uint64_t c = rd64(o + kOffRecords + 16ull * j + 8);
          if (k <= prev || k >= hi) return -11;
          prev = k;
          co = page_off(c);
          if (co < 0 || rd64(co + kOffLowest) != k) return -12;
          if ((int)img[co + kOffLevel] != lvl - 1) return -13;
          kids.push_back((uint64_t)co);
        }
        ++internals;
      }
      expect_low = hi;
      p = rd64(o + kOffSibling);
    }
    if (expect_low != kKeyMax) return -14;
    // the fences ascend along a walk, so it visits no page twice
    std::sort(visited.begin(), visited.end());
    for (const uint64_t c : named)
      if (!std::binary_search(visited.begin(), visited.end(), c)) return -16;
    named.swap(kids);
    head = next_head;
  }
  if (n_leaves) *n_leaves = leaves;
  if (n_internal) *n_internal = internals;
  if (n_keys) *n_keys = keys;
  return 0;
}
}  // namespace host
}  // namespace shm

extern "C" {

int shm_dump_image(shm_tree* t, void* host_buf, uint64_t cap,
                   uint64_t* bytes_used, uint64_t* root_ptr) {
  if (!t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  HIP_OK(hipDeviceSynchronize());
  mirror(t);
  const uint64_t used = t->next_page * kPageSize;
  if (bytes_used) *bytes_used = used;
  if (root_ptr) *root_ptr = t->root;
  if (!host_buf) return SHM_OK;
  if (cap < used) return SHM_EINVAL;
  HIP_OK(hipMemcpy(host_buf, t->arena, used, hipMemcpyDeviceToHost));
  return SHM_OK;
}

// The leaves a host image reaches from its root, one byte per page: the
// closure of the root under the child pointers of internal pages and the
// sibling pointers of all pages (a page that a missing separator left hanging
// on its left sibling alone is reached, as for every reader).  A pointer to
// another node, outside the image or off a page boundary is not followed
// (shm_check reports such an image); every page is visited once.
static void image_leaves(const uint8_t* img, uint64_t bytes, uint64_t pages, uint64_t root_ptr,
                         uint16_t node, std::vector<uint8_t>& leaf) {
  leaf.assign(pages, 0);
  std::vector<uint8_t> seen(pages, 0);
  std::vector<uint64_t> todo;
  auto u64_at = [&](uint64_t off) {
    uint64_t v;
    memcpy(&v, img + off, sizeof(v));
    return v;
  };
  auto push = [&](uint64_t ga) {
    const uint64_t off = ga_offset(ga);
    if (ga == 0 || ga_node(ga) != node || (off & (kPageSize - 1)) || off < kPageSize ||
        off + kPageSize > bytes)
      return;
    const uint64_t p = off / kPageSize;
    if (seen[p]) return;
    seen[p] = 1;
    todo.push_back(p);
  };
  push(root_ptr);
  while (!todo.empty()) {
    const uint64_t at = todo.back() * kPageSize;
    todo.pop_back();
    push(u64_at(at + kOffSibling));
    const uint64_t leftmost = u64_at(at + kOffLeftmost);
    if (leftmost == 0) {
      leaf[at / kPageSize] = img[at + kOffLevel] == 0;
      continue;
    }
    push(leftmost);
    int16_t last;
    memcpy(&last, img + at + kOffLastIndex, sizeof(last));
    const int n = last < 0 ? 0 : last >= kInternalCardinality ? kInternalCardinality : last + 1;
    for (int j = 0; j < n; ++j) push(u64_at(at + kOffRecords + kInternalEntry * j + 8));
  }
}

int shm_load_image(shm_tree* t, const void* host_buf, uint64_t bytes,
                   uint64_t root_ptr) {
  if (!t || !host_buf || bytes < 2 * kPageSize) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  const uint64_t pages = (bytes + kPageSize - 1) / kPageSize;
  if (pages > t->cap_pages || ga_node(root_ptr) != t->cfg.node_id) return SHM_EINVAL;
  const uint64_t ro = ga_offset(root_ptr);
  if (ro < kPageSize || ro + kPageSize > bytes) return SHM_EINVAL;
  HIP_OK(hipDeviceSynchronize());
  ++t->ord_gen;  // the pages change: the order index is of the tree before
  HIP_OK(hipMemcpy(t->arena, host_buf, bytes, hipMemcpyHostToDevice));
  // occupancy unknown for the loaded pages: whole-page reads until rewritten
  HIP_OK(hipMemset(t->leaf_hw, kLeafHwFull, t->cap_pages));
  // leaf summaries from the loaded pages: of the leaves the image reaches from
  // its root and of no other page, so no tag of the tree before it survives
  // and a page the image only carries along gets none (the page sweeps of the
  // directory's and the table's builds read tagged pages alone)
  HIP_OK(hipMemset(t->sum, 0, t->cap_pages * kSumBytes));
  {
    std::vector<uint8_t> leaf;
    image_leaves(static_cast<const uint8_t*>(host_buf), bytes, pages, root_ptr, t->cfg.node_id, leaf);
    uint8_t* d_leaf = nullptr;
    if (hipMalloc((void**)&d_leaf, pages) != hipSuccess) {
      (void)hipGetLastError();
      return SHM_ENOMEM;
    }
    hipError_t e = hipMemcpy(d_leaf, leaf.data(), pages, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      dev::launch_sum_rebuild(t->arena, pages, d_leaf, t->sum, nullptr);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(d_leaf);
    HIP_OK(e);
  }
  t->root = root_ptr;
  t->root_level = reinterpret_cast<const uint8_t*>(host_buf)[ro + kOffLevel];
  t->next_page = pages;
  dir_invalidate(t, false, false);  // contents changed
  Order ord(t, t->stream, true);
  return write_superblock(t, t->stream);
}

// The shape of a bulk-loaded tree: P0 = ceil(n / leaf_fill) leaves (one empty
// leaf for n == 0), ceil(P / (internal_fill + 1)) pages on each level above,
// the first level with one page the root.  Every level deals the C items
// below it over its P pages evenly (C / P each, one more for the first C % P).
// With internal_fill >= 2 every internal page gets at least two children:
// f = internal_fill + 1 >= 3 and P = ceil(C / f) <= (C + f - 1) / f; for
// C <= f the one page takes all C >= 2, and for C >= f + 1 the least share
// floor(C / P) is at least 2 because C f >= 2 (C + f - 1) follows from
// C (f - 2) >= (f + 1)(f - 2) >= 2 f - 2, i.e. f (f - 3) >= 0.
int shm_bulk_plan(uint64_t n, uint32_t leaf_fill, uint32_t internal_fill, shm_bulk_plan_t* out) {
  if (!out) return SHM_EINVAL;
  const uint64_t lf = leaf_fill ? leaf_fill : (uint32_t)kLeafSplitFill;
  const uint64_t inf = internal_fill ? internal_fill : (uint32_t)kInternalSplitFill;
  if (lf > (uint64_t)(kLeafCardinality - 1) || inf < 2 || inf > (uint64_t)(kInternalCardinality - 1))
    return SHM_EINVAL;
  shm_bulk_plan_t p{};
  uint64_t pages = n / lf + (n % lf ? 1 : 0);
  if (pages == 0) pages = 1;
  uint32_t level = 0;
  for (;; ++level) {
    if (level > (uint32_t)kMaxLevelOfTree) return SHM_EINVAL;
    p.level_pages[level] = pages;
    p.pages += pages;
    if (pages == 1) break;
    pages = pages / (inf + 1) + (pages % (inf + 1) ? 1 : 0);
  }
  p.root_level = level;
  *out = p;
  return SHM_OK;
}

// shm_bulk_load under t->mu, its arguments checked and its plan made
static int bulk_load_locked(shm_tree* t, const uint64_t* keys, const uint64_t* vals, uint64_t n,
                            const shm_bulk_plan_t& pl, hipStream_t s) {
  if (t->sync.n_pend) return SHM_EINVAL;  // an ordered chunk waits for its apply
  if (pl.pages + 1 > t->cap_pages) return SHM_ENOMEM;
  // exclusive and synchronising, as shm_load_image: after everything queued
  // before it on any stream
  HIP_OK(hipDeviceSynchronize());
  mirror(t);  // exact: the device is idle
  // word 15 of the device scratch: unused by the calls that share it (the
  // device is idle here in any case)
  uint32_t* status = reinterpret_cast<uint32_t*>(t->d_counts + 15);
  if (n) {
    // nothing is written before the input has passed
    HIP_OK(hipMemsetAsync(status, 0, sizeof(uint32_t), s));
    dev::launch_bulk_check(keys, vals, n, status, s);
    HIP_OK(hipGetLastError());
    if (const int rc = readback(t, s, status, sizeof(uint32_t))) return rc;
    if (reinterpret_cast<const uint32_t*>(t->h_pin)[0]) return SHM_EINVAL;
  }
  // the lowest fences of levels 1 .. root_level - 1, one array per level
  uint64_t low_words = 0;
  for (uint32_t l = 1; l < pl.root_level; ++l) low_words += pl.level_pages[l];
  if (low_words > t->bulk_low_words) {
    uint64_t* nl = nullptr;
    if (dalloc(&nl, low_words)) {
      (void)hipGetLastError();
      return SHM_ENOMEM;
    }
    if (t->bulk_low) (void)hipFree(t->bulk_low);
    t->bulk_low = nl;
    t->bulk_low_words = low_words;
  }
  const uint64_t old_next = t->next_page;
  const uint64_t new_next = pl.pages + 1;
  const uint16_t node = t->cfg.node_id;
  ++t->ord_gen;  // the pages change from here on: the order index is of the tree before
  // level l < root_level starts at page 2 + the pages of the levels below;
  // the root is page 1, as at create
  dev::BulkLeafArgs la{};
  la.arena = t->arena;
  la.node = node;
  la.keys = keys;
  la.vals = vals;
  la.pages = pl.level_pages[0];
  la.q = n / la.pages;
  la.r = n % la.pages;
  la.page0 = pl.root_level == 0 ? 1 : 2;
  la.sum = t->sum;
  la.leaf_hw = t->leaf_hw;
  dev::launch_bulk_leaves(la, s);
  uint64_t child0 = 2, low_at = 0;
  const uint64_t* low_in = nullptr;
  for (uint32_t l = 1; l <= pl.root_level; ++l) {
    const uint64_t below = pl.level_pages[l - 1];
    const bool root = l == pl.root_level;
    dev::BulkLevelArgs a{};
    a.arena = t->arena;
    a.node = node;
    a.level = l;
    a.keys = keys;
    a.leaf_q = la.q;
    a.leaf_r = la.r;
    a.low_in = low_in;
    a.low_out = root ? nullptr : t->bulk_low + low_at;
    a.pages = pl.level_pages[l];
    a.q = below / a.pages;
    a.r = below % a.pages;
    a.page0 = root ? 1 : child0 + below;
    a.child0 = child0;
    a.sum = t->sum;
    a.leaf_hw = t->leaf_hw;
    dev::launch_bulk_level(a, s);
    low_in = a.low_out;
    low_at += a.pages;
    child0 += below;
  }
  HIP_OK(hipGetLastError());
  // pages of the old tree past the new one keep no leaf tag
  if (old_next > new_next)
    HIP_OK(hipMemsetAsync(t->sum + new_next * kSumBytes, 0, (old_next - new_next) * kSumBytes, s));
  t->root = ga_make(node, kPageSize);
  t->root_level = pl.root_level;
  t->next_page = new_next;
  dir_invalidate(t, true, false);  // contents changed; the bucket table goes as well
  {
    Order ord(t, s, true);
    if (ord.rc) return ord.rc;
    if (const int rc = write_superblock(t, s)) return rc;
  }
  HIP_OK(hipStreamSynchronize(s));
  return SHM_OK;
}

int shm_bulk_load(shm_tree* t, const uint64_t* keys, const uint64_t* vals, uint64_t n,
                  uint32_t leaf_fill, uint32_t internal_fill, void* stream) {
  // the arguments first: a rejected call uses neither the handle nor the GPU
  if (n && (!keys || !vals)) return SHM_EINVAL;
  shm_bulk_plan_t pl{};
  if (const int rc = shm_bulk_plan(n, leaf_fill, internal_fill, &pl)) return rc;
  if (!t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  return bulk_load_locked(t, keys, vals, n, pl, pick(stream));
}

// ---- sorted export and compaction (export.hip) -----------------------------------
// The export in two halves, both under t->mu on an idle device: export_count
// runs the expansion and the leaf count pass and leaves the leaf list and its
// offsets in the workspace; export_write is the leaf write pass over them.
// Neither touches the tree, the directory, the bucket table or the counters.
static int export_ws(shm_tree* t, uint64_t pages) {
  if (pages <= t->ex_cap) return SHM_OK;
  // headroom, so a growing tree does not reallocate at every call
  const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(pages + pages / 4, 1024), t->cap_pages);
  uint64_t* nw = nullptr;
  if (dalloc(&nw, 6 * cap + dev::export_scan_tiles(cap) + 1)) {
    (void)hipGetLastError();
    return SHM_ENOMEM;
  }
  if (t->ex_ws) (void)hipFree(t->ex_ws);
  t->ex_ws = nw;
  t->ex_cap = cap;
  return SHM_OK;
}

static int export_count(shm_tree* t, hipStream_t s, uint64_t lo, uint64_t hi, uint64_t* n_out) {
  *n_out = 0;
  t->ex_units = 0;
  // it sees everything queued before it on any stream, and the mirror is exact
  HIP_OK(hipDeviceSynchronize());
  mirror(t);
  if (lo > hi || lo == kKeyMax) return SHM_OK;  // no stored key equals kKeyMax
  const uint64_t pages = t->next_page;
  if (const int rc = export_ws(t, pages)) return rc;
  const uint64_t cap = t->ex_cap;
  uint64_t* page[2] = {t->ex_ws, t->ex_ws + cap};
  uint64_t* bound[2] = {t->ex_ws + 2 * cap, t->ex_ws + 3 * cap};
  uint64_t* cnt = t->ex_ws + 4 * cap;
  uint64_t* off = t->ex_ws + 5 * cap;
  uint64_t* bsum = t->ex_ws + 6 * cap;
  uint64_t* tot = t->d_counts + 12;  // {total, error word}, as the range scans use it
  dev::ExportArgs a{};
  a.arena = t->arena;
  a.arena_bytes = t->arena_bytes;
  a.node = t->cfg.node_id;
  a.lo = lo;
  a.hi = hi;
  a.cnt = cnt;
  a.off = off;
  a.out_cap = cap;
  a.max_pages = pages;
  a.leaf_hw = t->leaf_hw;
  a.err = t->d_err;
  t->err_pending = true;
  int cur = 0;
  uint64_t n = 1;
  dev::launch_export_seed(t->root, page[0], bound[0], s);
  // one step per internal level: count, scan, one read of the total, emit
  auto counted = [&](uint64_t* total) -> int {
    dev::launch_export_scan(cnt, off, n, bsum, tot, t->d_err, s);
    HIP_OK(hipGetLastError());
    if (const int rc = readback(t, s, tot, 2 * sizeof(uint64_t))) return rc;
    *total = t->h_pin[0];
    // bits that are no error (a resumed chunk's) are taken and the export goes on
    return t->h_pin[1] ? check_err(t, s) : SHM_OK;
  };
  for (uint32_t level = t->root_level; level >= 1 && n; --level) {
    a.level = level;
    a.in_page = page[cur];
    a.in_bound = bound[cur];
    a.n = n;
    a.out_page = page[cur ^ 1];
    a.out_bound = bound[cur ^ 1];
    dev::launch_export_expand(a, false, s);
    uint64_t total = 0;
    if (const int rc = counted(&total)) return rc;
    if (total > cap) return SHM_EIO;  // more units than pages: not a tree
    dev::launch_export_expand(a, true, s);
    cur ^= 1;
    n = total;
  }
  if (n == 0) return check_err(t, s);
  a.level = 0;
  a.in_page = page[cur];
  a.in_bound = bound[cur];
  a.n = n;
  a.out_page = a.out_bound = nullptr;
  dev::launch_export_leaf(a, false, s);
  uint64_t total = 0;
  if (const int rc = counted(&total)) return rc;
  t->ex_cur = cur;
  t->ex_units = n;
  *n_out = total;
  return SHM_OK;
}

}  // extern "C"

namespace shm {
namespace host __attribute__((visibility("hidden"))) {
int order_count(shm_tree* t, hipStream_t s, const uint64_t** page, const uint64_t** bound,
                const uint64_t** off, const uint64_t** total_dev, uint64_t* total) {
  if (const int rc = export_count(t, s, 0, kKeyMax, total)) return rc;
  if (t->ex_units == 0) return SHM_EIO;  // the root alone is a unit: not a tree
  const uint64_t cap = t->ex_cap;
  *page = t->ex_ws + (uint64_t)t->ex_cur * cap;
  *bound = t->ex_ws + (2 + (uint64_t)t->ex_cur) * cap;
  *off = t->ex_ws + 5 * cap;
  *total_dev = t->d_counts + 12;  // export_count's {total, error word}
  return SHM_OK;
}
}  // namespace host
}  // namespace shm

extern "C" {

// the pairs of the last export_count (lo, hi as there; total = its count)
static int export_write(shm_tree* t, hipStream_t s, uint64_t lo, uint64_t hi, uint64_t* keys,
                        uint64_t* vals, uint64_t total) {
  if (t->ex_units && total) {
    const uint64_t cap = t->ex_cap;
    dev::ExportArgs a{};
    a.arena = t->arena;
    a.arena_bytes = t->arena_bytes;
    a.node = t->cfg.node_id;
    a.lo = lo;
    a.hi = hi;
    a.in_page = t->ex_ws + (uint64_t)t->ex_cur * cap;
    a.in_bound = t->ex_ws + (2 + (uint64_t)t->ex_cur) * cap;
    a.n = t->ex_units;
    a.off = t->ex_ws + 5 * cap;
    a.keys = keys;
    a.vals = vals;
    a.total = total;
    a.max_pages = t->next_page;
    a.leaf_hw = t->leaf_hw;
    a.err = t->d_err;
    t->err_pending = true;
    dev::launch_export_leaf(a, true, s);
    HIP_OK(hipGetLastError());
  }
  // synchronising: the outputs are complete, and the walks' error bits read
  return check_err(t, s);
}

int shm_export(shm_tree* t, uint64_t lo, uint64_t hi, uint64_t* keys_out, uint64_t* vals_out,
               uint64_t cap, uint64_t* n_out, void* stream) {
  // the arguments first: a rejected call uses neither the handle nor the GPU
  if (!n_out || !t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  hipStream_t s = pick(stream);
  Order ord(t, s, true);  // the export workspace; later calls follow the export
  if (ord.rc) return ord.rc;
  uint64_t total = 0;
  if (const int rc = export_count(t, s, lo, hi, &total)) return rc;
  *n_out = total;
  const bool out = keys_out || vals_out;
  if (out && total > cap) {
    const int rc = check_err(t, s);
    return rc ? rc : SHM_ENOSPC;  // nothing was written
  }
  return export_write(t, s, lo, hi, out ? keys_out : nullptr, out ? vals_out : nullptr,
                      out ? total : 0);
}

int shm_compact(shm_tree* t, uint32_t leaf_fill, uint32_t internal_fill, void* stream) {
  // the fills first: a rejected call uses neither the handle nor the GPU
  shm_bulk_plan_t pl{};
  if (const int rc = shm_bulk_plan(0, leaf_fill, internal_fill, &pl)) return rc;
  if (!t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  if (t->sync.n_pend) return SHM_EINVAL;  // an ordered chunk waits for its apply
  hipStream_t s = pick(stream);
  uint64_t n = 0;
  {
    Order ord(t, s, true);
    if (ord.rc) return ord.rc;
    if (const int rc = export_count(t, s, 0, kKeyMax, &n)) return rc;
  }
  // everything that can fail, before the first page is written
  int rc = shm_bulk_plan(n, leaf_fill, internal_fill, &pl);
  if (!rc && pl.pages + 1 > t->cap_pages) rc = SHM_ENOMEM;
  uint64_t* pairs = nullptr;
  if (!rc && n && dalloc(&pairs, 2 * n)) {
    (void)hipGetLastError();
    rc = SHM_ENOMEM;
  }
  if (rc) {
    const int e = check_err(t, s);
    return e ? e : rc;
  }
  rc = export_write(t, s, 0, kKeyMax, pairs, pairs ? pairs + n : nullptr, n);
  // the load's own input check runs on the exported run: a cross-check of the export
  if (!rc) rc = bulk_load_locked(t, pairs, pairs ? pairs + n : nullptr, n, pl, s);
  if (pairs) (void)hipFree(pairs);
  return rc;
}

// Library-internal (shard.cpp shm_shard_rebalance): the whole tree exported
// into a fresh device buffer the caller frees with hipFree, keys in
// (*pairs_out)[0, n), values in [n, 2 n) (nullptr for n == 0), as shm_compact
// takes it.  Read-only.  SHM_EINVAL with an outstanding shm_insert_order
// ticket: the load that follows would refuse it.
int shm__export_all(shm_tree* t, uint64_t** pairs_out, uint64_t* n_out, void* stream) {
  if (!t || !pairs_out || !n_out) return SHM_EINVAL;
  *pairs_out = nullptr;
  *n_out = 0;
  std::lock_guard<std::mutex> g(t->mu);
  if (t->sync.n_pend) return SHM_EINVAL;
  hipStream_t s = pick(stream);
  Order ord(t, s, true);
  if (ord.rc) return ord.rc;
  uint64_t n = 0;
  if (const int rc = export_count(t, s, 0, kKeyMax, &n)) return rc;
  uint64_t* pairs = nullptr;
  if (n && dalloc(&pairs, 2 * n)) {
    (void)hipGetLastError();
    const int e = check_err(t, s);
    return e ? e : SHM_ENOMEM;
  }
  const int rc = export_write(t, s, 0, kKeyMax, pairs, pairs ? pairs + n : nullptr, n);
  if (rc) {
    if (pairs) (void)hipFree(pairs);
    return rc;
  }
  *pairs_out = pairs;
  *n_out = n;
  return SHM_OK;
}

int shm_tree_set_key_range(shm_tree* t, uint64_t key_lo, uint32_t key_bits) {
  // the arguments first: a rejected call uses neither the handle nor the GPU
  if (key_bits > 64 || !t) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  if (t->sync.n_pend) return SHM_EINVAL;  // an ordered chunk was partitioned by the old range
  // exclusive and synchronising, as shm_bulk_load: every launch that took the
  // old range in its arguments (gets, the chunks' directory and table upkeep)
  // has run before the range changes
  HIP_OK(hipDeviceSynchronize());
  mirror(t);
  if (const int rc = dir_poll(t, true)) return rc;
  if (const int rc = vt_poll(t, true)) return rc;
  t->cfg.key_bits = key_bits ? key_bits : 64;
  t->cfg.key_lo = t->cfg.key_bits == 64 ? 0 : key_lo;
  // what the old range laid out, as shm_bulk_load drops it: the next reader
  // builds the directory (its entry count from the new key_bits: dir_bits_for),
  // the level hints and the bucket table over the new range
  dir_invalidate(t, true, true);
  return SHM_OK;
}

// test hook: check_image on host memory, its raw code in *code (0 = sound)
// and counts3 = {leaves, internal pages, valid keys} of a sound image.  No
// handle and no GPU, like shm__order_limits (tests/test_check_image.py).
int shm__check_image(const void* img, uint64_t bytes, uint64_t root, uint16_t node,
                     uint64_t* counts3, int* code) {
  if (!img || !code) return SHM_EINVAL;
  uint64_t c[3] = {0, 0, 0};
  *code = check_image(static_cast<const uint8_t*>(img), bytes, root, node, c, c + 1, c + 2);
  if (counts3) memcpy(counts3, c, sizeof(c));
  return SHM_OK;
}

// test hook: the side state of the pages, for a host-side check that shares
// no code with the kernels (tests/state_model.py), in the style of
// shm__dir_dump.  info = {next_page, cap_pages}; with buffers given
// (nullable: sizes only) the summary lines (kSumBytes each) and the
// occupancy bytes of the first min(cap_pages, the arena's pages) pages: the
// caller may ask past next_page.
int shm__side_dump(shm_tree* t, void* sum_out, void* hw_out, uint64_t cap_pages, uint64_t* info) {
  if (!t || !info) return SHM_EINVAL;
  std::lock_guard<std::mutex> g(t->mu);
  HIP_OK(hipDeviceSynchronize());
  mirror(t);
  info[0] = t->next_page;
  info[1] = t->cap_pages;
  const uint64_t n = std::min(cap_pages, t->cap_pages);
  if (sum_out && n) HIP_OK(hipMemcpy(sum_out, t->sum, n * kSumBytes, hipMemcpyDeviceToHost));
  if (hw_out && n) HIP_OK(hipMemcpy(hw_out, t->leaf_hw, n, hipMemcpyDeviceToHost));
  return SHM_OK;
}

int shm_check(shm_tree* t, uint64_t* n_leaves, uint64_t* n_internal,
              uint64_t* n_keys) {
  if (!t) return SHM_EINVAL;
  uint64_t used = 0, root = 0;
  int rc = shm_dump_image(t, nullptr, 0, &used, &root);
  if (rc) return rc;
  std::vector<uint8_t> img(used);
  rc = shm_dump_image(t, img.data(), used, &used, &root);
  if (rc) return rc;
  rc = check_image(img.data(), used, root, t->cfg.node_id, n_leaves, n_internal, n_keys);
  if (rc) {
    fprintf(stderr, "sherman_amd: structural check failed (%d)\n", rc);
    return SHM_EIO;
  }
  return SHM_OK;
}
}  // extern "C"
