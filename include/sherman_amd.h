/*
 * sherman_amd.h — C-ABI of the MI355X-native Sherman B+tree hot path.
 *
 * Plain C: opaque handle, plain pointers and sizes, int status codes. No HIP,
 * torch or C++ types appear in the signatures (streams are passed as void*,
 * i.e. a hipStream_t cast; NULL = the HIP null/default stream).
 *
 * Every batch entry point takes DEVICE pointers (HBM of the tree's GPU). The
 * host C++ facade (sherman_amd/csrc/Tree.hpp) provides the reference's
 * single-op, host-pointer Tree API on top of these.
 *
 * Reference interface each entry point replaces (paths relative to the
 * Sherman source tree, cmemory/Sherman):
 *   shm_tree_create     Tree::Tree(DSM*, uint16_t)        include/Tree.h:45,  src/Tree.cpp:27-61
 *                       + DSM::getInstance / alloc        include/DSM.h:33-40, 198-224
 *   shm_tree_destroy    (process teardown; DSM is a singleton, src/DSM.cpp:23-35)
 *   shm_search_batch    Tree::search(const Key&, Value&)  include/Tree.h:49-50, src/Tree.cpp:405-459
 *   shm_insert_batch    Tree::insert(const Key&, const Value&)
 *   shm_insert_batch_async                                include/Tree.h:47-48, src/Tree.cpp:353-403
 *   shm_mixed_batch     Tree::search + Tree::insert of one mixed op stream
 *                       (test/benchmark.cpp:165-188)
 *   shm_del_batch       Tree::del(const Key&)             include/Tree.h:51,   src/Tree.cpp:542-591
 *   shm_range_query     Tree::range_query(from, to, Value*)
 *                                                         include/Tree.h:53-54, src/Tree.cpp:461-540
 *   shm_scan_batch / shm_rscan_batch
 *                       (no reference counterpart beyond Tree::range_query's
 *                        traversal: ordered scans with a count limit, upwards
 *                        and downwards)
 *   shm_bulk_plan / shm_bulk_load
 *                       (no reference counterpart: the reference fills a tree
 *                        by Tree::insert alone, test/benchmark.cpp:150-158)
 *   shm_export / shm_compact
 *                       (no reference counterpart beyond Tree::range_query's
 *                        traversal; the reference never frees a page,
 *                        include/LocalAllocator.h:45-47)
 *   shm_rank_batch / shm_count_batch / shm_select_batch
 *                       (no reference counterpart beyond Tree::range_query's
 *                        traversal and validity rule: order statistics)
 *   shm_stats           Tree::print_and_check_tree / index_cache_statistics
 *                                                         include/Tree.h:56, 62; src/Tree.cpp:151-203
 *   shm_dump_image / shm_load_image
 *                       the MN arena + root pointer (src/DSM.cpp:37-53, src/Tree.cpp:90-114)
 *   shm_route_*         (no reference counterpart: the multi-GPU key routing
 *                        that replaces DSM chunk round-robin, include/DSM.h:198-224)
 *   shm_shard_*         a Tree spread over memory nodes: DSM::alloc's chunk
 *                       round-robin over nodes (include/DSM.h:198-224) and the
 *                       remote page reads of Tree::search / Tree::insert
 *                       (src/Tree.cpp:353-459), here range shards over RCCL
 */
#ifndef SHERMAN_AMD_H
#define SHERMAN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHM_ABI_VERSION 11

/* status codes (negative errno style) */
#define SHM_OK 0
#define SHM_EINVAL (-22)   /* bad argument, key == UINT64_MAX (kKeyMax) */
#define SHM_ENOMEM (-12)   /* page arena or workspace exhausted */
#define SHM_EIO (-5)       /* HIP failure or tree inconsistency detected */
#define SHM_EAGAIN (-11)   /* optimistic version/lock check failed */
#define SHM_E2BIG (-7)     /* batch larger than cfg.max_batch */
#define SHM_ENOSPC (-28)   /* output buffer too small (size reported) */

/* flags for shm_config.flags */
#define SHM_FLAG_SORT_GETS 0x1u  /* reorder gets by key and walk whole pages
                                    (k_get) instead of the leaf summaries */
#define SHM_FLAG_LEAF_DIR 0x2u   /* start gets / leaf locates at the leaf
                                    directory (default on) */
#define SHM_FLAG_AUTO_SORT_GETS 0x4u /* accepted; since ABI 5 no batch is
                                    reordered unless SHM_FLAG_SORT_GETS: the
                                    leaf-summary walk reads ~3 lines per get
                                    and ordering never pays */
#define SHM_FLAG_PAGE_CHECK 0x10u /* the batched get also checks the page-level
                                    version (front == rear, Tree.h:241-261) of
                                    every page it takes a value from, and
                                    reports a torn page as SHM_EIO; off by
                                    default: gets never overlap writers
                                    (exclusive calls), and it costs two lines
                                    per get */
#define SHM_FLAG_TOP_LDS 0x8u    /* without SHM_FLAG_LEAF_DIR: gets start from
                                    an LDS replica of the top of the tree (the
                                    pages of the deepest upper level that fits
                                    4096 entries) instead of the root */

typedef struct shm_tree shm_tree;

typedef struct shm_config {
  uint32_t struct_size;  /* sizeof(shm_config) */
  int32_t device;        /* HIP device ordinal */
  uint16_t node_id;      /* GlobalAddress.nodeID of this shard (= GPU id) */
  uint16_t reserved0;
  uint32_t flags;        /* SHM_FLAG_* */
  uint64_t arena_bytes;  /* HBM page arena (1 KB pages), at most 4 TB (else SHM_EINVAL) */
  uint64_t max_batch;    /* ops per device chunk of a batch call (< 2^24) */
  uint32_t num_locks;    /* HBM lock table words (reference: 16384) */
  uint32_t sort_bits;    /* top key bits that order gets: 0 or 16 */
  /* key range hint: this shard's keys lie in [key_lo, key_lo + 2^key_bits)
   * (a range shard of a multi-GPU tree; key_bits = 64: the whole key space).
   * It only steers the get ordering and the leaf directory; keys outside it
   * are still stored and found exactly. */
  uint64_t key_lo;
  uint32_t key_bits;     /* 1..64 (0 is read as 64) */
  uint32_t reserved1;
} shm_config;

typedef struct shm_stats_t {
  uint64_t root_ptr;      /* GlobalAddress of the root page */
  uint32_t root_level;    /* level of the root (leaves are level 0) */
  uint32_t height;        /* root_level + 1 */
  uint64_t pages_used;    /* allocated 1 KB pages (excluding superblock) */
  uint64_t pages_capacity;
  uint64_t arena_bytes;
  uint64_t batches;       /* mutating batches applied */
  uint64_t splits;        /* leaf + internal pages created by splits */
  uint32_t last_error;    /* sticky device error bits (0 = none) */
  uint32_t reserved;
} shm_stats_t;

/* lifecycle ------------------------------------------------------------------ */
int shm_config_init(shm_config *cfg);
int shm_tree_create(const shm_config *cfg, shm_tree **out);
int shm_tree_destroy(shm_tree *t);
/* cfg.max_batch of the handle (the largest chunk one batch call processes) */
uint64_t shm_tree_max_batch(const shm_tree *t);
const char *shm_strerror(int status);
int shm_abi_version(void);

/* batched hot path (device pointers) ------------------------------------------ */
/* vals_out[i] = value of keys[i] (0 if absent); found_out[i] = 1/0.
 * found_out may be NULL. Reads only.
 * The rule for every reader and every builder of an index that a reader
 * trusts (the leaf directory, the key-value bucket table, the leaf summaries):
 * NO DATA IS TAKEN FROM A PAGE THE TREE DOES NOT REACH FROM ITS ROOT (through
 * child and sibling pointers).  Below pages_used such pages exist -- pages a
 * failed take lost (shm_insert_batch, SHM_ENOMEM), pages of an earlier tree
 * that a smaller shm_bulk_load or shm_load_image left behind, pages a loaded
 * image carries along -- and their bytes may be those of a leaf with valid
 * entries.  A get answers what the tree holds, whatever they hold.
 * Streams: searches issued on distinct streams may run concurrently on the
 * device (an ordered batch uses one of two internal workspaces, alternating,
 * so consecutive batches on two streams overlap one's ordering with the
 * other's walk).  Every other call (insert, delete, range, routing, a
 * directory rebuild) is ordered on the device after all calls issued before
 * it on any stream, and before all calls issued after it: results follow
 * the host's call order. */
int shm_search_batch(shm_tree *t, const uint64_t *keys, uint64_t n,
                     uint64_t *vals_out, uint8_t *found_out, void *stream);
/* Upsert keys[i] -> vals[i] in batch order (last writer in the batch wins).
 * vals[i] == 0 (kValueNull) deletes keys[i]. Mutating calls on one handle are
 * serialised internally. Returns once the batch has been applied on `stream`
 * (one host synchronisation, for the status): SHM_EINVAL if the batch held
 * kKeyMax (the max_batch chunk holding it is rejected whole; the call's other
 * chunks, before and after it, are applied), SHM_ENOMEM if the arena ran out
 * (the splits that did not fit are left unapplied), SHM_EIO on a device fault
 * or a tree inconsistency the kernels detected (shm_last_error names the
 * bits and the chunk that first saw them).
 * After SHM_ENOMEM (tests/test_gpu_arena_full.py):
 *  - A leaf whose split did not fit keeps every entry it had: all ops of the
 *    chunk that fall inside its fences (new keys and overwrites alike) are
 *    left unapplied, together.  Every other op of the chunk is applied, the
 *    deletes included (they run after the splits).  So each key is either as
 *    it was before the chunk or as the whole chunk would have left it.
 *  - The pages of a split are not taken all at once: when the leaf level
 *    fitted and an internal level did not, the new pages exist, hold their
 *    keys and are reached through their left sibling alone (their separator
 *    is missing one level up, and stays missing).  That is a legal B-link
 *    state, which every reader follows and shm_check accepts; the allocation
 *    was not made all-or-nothing for a whole path.
 *  - Every reader (gets by any path: bucket table, directory, summary or
 *    page walk; scans, lower bounds, range queries) answers what the pages
 *    hold, also a get queued behind the failing chunk before the host has
 *    seen the status: the chunk's directory and table upkeep reads what the
 *    tree did when the device error word holds the bit.
 *  - The handle stays usable: ops that need no new page (overwrites,
 *    deletes, new keys in leaves with room) return SHM_OK, a chunk that needs
 *    a page returns SHM_ENOMEM again.  pages_used never exceeds
 *    pages_capacity; a failed take counts the free pages that were left
 *    (fewer than it asked for) as used, so those are lost to later chunks.
 * A chunk whose split propagation
 * gave up waiting (a hand-off bound) is completed in the same launch by its
 * last block alone, before any later call reads the tree (counted in
 * shm_error_t.resumed; not an error), as the reference always completes a
 * parent insert (src/Tree.cpp:973-988). */
int shm_insert_batch(shm_tree *t, const uint64_t *keys, const uint64_t *vals,
                     uint64_t n, void *stream);
/* The same batch queued on `stream` without any host wait (the reference's
 * Tree::insert returns nothing either, include/Tree.h:47-48): ordering, leaf
 * upserts, splits, parent levels and root growth all run on the device.  The
 * status of the batch is reported by the next synchronising call on the
 * handle (shm_synchronize, shm_insert_batch, shm_del_batch) as above. */
int shm_insert_batch_async(shm_tree *t, const uint64_t *keys, const uint64_t *vals,
                           uint64_t n, void *stream);
/* shm_insert_batch_async of one chunk (n <= max_batch) split in two calls,
 * so a caller can order the next batch while this one applies:
 * shm_insert_order queues the batch's ordering (last writer per key, sorted,
 * upserts / deletes split; it reads only keys / vals and touches no tree
 * state) on `stream` and returns a ticket; shm_insert_apply queues the tree
 * changes of that ticket (locate, leaf upserts, splits, parent levels,
 * deletes) on its own stream, ordered like any insert (after every earlier
 * call on the handle, before every later one).  At most two tickets are
 * outstanding (SHM_EAGAIN), applied oldest first (else SHM_EINVAL); other
 * insert calls are refused (SHM_EINVAL) while a ticket is outstanding.
 * The ordering reuses the buffers of the chunk two tickets back: when that
 * chunk was applied on another stream, shm_insert_order waits on the host
 * until the device has finished with them (flow control: a pipelined caller
 * stays about two chunks ahead of the device; after 2 s it queues a
 * device-side wait instead and returns).
 * Once per 2^32 - 1 chunks (see shm_last_chunk) shm_insert_order returns
 * SHM_EAGAIN with a single ticket outstanding: the chunk ids start over and
 * the chunk of that ticket must be applied under its old id first.  Apply it
 * and call again.
 * An empty chunk (n == 0; keys / vals may be null) takes no chunk id and
 * queues nothing: shm_insert_order returns SHM_OK with ticket 0, also while
 * two tickets are outstanding, and shm_insert_apply of ticket 0 returns
 * SHM_OK at any time and leaves the tree and the outstanding tickets as they
 * are.  No chunk has id 0.
 * Errors are reported as for shm_insert_batch_async.  Tree::insert
 * (src/Tree.cpp:353-403) for a batch, as shm_insert_batch_async. */
int shm_insert_order(shm_tree *t, const uint64_t *keys, const uint64_t *vals, uint64_t n,
                     void *stream, uint32_t *ticket);
int shm_insert_apply(shm_tree *t, uint32_t ticket, void *stream);
/* One mixed batch of gets and inserts (the reference benchmark's op stream,
 * test/benchmark.cpp:165-188, cut into batches): the gets see the tree as it
 * was before the batch's inserts, the inserts apply as shm_insert_batch_async
 * (the batch's status is reported by the next synchronising call).  Device
 * pointers; found_out nullable. */
int shm_mixed_batch(shm_tree *t, const uint64_t *get_keys, uint64_t n_get, uint64_t *vals_out,
                    uint8_t *found_out, const uint64_t *ins_keys, const uint64_t *ins_vals,
                    uint64_t n_ins, void *stream);
/* Tree::del for every key. */
int shm_del_batch(shm_tree *t, const uint64_t *keys, uint64_t n, void *stream);
/* Batched inclusive range scans [from[i], to[i]]: values of valid entries in
 * leaf order then slot order.  counts_out[i] = number of matches; values are
 * written to vals_out[offsets[i] ...] only when offsets != NULL (call once
 * with offsets == NULL to size, then again with an exclusive scan). */
int shm_range_query(shm_tree *t, const uint64_t *from, const uint64_t *to,
                    uint64_t n, uint64_t *counts_out, const uint64_t *offsets,
                    uint64_t *vals_out, void *stream);
/* The same scans sized in one call: counts_out, offsets_out (exclusive scan
 * of the counts, absolute) and *total_out are always produced (one host
 * synchronisation); the values are written to vals_out when total <=
 * vals_cap, else SHM_ENOSPC is returned and the caller fills a larger buffer
 * with shm_range_query(..., offsets_out, vals). */
int shm_range_query_batch(shm_tree *t, const uint64_t *from, const uint64_t *to,
                          uint64_t n, uint64_t *counts_out, uint64_t *offsets_out,
                          uint64_t *vals_out, uint64_t vals_cap, uint64_t *total_out,
                          void *stream);
/* The same scans without a host synchronisation, for one chunk (n <=
 * cfg.max_batch): total_dev (device, 2 words) receives the total and the
 * device error bits when the call completes on `stream`; values at output
 * index >= vals_cap are dropped, so the caller compares total_dev[0] with
 * vals_cap when it reads the result (the reference leaves sizing the buffer
 * to the caller too, Tree.cpp:513, 532).  Lets a caller queue further work
 * (e.g. the batch's inserts) behind the scans without waiting for them. */
int shm_range_query_batch_async(shm_tree *t, const uint64_t *from, const uint64_t *to,
                                uint64_t n, uint64_t *counts_out, uint64_t *offsets_out,
                                uint64_t *vals_out, uint64_t vals_cap, uint64_t *total_dev,
                                void *stream);
/* Tree::range_query(from, to, Value *buffer) for a batch, each scan with a
 * buffer of its own, as the reference's caller passes one per call
 * (src/Tree.cpp:461-540, include/Tree.h:53): scan i's values, in leaf then
 * slot order, go to vals_out[i * slot_cap ...] (at most slot_cap of them) and
 * counts_out[i] = its number of matches (the reference's return value; more
 * than slot_cap means the buffer was too small and holds the first
 * slot_cap).  One pass over the leaves, no host synchronisation, any n.
 * status_dev (device, 2 words, nullable): the call ADDS the number of scans
 * whose count passed slot_cap to status_dev[0] and ORs its device error bits
 * into status_dev[1] when it completes on `stream` (the caller zeroes the
 * pair; several batches may accumulate into one, checked once). */
int shm_range_query_slots(shm_tree *t, const uint64_t *from, const uint64_t *to,
                          uint64_t n, uint64_t slot_cap, uint64_t *counts_out,
                          uint64_t *vals_out, uint64_t *status_dev, void *stream);
/* Ordered scans with a count limit (YCSB-E's scan(start, count), lower_bound,
 * cursor paging): scan i returns the first min(limit, matches) valid entries
 * with from[i] <= key <= to[i] (to == NULL: no upper bound) in ascending
 * unsigned key order, keys to keys_out[i * limit ...] and values to
 * vals_out[i * limit ...]; counts_out[i] = the number of pairs written (at
 * most limit; == limit means there may be more: the last key + 1 is the next
 * from).  The rest of a scan's row is not written.  from[i] > to[i] and
 * from[i] == kKeyMax give 0.  The traversal (the leaf holding `from`, then the
 * sibling chain) and the validity rule (value != kValueNull, front == rear
 * entry version) are Tree::range_query's (src/Tree.cpp:461-540,
 * include/Tree.h:53-54); the order inside a leaf, the keys and the early stop
 * are new.  Device pointers, no host synchronisation, any n; queued like
 * shm_range_query_slots.  status_dev (device, 2 words, nullable): the call
 * ORs its device error bits into status_dev[1] and leaves status_dev[0]
 * alone.  n == 0 launches nothing; limit == 0, limit >= 2^31 or a null from /
 * keys_out / vals_out / counts_out with n > 0 is SHM_EINVAL. */
int shm_scan_batch(shm_tree *t, const uint64_t *from, const uint64_t *to, uint64_t n,
                   uint64_t limit, uint64_t *keys_out, uint64_t *vals_out,
                   uint64_t *counts_out, uint64_t *status_dev, void *stream);
/* The same scans downwards (floor / predecessor, the maximum key, paging
 * backwards): scan i returns the first min(limit, matches) valid entries with
 * to[i] <= key <= from[i] (to == NULL: a stop of 0, no lower bound) in
 * DESCENDING unsigned key order, keys to keys_out[i * limit ...] and values
 * to vals_out[i * limit ...]; counts_out[i] = the number of pairs written (at
 * most limit; == limit means there may be more: the last key - 1 is the next
 * from, unless the last key is 0).  The rest of a scan's row is not written.
 * to[i] > from[i] gives 0.  from[i] == kKeyMax is allowed and means "from the
 * largest stored key" (no stored key equals kKeyMax, so unlike
 * shm_scan_batch's from == kKeyMax it is not empty).  The leaf chain has no
 * left links: a step to the left is a descent to the leaf holding the current
 * leaf's lowest fence - 1 (a leaf directory entry plus the page; a descent
 * from the root without the directory), which also follows the B-link right
 * turns of a missing separator.  Validity, arguments, status_dev, queueing
 * and the SHM_EINVAL cases are shm_scan_batch's. */
int shm_rscan_batch(shm_tree *t, const uint64_t *from, const uint64_t *to, uint64_t n,
                    uint64_t limit, uint64_t *keys_out, uint64_t *vals_out,
                    uint64_t *counts_out, uint64_t *status_dev, void *stream);

/* introspection / images (host pointers) ------------------------------------- */
int shm_stats(shm_tree *t, shm_stats_t *out);
/* Copy the arena (superblock + pages) to host memory. *bytes_used receives
 * the number of bytes that hold pages; *root_ptr the root GlobalAddress. */
int shm_dump_image(shm_tree *t, void *host_buf, uint64_t cap,
                   uint64_t *bytes_used, uint64_t *root_ptr);
/* Replace the tree with a page image laid out by the reference format
 * (pages at GlobalAddress offsets, nodeID == cfg.node_id).  Every byte of the
 * image is copied, so shm_dump_image gives it back; but the tree is what
 * root_ptr reaches through child and sibling pointers, found by one walk
 * over the host buffer (every reached page read once), and only the leaves
 * it reaches are described to the readers' indexes.  A page the image merely
 * carries along (see the rule at shm_search_batch) is never read as data,
 * even where its bytes are those of a leaf.  Pointers to another node,
 * outside the image or off a page boundary are not followed (shm_check
 * reports such a tree). */
int shm_load_image(shm_tree *t, const void *host_buf, uint64_t bytes,
                   uint64_t root_ptr);
/* Bulk load: the tree of a sorted run of pairs, written in one pass.
 *
 * shm_bulk_plan is the shape such a load gives, by host arithmetic alone (no
 * handle, no GPU).  leaf_fill = entries per leaf, 1..53 (0: 36, the fill of a
 * batched leaf split); internal_fill = records per internal page, 2..60, so
 * children = records + 1 (0: 40); any other value is SHM_EINVAL.  Level 0 has
 * P0 = ceil(n / leaf_fill) leaves (n == 0: one empty leaf, the tree of
 * shm_tree_create), level l >= 1 has ceil(P(l-1) / (internal_fill + 1)) pages,
 * and the first level with a single page is the root; a root above level 7
 * (kMaxLevelOfTree) is SHM_EINVAL.  Every level deals the C items below it
 * (pairs for leaves, children above) over its P pages evenly: with q = C / P
 * and r = C % P, page p takes items [p q + min(p, r), (p + 1) q + min(p + 1,
 * r)), so every internal page has at least two children. */
typedef struct shm_bulk_plan_t {
  uint64_t pages;          /* tree pages the load writes (root included, superblock not) */
  uint32_t root_level;     /* 0..7 */
  uint32_t reserved;
  uint64_t level_pages[8]; /* pages of level 0..root_level, 0 above */
} shm_bulk_plan_t;
int shm_bulk_plan(uint64_t n, uint32_t leaf_fill, uint32_t internal_fill,
                  shm_bulk_plan_t *out);
/* Replace the tree's contents with the n pairs (keys[i], vals[i]): DEVICE
 * pointers, keys strictly ascending (unsigned); sorting is the caller's.
 * The tree has the shape of shm_bulk_plan(n, leaf_fill, internal_fill) at
 * fixed places: the root is page 1 (also after a shm_load_image that put it
 * elsewhere); below a root that is not a leaf, level 0 occupies pages 2 ..
 * 2 + P0 - 1 in key order, then level 1, and so on; shm_stats' pages_used ==
 * plan.pages afterwards.  Every page is written whole (lock word 0, versions
 * 1, sibling = the next page of its level, lowest fence = the first key under
 * it, 0 for a level's first page, highest = the next page's lowest, kKeyMax for
 * the last; a leaf's entries in slots 0 .. count - 1 in key order), so nothing
 * of the earlier tree survives in a reused page; the leaf directory and what
 * is built with it are dropped and rebuilt by the next reader.
 * Checked before anything is written, the tree staying exactly as it was:
 * SHM_EINVAL for keys[i] >= keys[i + 1], a key == kKeyMax or a value ==
 * kValueNull (one pass on the device), for a null handle, null keys / vals
 * with n > 0, a leaf_fill / internal_fill out of range, a plan that is too
 * tall, or an outstanding shm_insert_order ticket; SHM_ENOMEM when
 * plan.pages + 1 exceeds the arena's pages.  Rejected arguments return before
 * the handle is used.
 * Exclusive and synchronising, like shm_load_image: it runs after everything
 * queued before it on any stream and returns when the tree is complete.  n is
 * not bounded by cfg.max_batch. */
int shm_bulk_load(shm_tree *t, const uint64_t *keys, const uint64_t *vals,
                  uint64_t n, uint32_t leaf_fill, uint32_t internal_fill,
                  void *stream);
/* Sorted export: every valid pair with lo <= key <= hi in ascending unsigned
 * key order, in parallel passes on the device.  The result is exactly the
 * pairs, and the order, that shm_scan_batch(from = lo, to = hi) with an
 * unbounded limit would return: Tree::range_query's traversal (the leaf
 * holding lo, then the sibling chain; src/Tree.cpp:461-540) and validity rule
 * (value != kValueNull, front == rear entry version in the low nibble); pages
 * the tree does not reach are not read as data.  lo > hi gives 0 pairs and
 * SHM_OK; lo = 0, hi = UINT64_MAX is the whole tree (no stored key equals
 * kKeyMax).
 * keys_out / vals_out: DEVICE pointers; either may be NULL and that array is
 * then not written (a keys-only export feeds splitter sampling).  With both
 * NULL the call only counts and cap is ignored.  n_out: HOST pointer,
 * required; it always receives the number of matching pairs.  That is the
 * number of VALID pairs: shm_check's n_keys also counts torn entries (value
 * != 0, versions unequal), so it may be larger.
 * SHM_ENOSPC: a non-NULL output was given and the count exceeds cap; *n_out
 * is set and nothing is written (the host reads the total before the write
 * pass is launched).  Otherwise the first *n_out words of each given array
 * are written and no word past them is touched.
 * Ordered like shm_range_query_batch: it sees everything queued before it on
 * any stream (e.g. an shm_insert_batch_async), and it is synchronising: it
 * returns when the outputs are complete.  Read-only: the tree, the leaf
 * directory, the bucket table and shm_stats stay as they were.
 * SHM_EINVAL: null handle or null n_out (before the handle is used);
 * SHM_ENOMEM: the workspace (48 B per allocated page, kept on the handle)
 * could not be allocated; SHM_EIO with the scans' error bits: a bad pointer,
 * or a walk past its bound (every chain walk and list is bounded by the
 * allocated pages). */
int shm_export(shm_tree *t, uint64_t lo, uint64_t hi, uint64_t *keys_out,
               uint64_t *vals_out, uint64_t cap, uint64_t *n_out, void *stream);
/* Compaction: rebuild the tree from its own valid pairs.  The whole tree is
 * exported into a temporary device buffer of 16 B per pair and loaded with
 * shm_bulk_load(leaf_fill, internal_fill) (0 / 0: the defaults 36 / 40).
 * Afterwards the tree holds exactly the pairs it held before, in the shape of
 * shm_bulk_plan(n_valid, leaf_fill, internal_fill) at shm_bulk_load's fixed
 * page placement, and pages_used == plan.pages: the pages that deletes and
 * failed splits left behind are free again.  Every consequence of a bulk load
 * applies: entry and page versions restart at 1, the leaf directory and the
 * bucket table are dropped and rebuilt by the next reader.  Exclusive and
 * synchronising.
 * Checked before the first page is written, the tree staying byte for byte as
 * it was: SHM_EINVAL for fills out of range (before the handle is used), a
 * null handle, a plan that is too tall for the counted pairs, or an
 * outstanding shm_insert_order ticket; SHM_ENOMEM when the temporary buffer
 * cannot be allocated or plan.pages + 1 exceeds the arena's pages.
 * shm_bulk_load's own input check still runs on the exported run (about a
 * fifth of a load): a cross-check of the export. */
int shm_compact(shm_tree *t, uint32_t leaf_fill, uint32_t internal_fill, void *stream);
/* Order statistics: where a key stands in the key order, which pair stands at
 * a position, and how many pairs a range holds (offset paging, quantiles,
 * histograms, selectivity before a scan, the splitters of a first load).  No
 * reference counterpart beyond Tree::range_query's traversal and validity
 * rule (src/Tree.cpp:461-540, include/Tree.h:53-54: value != kValueNull, front
 * == rear entry version); a torn entry is not counted.
 *
 *   shm_rank_batch:   ranks_out[i] = the number of valid pairs with key <
 *     keys[i].  It counts exactly what shm_export(0, keys[i] - 1) counts
 *     (0 for keys[i] == 0); for keys[i] == kKeyMax it is the total, since no
 *     stored key equals kKeyMax.
 *   shm_count_batch:  counts_out[i] = the number of valid pairs with from[i]
 *     <= key <= to[i], i.e. rank(to[i] + 1) - rank(from[i]) with to[i] ==
 *     kKeyMax meaning the total; from[i] > to[i] and from[i] == kKeyMax give
 *     0.  It equals shm_range_query's counts on the same ranges, at a cost
 *     that does not grow with the ranges.
 *   shm_select_batch: the pair at position ranks[i] (from 0) of the key
 *     order, i.e. element ranks[i] of shm_export(0, kKeyMax): keys_out[i],
 *     vals_out[i], found_out[i] = 1; for ranks[i] >= the total kKeyMax, 0 and
 *     0.  Each of the three outputs may be NULL, not all three.
 *
 * All pointers are DEVICE pointers; any n (not bounded by cfg.max_batch);
 * n == 0 launches nothing and builds nothing.  The calls answer from an order
 * index kept on the handle: the leaves of the whole tree in key order with the
 * running count of their valid pairs (the whole-tree count pass of shm_export,
 * kept, about 26 B per leaf) and sampled search levels over it, so a query is
 * one search of the index and one leaf read.  Every call that can change the
 * stored pairs or the pages (the inserts, shm_insert_apply, shm_mixed_batch
 * with inserts, shm_del_batch, shm_bulk_load, shm_compact, a rebalance,
 * shm_load_image) makes the index stale as it is issued; the next of these
 * three calls rebuilds it first, and that call is synchronising like
 * shm_export (it sees everything queued before it on any stream).  While the
 * index is valid a call queues one kernel on `stream` and returns without a
 * host wait.  Ordered like shm_scan_batch (exclusive); read-only: the tree,
 * the leaf directory, the bucket table and shm_stats stay as they were.
 * status_dev (device, 2 words, nullable): as shm_scan_batch's, the call ORs
 * its device error bits into status_dev[1] and leaves status_dev[0] alone.
 * SHM_EINVAL: a null handle, a null required array with n > 0 (before the
 * handle is used), or an outstanding shm_insert_order ticket (its chunk is
 * ordered but not applied); SHM_ENOMEM: the index could not be allocated (the
 * handle stays usable); SHM_EIO with the error bits: a bad pointer, a walk
 * past its bound, or an index that does not match the pages. */
int shm_rank_batch(shm_tree *t, const uint64_t *keys, uint64_t n,
                   uint64_t *ranks_out, uint64_t *status_dev, void *stream);
int shm_count_batch(shm_tree *t, const uint64_t *from, const uint64_t *to,
                    uint64_t n, uint64_t *counts_out, uint64_t *status_dev,
                    void *stream);
int shm_select_batch(shm_tree *t, const uint64_t *ranks, uint64_t n,
                     uint64_t *keys_out, uint64_t *vals_out,
                     uint8_t *found_out, uint64_t *status_dev, void *stream);
/* The order index as it stands (host only; it builds nothing): `builds` tells
 * a call that found the index valid from one that rebuilt it. */
typedef struct shm_order_stats_t {
  uint64_t units;         /* leaf units of the last build (0: never built) */
  uint64_t pairs;         /* valid pairs it counted */
  uint64_t bytes;         /* the index's device allocation */
  uint64_t builds;        /* builds so far */
  double last_build_ms;   /* host time of the last build, -1 before the first */
} shm_order_stats_t;
int shm_order_stats(shm_tree *t, shm_order_stats_t *out);
/* Change the key range hint (cfg.key_lo / cfg.key_bits) of a live handle:
 * afterwards the handle behaves as one created with that hint.  The hint
 * steers the get ordering, the leaf directory and the bucket table only; keys
 * outside it are still stored and found exactly.  It is what makes a tree of
 * narrow keys fast: with key_bits = 64 and every key below 2^26 all keys share
 * directory entry 0 and every get starts at the root.  key_bits == 0 is read
 * as 64, and key_bits == 64 forces key_lo = 0, as at create.
 * Exclusive and synchronising, ordered like shm_bulk_load: it runs after
 * everything queued before it on any stream.  It drops exactly what
 * shm_bulk_load drops -- the leaf directory, its level hints, the LDS replica's
 * table and the bucket table -- and the next reader rebuilds them over the new
 * range; the tree's pages are not touched.
 * SHM_EINVAL: key_bits > 64 or a null handle (before the handle is used), or
 * an outstanding shm_insert_order ticket (its chunk was ordered by the old
 * range). */
int shm_tree_set_key_range(shm_tree *t, uint64_t key_lo, uint32_t key_bits);
/* Structural check on device data: fences, ordering, occupancy. */
int shm_check(shm_tree *t, uint64_t *n_leaves, uint64_t *n_internal,
              uint64_t *n_keys);
int shm_synchronize(shm_tree *t);
/* The device error block as the last synchronising call that found bits in
 * it read it (reset = 1 clears this record).  Errors of asynchronous calls
 * surface at the next synchronising call, whichever it is: `chunk` names the
 * insert chunk that first saw them, so a caller that noted shm_last_chunk()
 * after each async insert knows which batch failed (the reference asserts at
 * the failing operation instead, src/Tree.cpp:220-227, 332-337). */
typedef struct shm_error_t {
  uint32_t bits;     /* device error bits (0 = none was read) */
  uint32_t chunk;    /* insert chunk that first saw them (0: none, e.g. a
                        search's walk bound) */
  int32_t status;    /* the status that call returned */
  uint32_t resumed;  /* chunks whose split propagation gave up waiting and
                        was completed by the launch's last block alone
                        (cumulative) */
} shm_error_t;
int shm_last_error(shm_tree *t, shm_error_t *out, int reset);
/* id of the last insert chunk queued on the handle (1, 2, ...; a batch of n
 * ops is ceil(n / max_batch) chunks).  The id is also the tag the device
 * state is stamped with, 32 bits wide: the chunk after id 2^32 - 1 gets id 1
 * again, never 0.  Before it is issued the handle is drained (a device
 * synchronisation inside that insert call) and every word that carries a
 * chunk tag is cleared, so ids of the two epochs are never compared on the
 * device.  shm_last_chunk and shm_error_t.chunk count within the epoch: a
 * caller that pairs them must read both on the same side of the restart (the
 * restart is visible as shm_last_chunk going down); an error bit set before
 * the restart and read after it names its chunk by the old epoch's id.  The
 * contents, statuses and error bits of every chunk are unaffected. */
uint32_t shm_last_chunk(shm_tree *t);
/* Copy `bytes` (a multiple of 4, <= 1024) of device memory at `src` to
 * host_out once the work queued on `stream` before it has produced them,
 * through the library's zero-copy read-back (one-wave kernel into mapped
 * host memory + a spin on a sequence word) instead of a D2H copy and a stream
 * synchronisation.  Used by the shard router for the RCCL split sizes. */
int shm_read_words(shm_tree *t, const void *src, uint64_t bytes, void *host_out,
                   void *stream);

/* per-kernel timing with HIP events recorded on the launch stream around the
 * hot path's phases (get: order = top-bits sort, walk = the page walk kernel;
 * insert: the whole chunk and its in-place leaf upsert kernel; range: each
 * shm_range_query launch).  Enabled handles pay one event record per phase
 * boundary per call. */
typedef struct shm_profile_t {
  uint64_t calls;        /* search_batch calls (chunks) timed */
  uint64_t queries;      /* queries in those calls */
  double order_ms;       /* sum of get-ordering (partition) time */
  double walk_ms;        /* sum of k_get (page walk) kernel time */
  uint64_t insert_calls; /* insert_batch chunks timed */
  uint64_t insert_ops;   /* ops in those chunks (before dedup) */
  double insert_ms;      /* sum of whole-chunk insert time */
  double upsert_ms;      /* sum of k_leaf_upsert kernel time */
  uint64_t range_calls;  /* shm_range_query launches timed (count + fill) */
  uint64_t range_queries;/* scans in those launches */
  double range_ms;       /* sum of k_range kernel time */
  /* the timed insert chunks' work, counted on the device (ABI 9): the
   * per-touched-leaf algorithmic bytes of bench.py's insert roofline */
  uint64_t insert_unique;/* unique upserts after the batch's last-writer fold */
  uint64_t insert_dels;  /* unique deletes */
  uint64_t insert_staged;/* staged segments: leaves read whole (they get a new key) */
  double walk_kernel_ms; /* sum of the summary walk's device-clock spans (first block
                            start to last wave end: the kernel alone, no launch gap) */
} shm_profile_t;
/* on: bit 0 = the event timing above, bit 1 = the index statistics below */
int shm_profile_enable(shm_tree *t, int on);
int shm_profile_read(shm_tree *t, shm_profile_t *out, int reset);

/* Index statistics of the batched get walk (the role of the reference's
 * Tree::index_cache_statistics / clear_statistics, include/Tree.h:62-63:
 * how often the index cache — here the leaf directory or the LDS replica —
 * took a get straight to its leaf), collected while shm_profile_enable bit
 * 1 is on. */
typedef struct shm_index_stats_t {
  uint64_t gets;            /* queries walked */
  uint64_t start_internal;  /* start page without a leaf summary: a directory
                               miss, or a descent (no directory) */
  uint64_t right_moves;     /* B-link right turns (a stale directory entry) */
  uint64_t page_hops;       /* pages walked from their own bytes */
  uint64_t entry_reads;     /* leaf entries read (fingerprint matches) */
  uint64_t hits;            /* queries found */
  uint64_t dir_fp_hits;     /* found from the directory entry alone (no
                               summary line): its copy of the leaf's
                               fingerprints, or its pair form's slots */
} shm_index_stats_t;
int shm_index_stats(shm_tree *t, shm_index_stats_t *out, int reset);

/* The leaf directory the batched get starts from (the role of the
 * reference's IndexCache, include/IndexCache.h:59-259, whose size and hit
 * counts Tree::index_cache_statistics reports, include/Tree.h:62): its form,
 * the device memory it holds and what its rebuilds cost.  Synchronises with
 * the last rebuild's end (not with other work). */
typedef struct shm_dir_stats_t {
  uint32_t form;              /* 0 none, 1 leaf lists + fingerprints, 2 pair form */
  uint32_t bits;              /* log2 of the entries of the current build */
  uint64_t entries;           /* 2^bits entries of 64 B */
  uint64_t bytes;             /* device bytes held: the allocation (never shrunk)
                                 + the level hints */
  uint64_t builds;            /* builds so far */
  uint64_t pages_at_build;    /* tree pages at the last build */
  uint64_t pages_since_build; /* pages splits added since */
  double last_build_ms;       /* device time of the last build (-1: none yet) */
  double total_build_ms;      /* of every build */
  uint32_t maintained;        /* 1: insert chunks may keep the entries current */
  uint32_t exact;             /* 1: every usable entry equals a fresh build's */
} shm_dir_stats_t;
int shm_dir_stats(shm_tree *t, shm_dir_stats_t *out);

/* multi-GPU routing helpers (range shards: shard s owns
 * [s * 2^64 / P, (s+1) * 2^64 / P), or the range between two splitters:
 * shm_route_bucket_bounds) ---------------------------------------------------- */
/* Bucket n <= max_batch keys by owning shard (1 <= P <= 64): writes
 * per-shard counts[P], the keys grouped by shard into keys_out, and perm[i] =
 * source position of keys_out[i].  Stable: inside a shard, keys keep their
 * input order (routed insert batches keep last-writer-in-batch-order). */
int shm_route_bucket(shm_tree *t, const uint64_t *keys, uint64_t n,
                     uint32_t num_shards, uint64_t *counts_out,
                     uint64_t *keys_out, uint32_t *perm_out, void *stream);
/* shm_route_bucket for shards cut at arbitrary boundaries.  splitters_host:
 * HOST pointer to num_shards - 1 words, ascending (unsigned, not strictly);
 * shard p owns [splitters[p - 1], splitters[p]), shard 0 from key 0 and the
 * last shard up to 2^64, so a key's owner is the number of splitters <= it.
 * A repeated splitter x makes an empty shard [x, x), and a key equal to x
 * goes to the highest shard that starts at x.  The words are read during the
 * call (they travel in the kernel arguments), not afterwards.  Counts, order
 * inside a shard and perm as shm_route_bucket.  splitters_host == NULL behaves
 * as shm_route_bucket, bit for bit (the same kernels).  SHM_EINVAL: a splitter
 * below its predecessor, or one equal to kKeyMax (no key may be stored there),
 * checked before the handle is used. */
int shm_route_bucket_bounds(shm_tree *t, const uint64_t *keys, uint64_t n,
                            uint32_t num_shards, const uint64_t *splitters_host,
                            uint64_t *counts_out, uint64_t *keys_out,
                            uint32_t *perm_out, void *stream);
/* out[i] = in[perm[i]] (carry a companion array, e.g. insert values, along
 * with the bucketed keys). */
int shm_route_permute(shm_tree *t, const uint64_t *in, const uint32_t *perm,
                      uint64_t n, uint64_t *out, void *stream);
/* out[perm[i]] = in[i] (reverse of the bucket permutation). */
int shm_route_unpermute(shm_tree *t, const uint64_t *in, const uint32_t *perm,
                        uint64_t n, uint64_t *out, void *stream);
/* the same for routed get replies, with found_out[perm[i]] = in[i] != 0
 * (Tree::search's bool, Tree.cpp:445-448) in the same pass */
int shm_route_unpermute_found(shm_tree *t, const uint64_t *in, const uint32_t *perm,
                              uint64_t n, uint64_t *out, uint8_t *found_out, void *stream);

/* multi-GPU range shards over RCCL ------------------------------------------
 * Rank r of P (P <= 16) owns keys [r * 2^64 / P, (r+1) * 2^64 / P) in its own
 * shm_tree (create it with key_lo / key_bits of that slice), until splitters
 * are set (shm_shard_set_splitters, shm_shard_rebalance below).  One process per
 * GPU; every rank makes the same calls in the same order (collectives).
 * Every rank's tree has the same max_batch (checked at create).
 * A routed get: each key into its owner's run of fixed-size slots
 * (n / P + 6 sqrt(n / P) + 256 keys; the runs' tails padded with kKeyMax
 * once per size, later batches leaving earlier keys of the same owner
 * there), grouped ncclSend / ncclRecv of the runs and of the per-peer
 * counts, local shm_search_batch, results back the same way, gathered to
 * input order; no host wait before the key exchange.  Every rank passes the
 * same n: the slots' size derives from it, and ranks that disagree exchange
 * runs of different sizes.  Keys past their run's slot are answered by an
 * exact second round that end() runs after one read-back of the counts: no
 * lookup is dropped.  A routed insert: stable bucketing, each owner's run
 * in a slot of max_batch / P (kKeyMax padding the receiver skips; a batch
 * holding kKeyMax itself routes nothing and is reported as SHM_EINVAL by the
 * next synchronising call), keys / values / counts exchanged, queued as one
 * insert on the owner with no host wait.  Each rank's ops apply in its own
 * batch order; across ranks the slots apply in rank order, and a run's tail
 * past its slot is sent and applied by the next call on the shard (or
 * shm_shard_synchronize) before anything else, after every rank's slots: one
 * valid linearisation of the ranks' concurrent batches.  Device pointers;
 * n <= the local tree's max_batch. */
typedef struct shm_shard shm_shard;
/* rank 0 makes the id (NCCL_UNIQUE_ID_BYTES = 128), the caller broadcasts it */
int shm_nccl_unique_id(void *id_out, uint64_t bytes);
int shm_shard_create(shm_tree *local, const void *nccl_id, uint64_t id_bytes, uint32_t world,
                     uint32_t rank, shm_shard **out);
/* the same over a caller's communicator (an ncclComm_t as void*; not freed) */
int shm_shard_create_with_comm(shm_tree *local, void *nccl_comm, uint32_t world, uint32_t rank,
                               shm_shard **out);
int shm_shard_destroy(shm_shard *s);
/* vals_out / found_out in input order (Tree::search per key) */
int shm_shard_search(shm_shard *s, const uint64_t *keys, uint64_t n, uint64_t *vals_out,
                     uint8_t *found_out, void *stream);
/* the same in two halves for pipelining: begin = bucketing + the keys'
 * exchange, end = local get + the results' exchange + unpack (neither waits
 * for the device).  Two batches may be begun at once (two slots, each with
 * its own communicator); end them in order.  At world 1 begin does nothing
 * and end is the local get over keys[], so keys[] stays unchanged until
 * end's work has run on the stream. */
int shm_shard_search_begin(shm_shard *s, const uint64_t *keys, uint64_t n, void *stream,
                           uint32_t *ticket);
int shm_shard_search_end(shm_shard *s, uint32_t ticket, uint64_t *vals_out, uint8_t *found_out);
int shm_shard_insert(shm_shard *s, const uint64_t *keys, const uint64_t *vals, uint64_t n,
                     void *stream);
/* Tree::range_query over the shards (src/Tree.cpp:461-540, intended
 * semantics): scan i = [from[i], to[i]] inclusive; its pieces go only to the
 * shards it overlaps (row p of a P x n_cap piece matrix to rank p), the
 * owners scan them, counts come back, and ONE host read-back of the
 * per-peer value totals sizes the value exchange.  counts_out[i], offsets_out
 * (exclusive scan) and *total_out are always produced; values in key order
 * across shards go to vals_out when total <= vals_cap, else SHM_ENOSPC
 * (counts and offsets stay valid, and shm_shard_range_values copies the
 * batch's values into a larger buffer without another exchange).  n_cap:
 * the same on every rank, >= n, P * n_cap <= max_batch. */
int shm_shard_range_query(shm_shard *s, const uint64_t *from, const uint64_t *to, uint64_t n,
                          uint64_t n_cap, uint64_t *counts_out, uint64_t *offsets_out,
                          uint64_t *vals_out, uint64_t vals_cap, uint64_t *total_out,
                          void *stream);
/* The same batch with no host synchronisation: the values
 * travel in fixed runs of peer_cap values per peer each way (the same on
 * every rank), padded on the device, so nothing is read back to size the
 * exchange.  counts_out / offsets_out as above; status (2 device words,
 * written on the stream): status[0] = the batch's total values, status[1] =
 * flags -- 1: a run to or from a peer passed peer_cap (values lost), 2: the
 * scan pass's buffer was short, 4: total > vals_cap (values past vals_cap
 * dropped), 8: a device error of the scans.  Nonzero flags: the batch's
 * values are incomplete; repeat it with shm_shard_range_query (before any
 * tree change).  Sizing: peer_cap ~ 1.25 x the values a rank's scans find
 * on one shard, + a few thousand. */
int shm_shard_range_query_async(shm_shard *s, const uint64_t *from, const uint64_t *to,
                                uint64_t n, uint64_t n_cap, uint64_t *counts_out,
                                uint64_t *offsets_out, uint64_t *vals_out, uint64_t vals_cap,
                                uint64_t peer_cap, uint64_t *status, void *stream);
/* the last shm_shard_range_query batch's values (its offsets_out must still
 * be live), local only: valid until the next call on the shard */
int shm_shard_range_values(shm_shard *s, uint64_t *vals_out, uint64_t vals_cap, void *stream);
/* Apply what a routed insert left for the next call (its overflow tails),
 * then shm_synchronize the local tree: the status of every routed batch. */
int shm_shard_synchronize(shm_shard *s);

/* Shards that follow the stored keys -----------------------------------------
 * A shard handle starts with P equal slices of 2^64.  With splitters set,
 * shard p owns [b[p], b[p + 1]) with b[0] = 0, b[P] = 2^64 and b[1 .. P - 1]
 * the splitters, ascending and not strictly: a repeated splitter makes an
 * empty shard, and a key's owner is the number of splitters <= it (as
 * shm_route_bucket_bounds).  Routed gets, inserts, their overflow rounds and
 * range scans all cut at the same boundaries; a shard with no splitters set
 * runs the kernels it ran before they existed. */
/* splitters_host: HOST pointer to P - 1 words; NULL = back to equal slices.
 * A collective by convention: every rank passes the same words, checked with
 * one exchange (as max_batch is at create); ranks that differ get SHM_EINVAL
 * and keep their bounds.  Pending routed-insert tails are applied first (by
 * the old bounds).  It MOVES NO DATA: pairs stored under the old bounds stay
 * where they are, and a key whose owner changed is no longer found by routed
 * calls until shm_shard_rebalance (or the caller) has moved it -- a caller who
 * sets splitters over non-empty trees owns the consequences.  Meant for empty
 * trees, e.g. a caller that sampled its first batch itself.  The local trees'
 * key range hints are not changed (shm_tree_set_key_range).
 * SHM_EINVAL: a null handle, descending splitters or one equal to kKeyMax,
 * a shm_shard_search_begin ticket still outstanding, or ranks that disagree. */
int shm_shard_set_splitters(shm_shard *s, const uint64_t *splitters_host);
/* the current boundaries b[1 .. P - 1] (the equal slices' when none are set)
 * into out_host (HOST, P - 1 words; may be NULL at P = 1); local, no exchange */
int shm_shard_get_splitters(shm_shard *s, uint64_t *out_host);
/* The even re-cut of P shards holding counts[p] pairs, by host arithmetic
 * alone (no handle, no GPU, like shm_bulk_plan).  Shards are range-ordered,
 * so the global sorted order is the shards' sorted contents in rank order:
 * with N = sum(counts) and off[] its exclusive scan, old shard r holds global
 * positions [off[r], off[r] + counts[r]).  New shard p holds [cut[p],
 * cut[p + 1]) with cut[p] = floor(p N / P) (cut[P] = N), so new counts differ
 * by at most 1.  send_cnt[p] = pairs `rank` sends to p (the overlap of its old
 * positions with p's new ones), recv_cnt[p] = pairs it receives from p (the
 * overlap of p's old positions with its new ones); a rank's own part is in
 * both.  cut: P + 1 words, send_cnt / recv_cnt: P words each, all HOST.
 * SHM_EINVAL: P = 0, P > 16, rank >= P or a null pointer. */
int shm_rebalance_plan(const uint64_t *counts, uint32_t P, uint32_t rank,
                       uint64_t *cut, uint64_t *send_cnt, uint64_t *recv_cnt);
/* Rebalance: re-cut the stored pairs evenly over the shards and move them.
 * Collective (every rank calls it with the same fills), exclusive and
 * synchronising.  Per rank: pending routed-insert tails are applied; the
 * whole local tree is exported in key order (shm_export's passes, as
 * shm_compact) into a temporary device buffer of 16 B per pair; the ranks
 * exchange their counts and each runs shm_rebalance_plan; new splitter j is
 * the key at global position cut[j], contributed by the rank whose export
 * holds it -- exact quantiles, no sampling and no global sort; each
 * destination's contiguous run of the export (keys, then values) goes to it
 * point to point, received in source-rank order, so the received run is
 * already strictly ascending; the local tree's key range hint is set from the
 * run (key_lo = its first key, key_bits = max(1, ceil(log2(last - first +
 * 1))); a run of fewer than two pairs leaves the hint alone); the run is
 * loaded with shm_bulk_load(leaf_fill, internal_fill) (0 / 0: 36 / 40), whose
 * own input check runs on it as a cross-check; then the new bounds are
 * installed.  *n_local_out (HOST, required) = this rank's new pair count.
 * Afterwards every pair is where routed calls look for it, the counts differ
 * by at most 1 across ranks, shm_stats' pages_used == shm_bulk_plan(n_local)
 * .pages on every rank, and every consequence of a bulk load applies.  When
 * fewer than P pairs are stored several cuts coincide: repeated splitters,
 * empty shards.  When nothing is stored the bounds and the trees stay as they
 * are.  At world 1 the call is a compaction.
 * Temporary device memory per rank: 16 B x its old pairs + 16 B x its new
 * pairs; the tree is rewritten in place.
 * Checked by every rank before any tree is written, and agreed with one
 * exchange: the fills, an outstanding shm_insert_order ticket on the local
 * tree (SHM_EINVAL), shm_bulk_plan(n_new).pages + 1 against the arena's pages
 * and the two temporary buffers (SHM_ENOMEM).  If any rank fails, every rank
 * returns the status of the lowest such rank, and every tree, the bounds and
 * the directories stay exactly as they were.  SHM_EINVAL without an exchange:
 * a null handle or n_local_out, or a shm_shard_search_begin ticket still
 * outstanding (every rank has it or none: collectives). */
int shm_shard_rebalance(shm_shard *s, uint32_t leaf_fill, uint32_t internal_fill,
                        uint64_t *n_local_out, void *stream);

/* Tree::lock_bench (include/Tree.h:60, src/Tree.cpp:310-321) for a batch:
 * take and release lock[CityHash64(keys[i]) % num_locks] of the HBM lock
 * table (atomicCAS, try_lock_addr / unlock_addr, Tree.cpp:205-264); keys
 * sharing a word take it in turn.  Ordered like an insert; a spin past its
 * bound is reported at the next synchronising call. */
int shm_lock_bench(shm_tree *t, const uint64_t *keys, uint64_t n, void *stream);

/* workload generators on device (test/benchmark.cpp:43-46, zipf.h) ----------- */
/* keys[j] = CityHash64(i) + 1 (mod keyspace if keyspace != 0), i = first + j */
int shm_gen_keys(shm_tree *t, uint64_t first, uint64_t n, uint64_t keyspace,
                 uint64_t *keys_out, void *stream);
/* keys[j] = CityHash64(ids[j]) + 1 (mod keyspace if keyspace != 0): to_key
 * over an id array, e.g. a zipf stream (test/benchmark.cpp:43-46, 172-173) */
int shm_hash_keys(shm_tree *t, const uint64_t *ids, uint64_t n, uint64_t keyspace,
                  uint64_t *keys_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SHERMAN_AMD_H */
