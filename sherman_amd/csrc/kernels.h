// kernels.h — launch interface between the host runtime (tree*.cpp,
// shard*.cpp) and the HIP kernels (get.hip, get_sum.hip, get_side.hip,
// locate.hip, isort.hip, partition.hip, upsert.hip, insert.hip, leafdir.hip,
// tile_scan.hip, route.hip, range.hip, scan.hip, bulk.hip, export.hip,
// order.hip, service.hip).  Each section below names the unit that defines what it
// declares.  Host-only types; no torch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.h"

namespace shm {
namespace dev {

// ---- gets, locate, leaf directory (get.hip, get_sum.hip, get_side.hip,
// locate.hip, leafdir.hip) ---------------------------------------------------
// the key-value bucket table's format (valtab.h): 8 slots of (key, value) per
// 128 B bucket; the build's counter words
constexpr int kVtSlots = 8;
constexpr int kVtBucketWords = 2 * kVtSlots;  // u64 words: 128 B
constexpr int kVtCtrWords = 4;

struct WalkArgs {
  const uint8_t* arena;
  uint64_t arena_bytes;
  uint16_t node;
  uint64_t root;
  const uint64_t* keys;
  const uint32_t* perm;   // output position of walk query i (nullable)
  const uint64_t* n_dev;  // device count (nullable -> use n)
  uint64_t n;
  uint64_t* out_val;      // GET
  uint8_t* out_found;     // GET (nullable)
  uint64_t* out_page;     // LOCATE
  int target_level;       // LOCATE
  uint32_t* err;
  // leaf directory (leafdir.hip; nullable -> start at the root): 8 u32 per
  // entry, entry p covers keys [dir_lo + (p << dir_shift), ... + 2^dir_shift)
  const uint64_t* dir;
  uint64_t dir_lo;
  uint64_t dir_n;
  uint32_t dir_shift;
  // GET: map blocks to chunks XCD-contiguously (see get.hip)
  int xcd_remap;
  // LOCATE: the directory is in pair form (layout.h kDirPairs): the
  // pair-aware kernel (the fingerprint form's kernel stays as it was)
  int dir_pairs;
  // the directory is exact (built, then kept by every insert chunk since:
  // dir_upkeep.h): a usable entry's fingerprints / pairs name every key of
  // its prefix, so a key they do not lead to is absent, and its leaf is the
  // entry's (LOCATE: a new key needs no summary walk)
  int dir_exact;
  // GET (k_get_sum): the page-level version check on every hit
  // (SHM_FLAG_PAGE_CHECK)
  int page_check;
  // GET: page DMAs with the non-temporal policy (nt; streamed once per batch)
  int nt;
  // GET: per-page occupancy bound (nullable -> whole pages are read).  For a
  // leaf, every slot >= leaf_hw[page] is empty (value 0), so its page DMA
  // stops after that slot; kLeafHwFull (internal pages, pages of a loaded
  // image) reads the whole page
  const uint8_t* leaf_hw;
  // leaf summaries (layout.h kSumBytes per page; k_get_sum, LOCATE)
  const uint8_t* sum;
  // LOCATE at level 0 (nullable): an op whose key its leaf holds overwrites
  // that entry in place (vals[i], under the page's lock word taken with
  // lock_tag) and records out_slot[i] = bit 31 | slot; any other op gets 0
  // and marks its leaf out_new[page] = out_new_tag (staged whole by the upsert)
  uint32_t* out_slot;
  uint8_t* out_new;      // byte marks: new_mark(out_new_tag)
  uint32_t out_new_tag;
  // nullable: set to out_new_tag when any op marked a page (a wave stores
  // it once): the segmentation skips a chunk of updates only
  uint32_t* any_new;
  const uint64_t* vals;
  uint64_t* locks;
  uint32_t num_locks;
  uint64_t lock_tag;
  // GET (k_get_sum), nullable: the top of the tree replicated in LDS (the
  // fences and page indices of every page of one upper level, launch_top):
  // with no directory, each lane starts at the level page holding its key
  const uint64_t* top_keys;
  const uint32_t* top_pages;
  uint32_t top_n;
  // GET (k_get_sum), nullable: index statistics (kIdxStats words, added per
  // wave): see IdxStat
  uint64_t* stats;
  // GET (k_get_sum), nullable (profiling): the launch's device wall clock,
  // clk[b] = block b's start, clk[gridDim.x + w] = wave w's end (after its
  // result stores are issued); the host takes last end - first start
  uint64_t* clk;
  // GET (k_get_sum without page_check), nullable: the key-value bucket table
  // (valtab.h), read before the directory: vt_n buckets of 16 u64, bucket b
  // covers keys [vt_lo + (b << vt_shift), ... + 2^vt_shift).  Set only while
  // the table is trusted (tree.cpp vt_trusted); never in LOCATE or the scans
  const uint64_t* vt;
  uint64_t vt_lo;
  uint64_t vt_n;
  uint32_t vt_shift;
  // GET with a table: the probe loads each bucket line with one instruction
  // (SHM_GET_COOP), and the gets the table does not answer are packed into
  // the block's lowest waves (SHM_GET_PACK); 0 = the form before each (A/B,
  // tests).  launch_get_sum picks the instantiation
  int get_coop;
  int get_pack;
};
// k_get_sum's index statistics (shm_index_stats)
enum IdxStat {
  kIdxGets = 0,        // queries walked
  kIdxStartInternal,   // start page without a leaf summary (directory miss / descent)
  kIdxRightMoves,      // B-link right turns
  kIdxPageHops,        // pages walked from their own bytes (internal or unsummarised)
  kIdxEntryReads,      // leaf entries read (fingerprint matches)
  kIdxHits,            // queries found
  kIdxDirFp,           // found through the directory entry's fingerprints
  kIdxStats
};
// top-of-tree table for k_get_sum's LDS replica (get_side.hip: what the gets
// read beside the pages, rebuilt from the pages): every page of the deepest level
// whose page count fits max_n, in key order: keys[i] = its lowest fence,
// pages[i] = its page index; *n_out = the count, *level_out its level
void launch_top(const uint8_t* arena, uint64_t arena_bytes, uint16_t node, uint64_t root,
                uint32_t max_n, uint64_t* keys, uint32_t* pages, uint64_t* scratch,
                uint32_t* n_out, uint32_t* err, hipStream_t s);
constexpr uint32_t kTopMax = 4096;  // 48 KB of LDS per block

// batched get walk with grouped page resolution (get.hip)
void launch_get(const WalkArgs& a, uint64_t n, hipStream_t s);
// k_get_sum's block size, and its blocks for n queries (the profile's clock
// words: one per block + one per wave, WalkArgs.clk)
constexpr int kGetSumTPB = 256;
uint64_t get_sum_blocks(uint64_t n);
// batched get over the leaf summaries, lane = query (get_sum.hip): directory
// entry, summary line, matching entries; results in input order
void launch_get_sum(const WalkArgs& a, uint64_t n, hipStream_t s, hipEvent_t ev0 = nullptr,
                    hipEvent_t ev1 = nullptr);
// rebuild the summaries of pages [1, pages) from the page bytes (a loaded
// image; get_side.hip), one wave per page; leaf[p] != 0 (device bytes, one per page) names
// the leaves the image reaches from its root: only those get a line
void launch_sum_rebuild(const uint8_t* arena, uint64_t pages, const uint8_t* leaf, uint8_t* sum,
                        hipStream_t s);
// header-only descent, lane = op (locate.hip): out_page[i] = the page of
// a.target_level holding keys[i]; starts at the leaf directory for level 0
void launch_locate(const WalkArgs& a, uint64_t n_upper, hipStream_t s);
// leaf directory (leafdir.hip): n_ent entries of 8 u32 from dir_lo, 2^shift
// keys each
// hint (nullable): 2 x n_ent u32, the level-1 and level-2 pages (page
// indices, 0 = none) on the root-to-leaf path of each prefix's first key
// from_hint: start each prefix at the level-1 page the previous build
// recorded in hint (same entry count, same tree) instead of the root
// sum (nullable): the leaf summaries; an entry whose prefix lies inside one
// leaf then carries that leaf's fingerprints (layout.h kDirFp)
// pairs: build the pair form (layout.h kDirPairs) instead of the
// fingerprint form: the leaf lists here, then the pairs by launch_dir_pairs
void launch_leaf_dir(const uint8_t* arena, uint64_t arena_bytes, uint16_t node, uint64_t root,
                     uint64_t dir_lo, uint32_t shift, uint64_t n_ent, uint64_t* dir,
                     uint32_t* hint, int from_hint, const uint8_t* sum, uint32_t* err,
                     hipStream_t s, int pairs = 0);
// the pairs of a pair-form directory: one wave per page of [1, n_pages)
// whose summary line (sum) carries the leaf tag: the tree's current leaves
void launch_dir_pairs(const uint8_t* arena, const uint8_t* sum, uint64_t n_pages, uint16_t node,
                      uint64_t dir_lo, uint32_t shift, uint64_t n_ent, uint64_t* dir,
                      hipStream_t s);
// the value form after the pairs (layout.h kDirVals): one thread per entry
void launch_dir_vals(const uint8_t* arena, uint64_t n_pages, uint64_t n_ent, uint64_t* dir,
                     hipStream_t s);
// the key-value bucket table (valtab.h) from the leaves, after a zero fill:
// one wave per page of [1, n_pages) whose summary line (sum) carries the leaf
// tag; ctr (zeroed by the caller) = {dead buckets, stored keys that ended in
// dead buckets, stored keys}
void launch_vt_build(const uint8_t* arena, const uint8_t* sum, uint64_t n_pages, uint64_t lo,
                     uint32_t shift, uint64_t n_buckets, uint64_t* vt, uint64_t* ctr,
                     hipStream_t s);
// rebuild the entries an insert chunk listed (fix[0 .. fix_n[par]), at most
// cap) from the tree, in form `form` (kDirForm*); zeroes fix_n[par ^ 1]; the
// repairs past cap are added to *lost (host memory, nullable)
void launch_dir_repair(const uint8_t* arena, uint64_t arena_bytes, uint16_t node, uint64_t root,
                       uint64_t dir_lo, uint32_t shift, uint64_t n_ent, uint64_t* dir,
                       const uint32_t* hint, int form, const uint32_t* fix, uint32_t* fix_n,
                       uint32_t par, uint32_t cap, uint64_t* lost, uint32_t* err, hipStream_t s,
                       int vals = 0, uint64_t applied = 0);
struct UpperArgs;
// per-op word of the upsert (SegArgs.placed): the op's new key went into an
// empty slot of its leaf, the slot in the low 6 bits
constexpr uint32_t kOpPlaced = 0x40000000u;
// the chunk's directory upkeep after its k_upper (k_dir_upkeep): the placed
// new keys (ops: pages = k_locate's leaf per op, n_ops_dev their count) and
// the split segments; n_max bounds both counts (the grid)
void launch_dir_upkeep(const UpperArgs& u, const uint32_t* oslot, const uint64_t* pages,
                       const uint64_t* n_ops_dev, uint64_t n_max, hipStream_t s);
// diagnostics: the trusted entries against the tree (k_dir_verify): out =
// kDirVerifyWords words, zeroed by the caller
constexpr int kDirVerifyWords = 10;
void launch_dir_verify(const uint8_t* arena, uint64_t arena_bytes, uint16_t node, uint64_t root,
                       uint64_t dir_lo, uint32_t shift, uint64_t n_ent, const uint64_t* dir,
                       const uint32_t* hint, unsigned long long* out, hipStream_t s);

// ---- insert pipeline (upsert.hip, insert.hip) ---------------------------------
// k_upper runs one block per CU (at most kMaxUpper); its control block.
constexpr int kMaxUpper = 512;
// k_upper's phases (insert.hip): tickets / completion counts per phase.
// 0 = sibling pages of large leaf splits, 1 = leaf splits (dn[.][0] counts
// both), 1 + L = internal level L (L = 1 .. kMaxLevelOfTree)
constexpr int kUpPhases = 16;
constexpr int kLbBin = 0, kLbSeg = 1, kLbScan = 2;
struct UpperCtl {
  // Phase hand-offs (insert.hip handoff), each word on a 128 B line of its
  // own: tk = the next unclaimed task of a phase (tickets, taken in dispatch
  // order by running waves / blocks), dn = its finished tasks, abort = a
  // hand-off gave up (every block leaves at its next hand-off; the launch's
  // last block completes the chunk alone).  Double buffered by chunk parity:
  // a launch uses set par and zeroes set par ^ 1 for the next one.
  uint32_t tk[2][kUpPhases][32];
  uint32_t dn[2][kUpPhases][32];
  uint32_t abort[2][32];
  uint32_t gate;    // tag of the last chunk rejected by its ordering (kKeyMax)
  // block-index counters of the look-back kernels (lookback_index,
  // device_common.h), one 128 B line each: kLbBin k_bin_unique, kLbSeg
  // k_seg_fill(_slot), kLbScan k_scan_u64
  uint32_t lb_ids[3][32];
  // leaf split counts of the upsert kernel per k_upper block range, double
  // buffered by chunk parity (k_upper zeroes the other parity)
  uint32_t leaf_np[2][kMaxUpper];  // new pages
  uint32_t leaf_ns[2][kMaxUpper];  // split segments
  uint32_t leaf_nb[2][kMaxUpper];  // new pages of splits into more than kSmallSplit pages
  // internal levels (k_upper): pages allocated past the leaf level's, pages
  // made, the root's level after growth, separators emitted for each level
  // (all per parity, zeroed by the previous launch)
  uint64_t alloc[2][16];
  uint64_t made[2][16];
  uint32_t root_new[2][32];
  uint32_t lvl_sep[2][16];
  uint32_t done[2][32];  // blocks finished: the last one writes the superblock
  // pages the upsert kernel's early splits took (leaf and internal), from the
  // superblock's next_page on; k_upper's own pages follow them
  uint64_t ualloc[2][16];
  // set (plain stores) by the upsert kernel when it leaves a split to k_upper:
  // unset, a chunk without deletes needs only k_upper's block 0
  uint32_t late[2][32];
  // the tag of a chunk the segmentation kernel completed (no new key, no
  // delete: upper_quick.h); its k_upper returns at once
  uint64_t skip[2][16];
  // the chunk's delete count, copied from the ordering's counts by the
  // segmentation kernel's block 0 (k_seg_fill), which runs before anything
  // publishes the op buffers free; k_upper reads this copy, so no block of
  // it reads the ordering's count, which chunk tag + 2's ordering may rewrite
  // once the buffers are published
  uint64_t ndel[2][16];
};
// UpperArgs.pub word 4: the tag of the last chunk whose k_upper is done with
// the chunk's op buffers (tree.cpp insert_order's flow control)
constexpr int kPubApplied = 4;
// UpperArgs.pub word 6: directory repairs lost so far (k_dir_repair, cumulative)
constexpr int kPubDirLost = 6;
// words 7 / 8: the directory upkeep's work so far (new keys + split pages,
// cumulative) and the count of chunks whose upkeep finished (k_dir_repair
// publishes both from the device counters at dir_fix_n + kDirWorkWord)
constexpr int kPubDirWork = 7;
constexpr int kPubDirUpkeeps = 8;
constexpr int kDirWorkWord = 2;
// a leaf split into at most this many pages is built by one wave (pages
// 1.. first, page 0 last, no fan-in); larger ones are spread over the grid
constexpr uint32_t kSmallSplit = 4;

// a chunk's byte mark in the per-page new-key array (tree.cpp pnew): 1..255,
// repeating every 255 chunks (the host clears the array when it wraps).  One
// byte per page keeps the array L2-sized (1.9 MB at C2's 1.9 M pages), so the
// segmentation's per-run lookups hit L2
__host__ __device__ __forceinline__ uint8_t new_mark(uint32_t tag) {
  return (uint8_t)(tag % 255u + 1u);
}

// in-place leaf upserts (upsert.hip)
struct SegArgs {
  uint8_t* arena;
  uint64_t arena_bytes;
  uint16_t node;
  // sorted unique operation keys / values
  const uint64_t* op_key;
  const uint64_t* op_val;
  // staged segments (runs of ops targeting one page that gets a new key,
  // launch_segment): ops [seg_start, seg_end) of page seg_page
  const uint32_t* seg_start;  // [num_seg]
  const uint32_t* seg_end;    // [num_seg]
  const uint64_t* seg_page;   // [num_seg]
  uint32_t num_seg;           // an upper bound of *num_seg_dev (grid size)
  const uint32_t* num_seg_dev;  // device-side segment count
  uint32_t* seg_T;            // entries after applying
  uint32_t* seg_P;            // pages after applying (1 = in place)
  uint32_t* seg_newpages;     // P - 1
  uint32_t* seg_ver;          // front_version observed
  // per op: bit 31 = already applied in place by k_locate (out_slot)
  const uint32_t* oslot;
  // the same array, written: a new key the upsert stored in an empty slot
  // gets kOpPlaced | slot (k_dir_upkeep reads it; nullable)
  uint32_t* placed;
  // the lock table and the chunk's epoch tag (taken with each page's DMA)
  uint64_t* locks;
  uint32_t num_locks;
  uint64_t tag;
  uint32_t* err;
  // per-page occupancy bound and leaf summary kept by every leaf writer
  uint8_t* leaf_hw;
  uint8_t* sum;
  // split counts for k_upper: segment g adds to range g * up_nb / num_seg
  UpperCtl* ctl;
  uint32_t par;
  uint32_t up_nb;
};
struct UpperArgs;
// u: the split arguments of the chunk with u.early = 1 (small splits taken
// by the upsert kernel itself, upsert.hip) or 0 (every split left to k_upper)
void launch_leaf_upsert(const SegArgs& a, const UpperArgs& u, hipStream_t s);

// the directory form a kept chunk's upkeep writes (UpperArgs.dir_form,
// dir_upkeep.h)
constexpr uint32_t kDirFormNone = 0, kDirFormFp = 1, kDirFormPairs = 2;

// the device-driven split propagation (insert.hip)
struct UpperArgs {
  uint8_t* arena;
  uint64_t arena_bytes;
  uint16_t node;
  uint64_t root;             // the root page (fixed: a root split relocates its left half)
  uint8_t* leaf_hw;
  uint8_t* sum;              // leaf summaries (layout.h)
  uint64_t* locks;
  uint32_t num_locks;
  uint64_t tag;              // lock-word tag of this chunk
  uint64_t batch;            // chunk sequence number (superblock.batches)
  uint32_t par;              // chunk parity (UpperCtl double buffers)
  uint32_t* err;
  UpperCtl* ctl;
  // leaf level, as left by the upsert kernel
  const uint64_t* op_key;
  const uint64_t* op_val;
  const uint32_t* seg_start;
  const uint32_t* seg_end;
  const uint64_t* seg_page;
  const uint32_t* seg_T;
  const uint32_t* seg_P;
  const uint32_t* seg_np;
  const uint32_t* seg_ver;
  const uint32_t* ns_dev;
  uint64_t* leaf_rd;         // per segment: sibling builders that read page 0 (tag << 32 | count)
  // internal levels: separators (key, child) and their target page, ping-pong
  // by level parity (level 1: [1], level 2: [0], ...), sep_cap each
  uint64_t sep_cap;
  uint64_t* sep_key[2];
  uint64_t* sep_ptr[2];
  uint64_t* ipage[2];
  // per segment head (indexed by separator position)
  uint32_t* h_end;
  uint32_t* h_T;
  uint32_t* h_P;
  uint32_t* h_ver;
  uint32_t* h_lk;
  // dense segment list of a level
  uint32_t* d_head;
  uint32_t* d_base;
  uint64_t* int_rd;          // as leaf_rd, per internal segment (tag: chunk and level)
  uint64_t* pub;             // mapped host mirror {batch, next_page, root_level, splits} (nullable)
  // the chunk's deletes (Tree::del), applied after the splits
  const uint64_t* dk;
  const uint64_t* n_del;
  const uint64_t* dir;       // leaf directory (nullable), as in WalkArgs
  uint64_t dir_lo;
  uint64_t dir_n;
  uint32_t dir_shift;
  // nullable: the directory's level-1 / level-2 path pages (launch_leaf_dir),
  // start pages of parent_of walks
  const uint32_t* dir_hint;
  // nullable: the same directory, kept current after this chunk by
  // k_dir_upkeep in form dir_form (dir_upkeep.h: 1 fingerprint, 2 pair form)
  uint64_t* dir_w;
  uint32_t dir_form;
  // pair form: the upkeep writes and keeps the value form (layout.h kDirVals)
  uint32_t dir_vals;
  // the chunk's repair list (nullable): prefixes whose entries the upkeep
  // could not keep exact, for k_dir_repair after it; dir_fix_n[par]
  // counts them (past dir_fix_cap they are lost: the entry stays marked)
  uint32_t* dir_fix;
  uint32_t* dir_fix_n;
  uint32_t dir_fix_cap;
  // nullable: block 0 records the wall clock (100 MHz) at each phase end,
  // stamps[0] = count (tools/upper_stamps.py)
  uint64_t* stamps;
  // diagnostics (shm__upper_force): every block gives up at the first phase
  // hand-off of this launch, as if its wait had timed out (the last block
  // then completes the chunk alone)
  uint32_t force_abort;
  // diagnostics (shm__upper_force bit 1): never propagate directly, every
  // chunk through the level lists and their hand-offs
  uint32_t no_direct;
  // the upsert kernel's copy (upsert.hip): small splits are built and
  // propagated there, their pages counted in UpperCtl.ualloc; 0 in k_upper's
  uint32_t early;
  // nullable (profiling on): per chunk, {unique upserts, deletes, staged
  // segments} added by whichever kernel completes the chunk's counts --
  // k_upper's block 0, or the segmentation's block 0 for a chunk it
  // completes -- before the op buffers are published free
  uint64_t* prof;
  // publish the chunk's tag in the host mirror even without new pages (the
  // host's directory is behind the tree and it watches for a quiet tree)
  uint32_t pub_always;
  // k_dir_upkeep follows this chunk's k_upper and reads the op buffers and
  // the ordering's counts after it: the word kPubApplied (the buffers are
  // free) is then published by k_dir_repair, which runs after the upkeep,
  // and not by the kernel that completes the chunk
  uint32_t pub_later;
  // nullable: the key-value bucket table (valtab.h), kept by k_dir_upkeep in
  // the same launch: every upsert of the chunk stored, every delete removed;
  // vt_ctr[0] counts the buckets the chunk's keys overflowed
  uint64_t* vt;
  uint64_t vt_lo;
  uint64_t vt_n;
  uint32_t vt_shift;
  uint64_t* vt_ctr;
};
constexpr int kUpperStamps = 32;
// diagnostic clock words: k_upper's, then k_bin_unique's 8 phases x kCoarse bins
// + k_bin_unique's 7 x 256 phase words, then k_upper's per-block start (row 8)
// and end (row 9) clocks
// + the upsert kernel's per-block clocks (start, in-place groups done, end)
// and early-split counts, rows of 1024 (tools/upper_stamps.py)
constexpr int kUpsertStamps = kUpperStamps + 10 * 256;
constexpr int kStampWords = kUpsertStamps + 9 * 1024;
uint32_t upper_blocks();
// k_upper's blocks (512 threads) fit a CU at all
bool upper_resident();
void launch_upper(const UpperArgs& a, hipStream_t s);

void launch_empty_leaf(uint8_t* arena, uint64_t page_off, uint8_t* sum, hipStream_t s);
void launch_write_superblock(uint8_t* arena, const Superblock& sb, hipStream_t s);

// ---- ordering (partition.hip, isort.hip) ------------------------------------
// order a get batch by its top 16 key bits (partition.hip): keys_out is the
// walk order, src[p] = keys1 slot of walk slot p, pos1[i] = keys1 slot of
// input i.  M = [kMaxTiles][kCoarse] tile counts, S = group sums (all zero
// between calls; zero it once at creation), chunks = 2 x
// partition_chunk_slots(n) words.
constexpr int kCoarse = 256;
constexpr int kFine = 256;
constexpr int kMaxTiles = 512;
constexpr int kFineCap = 8192;
constexpr int kPartHistWords = kMaxTiles * kCoarse;
constexpr int kPartGroupWords = kMaxTiles / 16 * kCoarse;
uint32_t partition_chunk_slots(uint64_t n);
// get ordering by the top 16 bits of the key's offset in the shard's range
// [key_lo, key_lo + 2^key_bits) (keys outside clamp to the first/last bucket)
void launch_partition(const uint64_t* keys, uint64_t n, uint64_t key_lo, uint32_t key_bits,
                      uint32_t* M, uint32_t* S, uint32_t* chunks, uint64_t* keys1,
                      uint32_t* pos1, uint64_t* keys_out, uint32_t* src, hipStream_t s);
// insert ordering, step 2: the coarse pass alone over per-group
// de-duplicated runs (group gi = keys [gi * kIsortTile, ...) holds gcount[gi]
// keys), carrying a u32 payload; bins = 2 x 256 words of (start, count)
void launch_partition_coarse(const uint64_t* keys, uint64_t n, const uint32_t* gcount,
                             const uint32_t* pay_in, uint64_t key_lo, uint32_t key_bits,
                             uint32_t* M, uint32_t* S, uint64_t* keys1, uint32_t* pay1,
                             uint32_t* bins, hipStream_t s);
// insert ordering (isort.hip).  Step 1: every 2048-op tile reduced to its
// last writer per key (LDS hash table, atomic max of the op index); a kKeyMax
// key rejects the chunk: gate = tag (k_bin_unique then emits nothing) and the
// sticky error word gets kErrKeyMax; with skip_pad, kKeyMax keys are slot
// padding of a routed insert (shard.cpp) and are skipped instead.
constexpr int kIsortTile = 2048;
constexpr uint32_t kErrKeyMax = 1u << 31;
// For batches of <= kMaxTiles tiles it also writes the coarse pass's tile
// histograms M and group sums S (launch_partition_coarse then skips its own).
// Tile mode (Mx non-null, <= kMaxTiles tiles): each tile's survivors are
// written sorted by coarse bin, bin b's run at tile base + Mx[b][tile] with
// M[b][tile] keys (bin-major, [kCoarse][kMaxTiles]: a bin's row is read
// whole), and k_bin_unique gathers them (TileRuns) -- no coarse scatter
// pass.  S still gets the group sums.
void launch_tile_dedup(const uint64_t* keys, uint64_t n, uint64_t* keys_out, uint32_t* idx_out,
                       uint32_t* gcount, uint32_t* err, uint32_t* gate, uint32_t tag,
                       uint64_t key_lo, uint32_t key_bits, uint32_t* M, uint32_t* S,
                       uint32_t* Mx, int skip_pad, hipStream_t s);
// the tile mode's runs for k_bin_unique (tiles = 0: the coarse pass's bins)
struct TileRuns {
  const uint64_t* keys;  // tile_dedup's keys_out
  const uint32_t* idx;   // tile_dedup's idx_out
  const uint32_t* M;
  const uint32_t* Mx;
  uint32_t tiles;
};
// steps 3-4: per-bin last-writer dedup + sort (bins of <= 6144 ops in LDS,
// larger ones by an LSD radix sort through global scratch kscr / iscr, n
// words each), then uk / uv / dk at the bins' prefixes and (upserts, deletes)
// in counts[0..1]; lbw = kCoarse tagged count words (the bins' look-back),
// lrank = one u32 per op (bins over 6144 ops)
void launch_bin_unique(uint64_t* keys1, uint32_t* pay1, const uint32_t* bins, uint64_t key_lo,
                       uint32_t key_bits, const uint64_t* vals, uint32_t* lrank, uint64_t* lbw,
                       uint64_t* kscr, uint32_t* iscr, uint64_t* uk, uint64_t* uv, uint64_t* dk,
                       uint64_t* counts, uint32_t* err, uint32_t* S, const uint32_t* gate,
                       uint32_t tag, uint64_t* stamps, const TileRuns& tr, uint32_t* ids,
                       hipStream_t s);
// the constants that decide an ordering's path (shm__order_limits): tile
// size, tiles in tile mode, ops of a bin sorted in LDS, keys of a fine
// sub-bucket ranked in place, coarse bins, fine sub-buckets
void order_limits(uint64_t out[6]);
// out[i] = vals1[pos1[i]], found[i] = out[i] != 0
void launch_unpartition(const uint64_t* vals1, const uint32_t* pos1, uint64_t n,
                        uint64_t* out, uint8_t* found, hipStream_t s);

// ---- segmentation and tile scans (tile_scan.hip) ------------------------------
// Staged segments of a located op list (n_dev: device-side op count <= n):
// the runs of ops on one page whose page k_locate marked (pnew[page] ==
// tag: it gets a new key); runs of in-place overwrites are left out.  One
// launch: per 1024-op tile a staged-head count published in a tagged word
// (lbw: seg_tiles(n) u64, zero at creation), the counts of the tiles before
// it summed, its segments filled.
constexpr uint32_t kSegTile = 1024;
inline uint64_t seg_tiles(uint64_t n) { return (n + kSegTile - 1) / kSegTile; }
// any_new (nullable): the locate's any-page-marked word (== tag: some page
// gets a new key; otherwise there are no staged segments)
// self_after: a tile that has waited this many polls for an earlier tile's
// word counts that tile's staged heads itself (0: at once, the test knob), so
// no tile depends on another being placed (seg_tile.h)
void launch_segment(const uint64_t* page, uint64_t n, const uint64_t* n_dev, uint64_t* lbw,
                    uint32_t* seg_start, uint32_t* seg_end, uint64_t* seg_page,
                    uint32_t* num_seg, const uint8_t* pnew, uint32_t tag,
                    const uint32_t* any_new, uint32_t* err, hipStream_t s,
                    const UpperArgs* quick, uint32_t* ids, uint32_t self_after,
                    const uint64_t* ndel_src, uint64_t* ndel_dst);
// exclusive scan of u64 in one launch (lbw: seg_tiles(n) tagged words, zero
// at creation; tag: a fresh 16-bit value per call, lbw zeroed again when it
// wraps); tot = {total, *err} for the range scan's one read-back
void launch_scan_u64_total(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* lbw,
                           uint32_t tag, const uint32_t* err, uint64_t* tot, uint32_t* err_out,
                           uint32_t* ids, hipStream_t s);
// x[i] += c for i < n
void launch_add_u64(uint64_t* x, uint64_t n, uint64_t c, hipStream_t s);

// ---- multi-GPU routing (route.hip) ---------------------------------------------
// The shards' boundaries for routing: s[j - 1] = the first key of shard j
// (j = 1 .. P - 1, ascending, repeats allowed: shard [x, x) is empty, none
// equals kKeyMax), so a key's owner is the number of splitters <= it.  Passed
// by value in the kernel arguments.  Every routing launch takes a nullable
// split (nullptr: equal slices, the kernels as they were before splitters)
// and a mode for the owner search (0 or 2: binary search in LDS; 1: compare-
// and-add over the kernel arguments, P <= 16, measured slower --
// tools/route_bounds.py)
struct RouteSplit {
  uint64_t s[63];
};
// stable bucketing by owning shard; cm = route_scratch_words(n) words
uint64_t route_scratch_words(uint64_t n_max);
// keymax / err (nullable): a routed insert's batch holding kKeyMax is
// rejected whole (every count 0, kErrKeyMax in *err; keymax: a zeroed word)
void launch_route_bucket(const uint64_t* keys, uint64_t n, uint32_t shards,
                         uint64_t* counts, uint64_t* keys_out, uint32_t* perm,
                         uint32_t* cm, uint32_t* keymax, uint32_t* err, hipStream_t s,
                         const RouteSplit* split = nullptr, int mode = 0);
// out[i] = in[perm[i]]
void launch_permute(const uint64_t* in, const uint32_t* perm, uint64_t n, uint64_t* out,
                    hipStream_t s);
void launch_unpermute(const uint64_t* in, const uint32_t* perm, uint64_t n,
                      uint64_t* out, uint8_t* found, hipStream_t s);
// fixed-capacity get exchange (shard.cpp): keys straight into P runs of cap
// slots (kKeyMax padding; spos[i] = input i's slot, ~0 when its run is full;
// cursor = P + 1 words: per-peer routed counts, then the overflow count).
// An overflowed key goes to ovk / ovi (its input position) for the second
// round; with ovk == nullptr it finds nothing and kErrOverflow goes to *err.
// The results are gathered back to input order.
// Own run (own_out non-null): the run of peer `own` (this rank) is written to
// own_out[0, cap) instead of out[own * cap, ...), i.e. straight into the
// receive buffer the local get reads, so it never enters the collective
// (VERDICT r4 #2); spos still names slot own * cap + pos.
// the routed get's slot placement (k_route_slots); ctr: the claim
// words, route_ctr_words(P) u32 zeroed once at allocation
constexpr uint32_t kCtrStride = 64;  // 256 B: one claim word per line
inline uint64_t route_ctr_words(uint32_t P) { return (uint64_t)(P + 2) * kCtrStride; }
void launch_route_slots(const uint64_t* keys, uint64_t n, uint32_t P, uint64_t cap,
                        uint32_t* cursor, uint32_t* ctr, uint64_t* out, uint32_t* spos,
                        uint64_t* ovk, uint32_t* ovi, uint32_t* err, hipStream_t s, uint32_t own = 0,
                        uint64_t* own_out = nullptr, bool fill = true,
                        const RouteSplit* split = nullptr, int mode = 0);
// out[i] = in[spos[i]]; with own_src non-null, slots of run `own` (own * cap
// .. + cap) are read from own_src (the local get's results, never exchanged)
void launch_route_gather(const uint64_t* in, const uint32_t* spos, uint64_t n, uint64_t* out,
                         uint8_t* found, hipStream_t s, uint32_t own = 0, uint64_t cap = 0,
                         const uint64_t* own_src = nullptr);
// out[ovi[perm[j]]] = in[j], found likewise (the overflow round's results)
void launch_route_ov_scatter(const uint64_t* in, const uint32_t* perm, const uint32_t* ovi,
                             uint64_t m, uint64_t* out, uint8_t* found, hipStream_t s);
// routed insert: the bucketed runs (cnt[p] keys of peer p, in order) packed
// into P slot runs of cap (kKeyMax / 0 padding)
// (own_k / own_v non-null: run `own` goes there, straight into the receive
// buffers of the local insert, instead of pk / pv)
void launch_route_pack(const uint64_t* kb, const uint64_t* vb, const uint64_t* cnt, uint32_t P,
                       uint64_t cap, uint64_t* pk, uint64_t* pv, hipStream_t s, uint32_t own = 0,
                       uint64_t* own_k = nullptr, uint64_t* own_v = nullptr);
// routed range scans: shard p owns [b[p], b[p + 1]) (P <= 16; b[P] unused);
// b[p + 1] <= b[p] (repeated splitters): shard p owns nothing
struct ShardBounds {
  uint64_t b[17];
};
// the P x cap piece matrix of n scans (empty pieces: lo = 1 > hi = 0)
void launch_range_pieces(const uint64_t* from, const uint64_t* to, uint64_t n, uint64_t cap,
                         uint32_t P, const ShardBounds& bnd, uint64_t* plo, uint64_t* phi,
                         hipStream_t s);
// rw[r] = sum of row r of rc, rw[P + p] = sum of row p of bc (P x cap
// matrices); counts[j] = sum over p of bc[p][j], j < n
void launch_range_sums(const uint64_t* rc, const uint64_t* bc, uint64_t n, uint64_t cap,
                       uint32_t P, uint64_t* rw, uint64_t* counts, hipStream_t s);
// scan j's pieces' values (bv at bsc[p][j], bc[p][j] of them) to
// vals[offsets[j] ...] in shard order, bounded by vals_cap
void launch_range_assemble(const uint64_t* bv, const uint64_t* bc, const uint64_t* bsc,
                           uint64_t n, uint64_t cap, uint32_t P, const uint64_t* offsets,
                           uint64_t* vals, uint64_t vals_cap, hipStream_t s, uint64_t pitch = 0);
void launch_range_pitch(const uint64_t* rvals, const uint64_t* rw, uint32_t P, uint64_t pitch,
                        uint64_t* out, uint64_t rvcap, uint64_t vals_cap, uint64_t* status,
                        hipStream_t s);

// ---- batched range scans (range.hip) -------------------------------------------
struct RangeArgs {
  const uint8_t* arena;
  uint64_t arena_bytes;
  uint16_t node;
  uint64_t root;
  const uint64_t* from;
  const uint64_t* to;
  uint64_t n;
  uint64_t* counts;
  const uint64_t* offsets;  // nullptr -> count only
  uint64_t* vals;
  uint32_t* err;
  // leaf directory (nullable), as in WalkArgs
  const uint64_t* dir;
  uint64_t dir_lo;
  uint64_t dir_n;
  uint32_t dir_shift;
  // staging (nullable): the count pass also keeps up to stage_cap values of
  // scan q at stage[q * stage_cap]; the fill pass copies those scans from
  // there instead of walking their leaves again
  uint64_t* stage;
  uint32_t stage_cap;
  // fill pass: values at output index >= vals_cap are dropped (the async
  // batch call writes before the host knows the total; it reports the total)
  uint64_t vals_cap;
  // per-page occupancy bound (nullable, layout.h): a sibling leaf's bytes
  // past its last possibly valid slot are not read
  const uint8_t* leaf_hw;
  // slotted scans (shm_range_query_slots, nullable): += scans whose count
  // passed stage_cap, |= this launch's error bits (the caller zeroes them)
  uint64_t* status;
};
void launch_range(const RangeArgs& a, hipStream_t s);

// ---- ordered scans with a count limit (scan.hip) ----------------------------------
struct ScanArgs {
  const uint8_t* arena;
  uint64_t arena_bytes;
  uint16_t node;
  uint64_t root;
  const uint64_t* from;
  const uint64_t* to;  // nullable: no upper bound
  uint64_t n;
  uint32_t limit;      // 1 .. 2^31 - 1 pairs per scan
  // scan i's first min(limit, matches) pairs in ascending key order at
  // keys / vals [i * limit ...], their number in counts[i]; the rest of the
  // row is not written
  uint64_t* keys;
  uint64_t* vals;
  uint64_t* counts;
  uint32_t* err;
  // leaf directory (nullable), as in WalkArgs
  const uint64_t* dir;
  uint64_t dir_lo;
  uint64_t dir_n;
  uint32_t dir_shift;
  // per-page occupancy bound (nullable), as in RangeArgs
  const uint8_t* leaf_hw;
  // nullable: status[1] |= this launch's error bits (status[0] is left alone)
  uint64_t* status;
};
void launch_scan(const ScanArgs& a, hipStream_t s);
// the same arguments read downwards (shm_rscan_batch): from = the start, to =
// the stop (nullable: 0); pairs with to <= key <= from in descending key order
void launch_rscan(const ScanArgs& a, hipStream_t s);

// ---- bulk load (bulk.hip) -------------------------------------------------------
// Every level deals its C items (pairs for leaves, children above) over its
// pages evenly: q = C / pages each, one more for the first r = C % pages.
// status |= 1 unless keys[0, n) strictly ascend (so none is kKeyMax but
// possibly the last, which is rejected too) and no value is kValueNull
void launch_bulk_check(const uint64_t* keys, const uint64_t* vals, uint64_t n, uint32_t* status,
                       hipStream_t s);
// the leaves: leaf p is arena page page0 + p (whole page, summary line,
// leaf_hw byte), its sibling the next page, 0 for the last
struct BulkLeafArgs {
  uint8_t* arena;
  uint16_t node;
  const uint64_t* keys;
  const uint64_t* vals;
  uint64_t pages;  // >= 1 (one empty leaf for no pairs)
  uint64_t q, r;
  uint64_t page0;
  uint8_t* sum;
  uint8_t* leaf_hw;
};
void launch_bulk_leaves(const BulkLeafArgs& a, hipStream_t s);
// one internal level: page p is arena page page0 + p, its children the pages
// child0 + c of the level below.  A child's lowest fence comes from low_in[c]
// (what the level below wrote to its low_out), or with low_in == nullptr
// (level 1) from keys[] by the leaves' deal (leaf_q, leaf_r); child 0's is 0
struct BulkLevelArgs {
  uint8_t* arena;
  uint16_t node;
  uint32_t level;
  const uint64_t* keys;
  uint64_t leaf_q, leaf_r;
  const uint64_t* low_in;
  uint64_t* low_out;  // nullable (the root)
  uint64_t pages;
  uint64_t q, r;
  uint64_t page0, child0;
  uint8_t* sum;
  uint8_t* leaf_hw;
};
void launch_bulk_level(const BulkLevelArgs& a, hipStream_t s);

// ---- sorted export of a key range (export.hip) -----------------------------------
// One argument block for the expansion of an internal level and for the leaf
// passes.  A unit is (page, upper bound of the key range its parent gave it);
// a level's list holds its units in key order.
struct ExportArgs {
  const uint8_t* arena;
  uint64_t arena_bytes;
  uint16_t node;
  uint32_t level;            // expansion: the level of the units read (>= 1)
  uint64_t lo, hi;           // the exported range, inclusive
  const uint64_t* in_page;   // the units read: n of them
  const uint64_t* in_bound;
  uint64_t n;
  uint64_t* cnt;             // count passes: per unit, its children / its valid pairs
  const uint64_t* off;       // emit / write passes: the exclusive scan of cnt
  uint64_t* out_page;        // expansion's emit pass: the units of the level below,
  uint64_t* out_bound;       // out_cap of them at most
  uint64_t out_cap;
  uint64_t* keys;            // leaf write pass (either nullable): the pairs, `total`
  uint64_t* vals;            // of them as the count pass found
  uint64_t total;
  uint64_t max_pages;        // allocated pages: bounds every chain walk
  const uint8_t* leaf_hw;    // per-page occupancy bound (nullable), as in RangeArgs
  uint32_t* err;
};
void launch_export_seed(uint64_t root, uint64_t* page, uint64_t* bound, hipStream_t s);
void launch_export_expand(const ExportArgs& a, bool emit, hipStream_t s);
void launch_export_leaf(const ExportArgs& a, bool write, hipStream_t s);
// out = exclusive scan of in[0, n) in three launches, none waiting on another
// block; bsum: export_scan_tiles(n) + 1 words of scratch; tot = {total, *err}
uint64_t export_scan_tiles(uint64_t n);
void launch_export_scan(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* bsum,
                        uint64_t* tot, const uint32_t* err, hipStream_t s);

// ---- order statistics (order.hip) ------------------------------------------------
// The order index: the whole tree's leaf units in key order (page, bound, and
// off = the exclusive scan of their valid-pair counts with the total at
// off[units]: the last export count pass's lists, copied), and over bound[]
// and over off[1 ..] a pyramid of sampled levels.  Level 0 is the array
// itself, level j + 1 holds the last word of every kOrdFan words of level j
// (a block's largest), every level is padded to whole blocks with ~0, and the
// top level is one block.  "The first word above x" is then one 128 B line per
// level: the block found on the level above, one compare per lane.
constexpr int kOrdFan = 16;     // words per block = lanes per query
constexpr int kOrdLevels = 8;   // 16^8 units: more than any arena holds pages
struct OrderArgs {
  const uint8_t* arena;
  uint64_t arena_bytes;
  uint16_t node;
  const uint8_t* leaf_hw;    // per-page occupancy bound (nullable), as in RangeArgs
  uint32_t* err;
  uint64_t* status;          // nullable: error bits ORed into status[1]
  const uint64_t* page;      // the units
  const uint64_t* bound;
  const uint64_t* off;       // units + 1 words
  const uint64_t* blv[kOrdLevels];  // blv[0] = bound
  const uint64_t* olv[kOrdLevels];  // olv[0] = off + 1
  uint64_t nblk[kOrdLevels];        // blocks of level j (both pyramids)
  uint32_t nlev;
  uint64_t units, total;
  uint64_t max_pages;        // allocated pages at the build: bounds every chain walk
  const uint64_t* in0;       // rank: keys; count: from; select: ranks
  const uint64_t* in1;       // count: to
  uint64_t n;
  uint64_t* out0;            // rank: ranks; count: counts; select: keys (nullable)
  uint64_t* out1;            // select: values (nullable)
  uint8_t* found;            // select (nullable)
};
void launch_order_rank(const OrderArgs& a, hipStream_t s);
void launch_order_count(const OrderArgs& a, hipStream_t s);
void launch_order_select(const OrderArgs& a, hipStream_t s);
// out[i] = in[min(kOrdFan i + kOrdFan - 1, n_in - 1)] for i < ceil(n_in / kOrdFan)
void launch_order_sample(const uint64_t* in, uint64_t n_in, uint64_t* out, hipStream_t s);

// ---- read-back, generators, lock_bench, diagnostics (service.hip) ----------------
// dst[i] = src[i] for i < nw (<= 256, dst in mapped host memory), then a
// system-scope release store of seq to *flag; clear: src[i] is exchanged
// with 0 (atomically) as it is read
void launch_readback(uint32_t* dst, const uint32_t* src, uint32_t nw, uint32_t* flag,
                     uint32_t seq, int clear, hipStream_t s);
void launch_gen_keys(uint64_t first, uint64_t n, uint64_t keyspace,
                     uint64_t* out, hipStream_t s);
void launch_hash_ids(const uint64_t* ids, uint64_t n, uint64_t keyspace, uint64_t* out,
                     hipStream_t s);
// Tree::lock_bench over the HBM lock table: each key's word taken (atomicCAS
// to tag | 1) and released (tag), bounded spins (kErrLock)
void launch_lock_bench(const uint64_t* keys, uint64_t n, uint64_t* locks, uint32_t num_locks,
                       uint64_t tag, uint32_t* err, hipStream_t s);
// diagnostics (shm__hog): n blocks that each hold a whole CU's LDS and spin
// until `ticks` of the 100 MHz wall clock have passed since they started
void launch_hog(uint32_t n, uint64_t ticks, hipStream_t s);
// diagnostics (shm__mark): an empty kernel marking a profile window's edge
void launch_mark(uint32_t tag, hipStream_t s);

}  // namespace dev
}  // namespace shm
