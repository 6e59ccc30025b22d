"""A host-side reference for the side state of the pages and for the
structural check, in numpy.

Every arena page carries two pieces of device state that are not part of its
bytes: the leaf summary line (64 B) and the occupancy bound (one byte).
Every leaf writer keeps them and every reader trusts them: the summary walk of
the get reads only entries whose fingerprint matches and turns right on the
line's highest fence, the page readers stop at the occupancy bound, and the
page sweeps of the directory's and the bucket table's builds take a page as a
leaf of the tree by its tag alone.  This module shares nothing with the
library or the oracle: it restates the documented formats (layout.h) as
constants of its own and checks a raw dump of the side state
(Tree.side_dump()) against a raw dump of the pages (Tree.dump_image()).

The summary line of page p (u8 line[64]):
  bytes 0..7   the highest fence of the leaf (u64, little endian)
  byte  8      0xA5 while the line describes a current leaf of the tree
  byte  9 + s  key_fp of slot s's key where its value != 0 (a torn entry
               included), 0 where the value is 0; s < 54
  byte  63     belongs to no field
The occupancy bound hw[p]: every slot >= hw holds value 0; 0xFF = unknown.

structure() restates the invariants of the library's structural check
(check_image, behind Tree.check()) and names what it finds.
"""
import numpy as np

from image_builder import (INTERNAL_ENTRY, INTERNAL_SLOTS, KEY_MAX, LEAF_ENTRY, LEAF_SLOTS,
                           OFF_FRONT_VER, OFF_HIGHEST, OFF_INTERNAL_REAR, OFF_LAST_INDEX,
                           OFF_LEAF_REAR, OFF_LEFTMOST, OFF_LEVEL, OFF_LOWEST, OFF_RECORDS,
                           OFF_SIBLING, PAGE, reached_pages)

U64 = np.uint64

# the summary line
SUM_BYTES, SUM_OFF_HIGHEST, SUM_OFF_TAG, SUM_OFF_FP = 64, 0, 8, 9
SUM_LEAF = 0xA5
HW_FULL = 0xFF

# side_violations' kinds
UNTAGGED_LEAF, TAGGED_OTHER, HIGHEST = "untagged_leaf", "tagged_other", "highest"
FP_MISSING, FP_STALE, HW_HIDES, LINE_PAST_END = "fp_missing", "fp_stale", "hw_hides", "line_past_end"
SIDE_KINDS = (UNTAGGED_LEAF, TAGGED_OTHER, HIGHEST, FP_MISSING, FP_STALE, HW_HIDES, LINE_PAST_END)


def key_fp(k):
    """the 8-bit fingerprint of a key (array of uint64):
    (k * 0x9E3779B97F4A7C15 mod 2^64) >> 56, with 0 read as 1"""
    k = np.asarray(k, dtype=U64)
    with np.errstate(over="ignore"):
        f = ((k * U64(0x9E3779B97F4A7C15)) >> U64(56)).astype(np.uint8)
    return np.where(f == 0, np.uint8(1), f).astype(np.uint8)


def _pages(img):
    img = np.asarray(img, dtype=np.uint8).reshape(-1)
    return img[:(img.size // PAGE) * PAGE].reshape(-1, PAGE)


def _f64(pg, off):
    return np.ascontiguousarray(pg[:, off:off + 8]).view("<u8").ravel()


def _slots(pg):
    """(keys, values) of the 54 leaf slots of every page, (n, 54) uint64 each"""
    rec = pg[:, OFF_RECORDS:OFF_RECORDS + LEAF_SLOTS * LEAF_ENTRY].reshape(-1, LEAF_SLOTS, LEAF_ENTRY)
    k = np.ascontiguousarray(rec[:, :, 1:9]).view("<u8").reshape(-1, LEAF_SLOTS)
    v = np.ascontiguousarray(rec[:, :, 9:17]).view("<u8").reshape(-1, LEAF_SLOTS)
    return k, v


def reached_leaves(img, root_ptr):
    """(reached, leaf): masks over the image's pages: the pages the root
    reaches, and those of them that are leaves (no leftmost pointer, level 0)"""
    pg = _pages(img)
    reached = reached_pages(pg, root_ptr)
    leaf = reached & (_f64(pg, OFF_LEFTMOST) == 0) & (pg[:, OFF_LEVEL] == 0)
    return reached, leaf


def side_expected(img, root_ptr, n_pages):
    """The exact summary lines of an image, (n_pages, 64) uint8: the tag and
    the highest fence for every leaf the root reaches, fp[s] = key_fp(key)
    where slot s's value != 0 (torn entries included), 0 elsewhere; every
    other page's line is zero.  n_pages may exceed the image's pages."""
    pg = _pages(img)
    _, leaf = reached_leaves(pg, root_ptr)
    assert n_pages >= pg.shape[0] or not leaf[n_pages:].any()
    lines = np.zeros((n_pages, SUM_BYTES), dtype=np.uint8)
    at = np.nonzero(leaf[:n_pages])[0]
    k, v = _slots(pg[at])
    lines[at, SUM_OFF_HIGHEST:SUM_OFF_HIGHEST + 8] = pg[at, OFF_HIGHEST:OFF_HIGHEST + 8]
    lines[at, SUM_OFF_TAG] = SUM_LEAF
    lines[at, SUM_OFF_FP:SUM_OFF_FP + LEAF_SLOTS] = np.where(v != 0, key_fp(k), np.uint8(0))
    return lines


def hw_tight(img, root_ptr, n_pages):
    """The tightest sound occupancy bounds of an image, (n_pages,) uint8:
    1 + the last slot with a value != 0 for every reached leaf (0 for a leaf
    without one), 0xFF for every other page."""
    pg = _pages(img)
    _, leaf = reached_leaves(pg, root_ptr)
    hw = np.full(n_pages, HW_FULL, dtype=np.uint8)
    at = np.nonzero(leaf[:n_pages])[0]
    _, v = _slots(pg[at])
    hw[at] = np.where(v != 0, np.arange(1, LEAF_SLOTS + 1), 0).max(axis=1)
    return hw


def side_violations(img, root_ptr, lines, hw, next_page):
    """What a dump of the side state (lines (n, 64) uint8, hw (n,) uint8, n
    may reach past next_page) gets wrong about the image, as a list of
    (kind, page, slot):

      untagged_leaf  a reached leaf has no tag (slot -1); its line is not
                     looked at further
      tagged_other   an internal page, or a page below next_page the root
                     does not reach, has the tag (slot -1)
      highest        the line's fence != the page's (slot -1)
      fp_missing     value != 0 and fp != key_fp(key): a get would miss it
      fp_stale       value == 0 and fp != 0
      hw_hides       hw != 0xFF and a slot >= hw has value != 0
      line_past_end  a nonzero line byte for a page >= next_page (slot: the
                     byte's index in the line)
    """
    pg = _pages(img)
    lines = np.asarray(lines, dtype=np.uint8).reshape(-1, SUM_BYTES)
    hw = np.asarray(hw, dtype=np.uint8).reshape(-1)
    n = lines.shape[0]
    assert hw.size == n and pg.shape[0] <= n and next_page <= n
    assert next_page >= pg.shape[0] or not reached_pages(pg, root_ptr)[next_page:].any()
    _, leaf = reached_leaves(pg, root_ptr)
    is_leaf = np.zeros(n, dtype=bool)
    is_leaf[:pg.shape[0]] = leaf
    below = np.arange(n) < next_page
    tagged = lines[:, SUM_OFF_TAG] == SUM_LEAF
    out = []
    out += [(UNTAGGED_LEAF, int(p), -1) for p in np.nonzero(is_leaf & ~tagged)[0]]
    out += [(TAGGED_OTHER, int(p), -1) for p in np.nonzero(below & ~is_leaf & tagged)[0]]
    at = np.nonzero(is_leaf)[0]
    k, v = _slots(pg[at])
    line_hi = np.ascontiguousarray(lines[at, SUM_OFF_HIGHEST:SUM_OFF_HIGHEST + 8]).view("<u8").ravel()
    page_hi = _f64(pg[at], OFF_HIGHEST)
    fp = lines[at, SUM_OFF_FP:SUM_OFF_FP + LEAF_SLOTS]
    look = tagged[at]
    out += [(HIGHEST, int(at[i]), -1) for i in np.nonzero(look & (line_hi != page_hi))[0]]
    miss = look[:, None] & (v != 0) & (fp != key_fp(k))
    stale = look[:, None] & (v == 0) & (fp != 0)
    hidden = (hw[at] != HW_FULL)[:, None] & (np.arange(LEAF_SLOTS)[None, :] >= hw[at][:, None]) & (v != 0)
    for kind, mask in ((FP_MISSING, miss), (FP_STALE, stale), (HW_HIDES, hidden)):
        out += [(kind, int(at[i]), int(s)) for i, s in zip(*np.nonzero(mask))]
    past, byte = np.nonzero(lines[next_page:] != 0)
    out += [(LINE_PAST_END, int(next_page + p), int(b)) for p, b in zip(past, byte)]
    return out


# ---- the structural check, restated --------------------------------------------------
# structure()'s kinds
BAD_ROOT, BAD_SIBLING, BAD_CHILD = "bad_root", "bad_sibling", "bad_child"
LEVEL, LEAF_KIND, VERSION, FENCES, KEY_OUTSIDE = "level", "leaf_kind", "version", "fences", "key_outside"
LEAF_FULL, DUPLICATE, LAST_INDEX, CHILD_LOWEST = "leaf_full", "duplicate", "last_index", "child_lowest"
SEPARATORS, CHILD_LEVEL, LAST_HIGHEST, CHILD_OFF_CHAIN = \
    "separators", "child_level", "last_highest", "child_off_chain"


def structure(img, root, node=0):
    """The invariants of a sound page image, checked from the root down; returns
    (violations, counts): a list of (kind, page, index) and {"leaves",
    "internal", "keys"} (keys: slots with value != 0).  An image is sound when
    the list is empty.

    A pointer is good when it is not 0, names `node`, and its byte offset is a
    multiple of 1024, at least 1024 (page 0 is the superblock) and inside the
    image.  The root pointer is good (bad_root).  The level of the root page
    is the top level; the pages of level L are those on the sibling chain that
    starts at the root (top level) or at the leftmost pointer of the first
    page of level L + 1.  Along a chain every sibling pointer is 0 or good
    (bad_sibling) and every page
      has level byte L (level); has a leftmost pointer iff L > 0 (leaf_kind);
      has equal front and rear versions (version);
      has lowest == the highest of the page before it, 0 for the first, and
      highest > lowest (fences); the last page's highest is 2^64 - 1
      (last_highest).
    A leaf holds at most 53 slots with value != 0 (leaf_full), each key inside
    [lowest, highest) (key_outside) and no key twice (duplicate).  An internal
    page has last_index in -1..59 (last_index); its leftmost pointer is good
    and names a page whose lowest is the page's lowest (child_lowest); its
    last_index + 1 separators ascend strictly inside (lowest, highest)
    (separators); record j's pointer is good (bad_child), names a page whose
    lowest is separator j (child_lowest) and whose level is L - 1
    (child_level).  Every child a page of level L names, leftmost included, is
    on the chain of level L - 1 (child_off_chain): a page that hangs on its
    left sibling alone is on the chain and needs no record.

    The walk stops at a pointer it cannot follow, and a chain stops at a page
    whose fences do not continue it (so a sibling pointer that turns back
    ends the walk)."""
    pg = _pages(img)
    n = pg.shape[0]
    leftmost, sibling = _f64(pg, OFF_LEFTMOST).tolist(), _f64(pg, OFF_SIBLING).tolist()
    lowest, highest = _f64(pg, OFF_LOWEST).tolist(), _f64(pg, OFF_HIGHEST).tolist()
    level = pg[:, OFF_LEVEL].tolist()
    last = np.ascontiguousarray(pg[:, OFF_LAST_INDEX:OFF_LAST_INDEX + 2]).view("<i2").ravel().tolist()
    front = pg[:, OFF_FRONT_VER].tolist()
    rear_leaf, rear_int = pg[:, OFF_LEAF_REAR].tolist(), pg[:, OFF_INTERNAL_REAR].tolist()
    bad, counts = [], {"leaves": 0, "internal": 0, "keys": 0}

    def page(ptr):
        off = int(ptr) >> 16
        if ptr == 0 or (int(ptr) & 0xFFFF) != node or off % PAGE or not 0 < off // PAGE < n:
            return None
        return off // PAGE

    p = page(root)
    if p is None:
        return [(BAD_ROOT, -1, -1)], counts
    L = level[p]
    named = set()
    leaves = []
    while L >= 0:
        chain, kids, below, want = [], set(), None, 0
        while p is not None:
            is_leaf = leftmost[p] == 0
            if level[p] != L:
                bad.append((LEVEL, p, -1))
            elif is_leaf != (L == 0):
                bad.append((LEAF_KIND, p, -1))
            elif front[p] != (rear_leaf[p] if is_leaf else rear_int[p]):
                bad.append((VERSION, p, -1))
            elif lowest[p] != want or highest[p] <= lowest[p]:
                bad.append((FENCES, p, -1))
            if bad:
                return bad, counts
            chain.append(p)
            if is_leaf:
                leaves.append(p)
            else:
                cnt = last[p] + 1
                if not 0 <= cnt <= INTERNAL_SLOTS - 1:
                    return bad + [(LAST_INDEX, p, -1)], counts
                c = page(leftmost[p])
                if c is None or lowest[c] != lowest[p]:
                    return bad + [(CHILD_LOWEST if c is not None else BAD_CHILD, p, -1)], counts
                if below is None:
                    below = c
                kids.add(c)
                rec = np.ascontiguousarray(
                    pg[p, OFF_RECORDS:OFF_RECORDS + INTERNAL_ENTRY * cnt]).view("<u8").tolist()
                prev = lowest[p]
                for j in range(cnt):
                    sep, c = rec[2 * j], page(rec[2 * j + 1])
                    if sep <= prev or sep >= highest[p]:
                        return bad + [(SEPARATORS, p, j)], counts
                    prev = sep
                    if c is None:
                        return bad + [(BAD_CHILD, p, j)], counts
                    if lowest[c] != sep:
                        return bad + [(CHILD_LOWEST, p, j)], counts
                    if level[c] != L - 1:
                        return bad + [(CHILD_LEVEL, p, j)], counts
                    kids.add(c)
                counts["internal"] += 1
            want = highest[p]
            if sibling[p] == 0:
                break
            nxt = page(sibling[p])
            if nxt is None:
                return bad + [(BAD_SIBLING, p, -1)], counts
            p = nxt
        if want != KEY_MAX:
            return bad + [(LAST_HIGHEST, chain[-1], -1)], counts
        off = sorted(named - set(chain))
        if off:
            return bad + [(CHILD_OFF_CHAIN, c, -1) for c in off], counts
        named, p, L = kids, below, L - 1
    # the leaves at once
    at = np.array(leaves, dtype=np.int64)
    k, v = _slots(pg[at])
    lo = _f64(pg[at], OFF_LOWEST)[:, None]
    hi = _f64(pg[at], OFF_HIGHEST)[:, None]
    held = v != 0
    outside = held & ((k < lo) | (k >= hi))
    bad += [(KEY_OUTSIDE, int(at[i]), int(s)) for i, s in zip(*np.nonzero(outside))]
    bad += [(LEAF_FULL, int(at[i]), -1) for i in np.nonzero(held.sum(axis=1) > LEAF_SLOTS - 1)[0]]
    # a held key is below its leaf's highest fence, so never 2^64 - 1
    order = np.sort(np.where(held & ~outside, k, U64(KEY_MAX)), axis=1)
    twice = (order[:, 1:] == order[:, :-1]) & (order[:, 1:] != U64(KEY_MAX))
    bad += [(DUPLICATE, int(at[i]), -1) for i in np.nonzero(twice.any(axis=1))[0]]
    counts["leaves"], counts["keys"] = int(at.size), int(held.sum())
    return bad, counts
