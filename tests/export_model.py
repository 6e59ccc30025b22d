"""Host model of the sorted export (shm_export) over a page IMAGE, in numpy
and plain Python, sharing no code with the library: the byte offsets of
sherman_amd/csrc/layout.h are restated below.

export(image, root_ptr, lo, hi): descend from the root to the leaf of `lo`
(the leftmost child, then every separator <= lo one child further; a right
turn to the sibling while lo >= the page's highest fence), then follow the
leaf siblings while the last leaf's highest fence is <= hi.  Of every leaf
keep the entries with value != 0 and equal version nibbles, sort them by
key, cut to [lo, hi], append.  The appended run must ascend: the leaf order is
the key order.  This is Tree::range_query's traversal, which follows the
sibling chain and so reads the leaves a missing separator hides from their
parent.
"""
import numpy as np

U64 = np.uint64
PAGE = 1024
KEY_MAX = (1 << 64) - 1

OFF_LEFTMOST, OFF_SIBLING, OFF_LEVEL, OFF_LAST_INDEX = 9, 17, 25, 26
OFF_LOWEST, OFF_HIGHEST, OFF_RECORDS = 28, 36, 44
LEAF_SLOTS, LEAF_ENTRY, INTERNAL_ENTRY = 54, 18, 16


def _u64(img, at):
    return int.from_bytes(bytes(img[at:at + 8]), "little")


def _page(ga, node_id, n_pages):
    """byte offset of the page a GlobalAddress {node:16, offset:48} names"""
    off = ga >> 16
    assert ga != 0 and (ga & 0xFFFF) == node_id and off % PAGE == 0, hex(ga)
    assert PAGE <= off < n_pages * PAGE, hex(ga)
    return off


def leaf_pairs(img, at):
    """the valid pairs of the leaf at byte offset `at`, sorted by key"""
    e = np.asarray(img[at + OFF_RECORDS:at + OFF_RECORDS + LEAF_SLOTS * LEAF_ENTRY],
                   dtype=np.uint8).reshape(LEAF_SLOTS, LEAF_ENTRY)
    keys = np.ascontiguousarray(e[:, 1:9]).view("<u8").reshape(-1).astype(U64)
    vals = np.ascontiguousarray(e[:, 9:17]).view("<u8").reshape(-1).astype(U64)
    ok = (vals != 0) & (((e[:, 0] ^ e[:, 17]) & 0xF) == 0)
    o = np.argsort(keys[ok], kind="stable")
    return keys[ok][o], vals[ok][o]


def export(image, root_ptr, lo=0, hi=KEY_MAX, node_id=0):
    """(keys, vals) uint64 arrays: every valid pair with lo <= key <= hi in
    ascending key order, by the walk above."""
    img = np.asarray(image, dtype=np.uint8).reshape(-1)
    n_pages = img.size // PAGE
    none = np.zeros(0, dtype=U64)
    if lo > hi or lo == KEY_MAX:
        return none, none.copy()
    at = _page(root_ptr, node_id, n_pages)
    for _ in range(n_pages + 8):  # the descent: bounded by the pages
        highest, sibling = _u64(img, at + OFF_HIGHEST), _u64(img, at + OFF_SIBLING)
        leftmost = _u64(img, at + OFF_LEFTMOST)
        if lo >= highest and sibling:
            at = _page(sibling, node_id, n_pages)
            continue
        if leftmost == 0:
            break
        assert img[at + OFF_LEVEL] > 0
        last = int.from_bytes(bytes(img[at + OFF_LAST_INDEX:at + OFF_LAST_INDEX + 2]), "little",
                              signed=True)
        child = leftmost
        for j in range(last + 1):
            if _u64(img, at + OFF_RECORDS + INTERNAL_ENTRY * j) <= lo:
                child = _u64(img, at + OFF_RECORDS + INTERNAL_ENTRY * j + 8)
        at = _page(child, node_id, n_pages)
    else:
        raise AssertionError("the descent did not end")
    ks, vs, seen = [], [], 0
    while True:
        seen += 1
        assert seen <= n_pages, "the leaf chain does not end"
        assert img[at + OFF_LEVEL] == 0 and _u64(img, at + OFF_LEFTMOST) == 0
        k, v = leaf_pairs(img, at)
        cut = (k >= U64(lo)) & (k <= U64(hi))
        ks.append(k[cut])
        vs.append(v[cut])
        highest, sibling = _u64(img, at + OFF_HIGHEST), _u64(img, at + OFF_SIBLING)
        if not sibling or highest > hi:
            break
        at = _page(sibling, node_id, n_pages)
    keys, vals = np.concatenate(ks), np.concatenate(vs)
    assert keys.size < 2 or (keys[1:] > keys[:-1]).all(), "the leaf order is not the key order"
    return keys, vals


def drop_last_separators(image, root_ptr, node_id=0, in_root=True, in_level1=True):
    """A copy of a level-2 image (build_entry_states) with the root's
    last_index decremented (in_root) and every level-1 page's (in_level1): the
    last child of each such page is then reachable through its left sibling
    alone, the B-link state a missing separator leaves."""
    img = np.array(image, dtype=np.uint8).reshape(-1).copy()
    n_pages = img.size // PAGE

    def dec(at):
        last = int.from_bytes(bytes(img[at + OFF_LAST_INDEX:at + OFF_LAST_INDEX + 2]), "little",
                              signed=True)
        assert last >= 1
        img[at + OFF_LAST_INDEX:at + OFF_LAST_INDEX + 2] = np.frombuffer(
            (last - 1).to_bytes(2, "little", signed=True), dtype=np.uint8)

    root = _page(root_ptr, node_id, n_pages)
    assert img[root + OFF_LEVEL] == 2
    at = _page(_u64(img, root + OFF_LEFTMOST), node_id, n_pages)
    level1 = []
    while True:
        assert img[at + OFF_LEVEL] == 1
        level1.append(at)
        sib = _u64(img, at + OFF_SIBLING)
        if not sib:
            break
        at = _page(sib, node_id, n_pages)
    for at in (level1 if in_level1 else []) + ([root] if in_root else []):
        dec(at)
    return img
