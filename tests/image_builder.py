"""Deterministic page images of tall, thin B-link trees, in numpy.

A tree built by inserts reaches root level 3 only after millions of keys, so
no test built that way ever runs a split above level 2 or a descent deeper
than four pages.  B-link trees have no minimum occupancy: a tree can be tall
with few pages when only the pages on one root-to-leaf path are full.  This
module writes such trees straight into the 1 KB page format (the byte offsets
of sherman_amd/csrc/layout.h, restated below) as images for Tree.load_image
and OracleTree(image=...).  It shares no code with the library or the oracle.

build_tall(): one full page per level on a path down to a full ("hot") leaf,
every other page nearly empty.  A few new keys in the hot leaf split every
level of the path.
build_entry_states(): a small tree whose leaves mix valid entries, deleted
slots, torn entries and entries at version 15.

Every page's front and rear versions are equal and every pointer, fence and
level is sound: the images pass the structural checks of both trees.
"""
import numpy as np

U64 = np.uint64
PAGE = 1024
KEY_MAX = (1 << 64) - 1
MAX_LEVEL = 7

# byte offsets inside a page
OFF_FRONT_VER, OFF_LEFTMOST, OFF_SIBLING, OFF_LEVEL, OFF_LAST_INDEX = 8, 9, 17, 25, 26
OFF_LOWEST, OFF_HIGHEST, OFF_RECORDS = 28, 36, 44
OFF_LEAF_REAR, OFF_INTERNAL_REAR = 1016, 1020
LEAF_SLOTS, LEAF_ENTRY = 54, 18          # {f:4, key, value, r:4}
INTERNAL_SLOTS, INTERNAL_ENTRY = 61, 16  # {key, ptr}

FULL_SEPS = INTERNAL_SLOTS - 1  # a page one separator away from its split
FULL_KEYS = LEAF_SLOTS - 1      # a leaf one key away from its split
HALF_SEPS = 30                  # the root that can absorb a separator
THIN_KEYS = 2
DELETED_EVERY = 17              # every 17th thin leaf holds deleted entries only
VALUE_XOR = 0x1111

PATH_CHILD = {"left": 0.0, "middle": 0.5, "right": 1.0}


def _put64(img, pages, off, vals):
    v = np.ascontiguousarray(np.asarray(vals, dtype=U64).astype("<u8"))
    img[pages, off:off + 8] = v.view(np.uint8).reshape(-1, 8)


def _put_entries(img, pages, slots, keys, vals, ver_f, ver_r):
    """leaf entries {f, key, value, r} at (page, slot) pairs"""
    pages = np.asarray(pages, dtype=np.int64)
    base = OFF_RECORDS + LEAF_ENTRY * np.asarray(slots, dtype=np.int64)
    k = np.ascontiguousarray(np.asarray(keys, dtype=U64).astype("<u8")).view(np.uint8).reshape(-1, 8)
    v = np.ascontiguousarray(np.asarray(vals, dtype=U64).astype("<u8")).view(np.uint8).reshape(-1, 8)
    img[pages, base] = np.asarray(ver_f, dtype=np.uint8) & 0xF
    img[pages, base + 17] = np.asarray(ver_r, dtype=np.uint8) & 0xF
    for b in range(8):
        img[pages, base + 1 + b] = k[:, b]
        img[pages, base + 9 + b] = v[:, b]


def _ga(page, node_id):
    """GlobalAddress {node:16, byte offset:48} of a page index"""
    return (np.asarray(page, dtype=U64) << U64(26)) | U64(node_id)


def _write_levels(kids, leaf_low, page_ver, node_id, rng):
    """The headers, links and separators of a tree given, per level L >= 1,
    the child count of every page in key order (kids[L]; the children of
    consecutive pages are consecutive pages of level L - 1) and the lowest
    fence of every leaf.  Pages get shuffled indices 1..n.  Returns the image
    (page 0 zero) and, per level, the page index, lowest and highest fence of
    every page."""
    top = len(kids)  # kids[0] unused
    counts = [leaf_low.size] + [len(kids[L]) for L in range(1, top)]
    n_pages = sum(counts)
    order = rng.permutation(n_pages) + 1
    img = np.zeros((n_pages + 1, PAGE), dtype=np.uint8)
    page, low, high = [], [], []
    at = 0
    for L, n in enumerate(counts):
        page.append(order[at:at + n].astype(np.int64))
        at += n
    low.append(np.asarray(leaf_low, dtype=U64))
    for L in range(1, top):
        first = np.concatenate([[0], np.cumsum(kids[L])[:-1]]).astype(np.int64)
        assert first[-1] + kids[L][-1] == counts[L - 1]
        low.append(low[L - 1][first])
    for L in range(top):
        high.append(np.concatenate([low[L][1:], np.array([KEY_MAX], dtype=U64)]))
        pg = page[L]
        img[pg, OFF_FRONT_VER] = page_ver
        img[pg, OFF_LEAF_REAR if L == 0 else OFF_INTERNAL_REAR] = page_ver
        img[pg, OFF_LEVEL] = L
        _put64(img, pg, OFF_SIBLING, np.concatenate([_ga(pg[1:], node_id), [U64(0)]]))
        _put64(img, pg, OFF_LOWEST, low[L])
        _put64(img, pg, OFF_HIGHEST, high[L])
        last = np.full(pg.size, -1, dtype="<i2") if L == 0 else \
            (np.asarray(kids[L], dtype="<i2") - np.int16(2))
        img[pg, OFF_LAST_INDEX:OFF_LAST_INDEX + 2] = last.view(np.uint8).reshape(-1, 2)
        if L == 0:
            continue
        first = np.concatenate([[0], np.cumsum(kids[L])[:-1]]).astype(np.int64)
        _put64(img, pg, OFF_LEFTMOST, _ga(page[L - 1][first], node_id))
        for j in range(max(kids[L]) - 1):  # separator j names child j + 1
            has = np.asarray(kids[L]) > j + 1
            c = first[has] + j + 1
            _put64(img, pg[has], OFF_RECORDS + INTERNAL_ENTRY * j, low[L - 1][c])
            _put64(img, pg[has], OFF_RECORDS + INTERNAL_ENTRY * j + 8,
                   _ga(page[L - 1][c], node_id))
    return img, page, low, high


def build_tall(root_level, path, root_full, seed=0, page_ver=1, entry_ver=1, node_id=0):
    """A tree of root level `root_level` (1..7) with one full page per level.

    The path page of level L >= 1 has 60 separators; its path child is child
    0, 30 or 60 (path = "left", "middle", "right"); the path leaf (the hot
    leaf) has 53 valid entries in shuffled slots.  With root_full False the
    root has 30 separators instead (path child 0, 15 or 30).  Every other
    internal page has one separator and every other leaf two entries in two
    random slots; every 17th of those leaves has both deleted (value 0, the
    key bytes left in place).  Key i (in leaf order, deleted ones counted) is
    (i + 1) * step with step = 2^64 // (n + 2) cut to a multiple of 64; the
    value is key ^ 0x1111; a leaf's lowest fence is its first key (0 for the
    first leaf).  A full root at level 7 could not grow and is refused.

    Returns (image, root_ptr, info): the image as a flat uint8 array whose
    page 0 is zero, and info = {"keys", "vals": the valid pairs sorted by
    key; "deleted": the deleted keys; "hot_lo", "hot_hi", "hot_page": the hot
    leaf; "path": {level: (page, lowest, highest)} of the path page of every
    level 0..root_level; "leaves", "internal", "n_keys": what a structural
    check counts; "root_level", "step"}."""
    if not 1 <= root_level <= MAX_LEVEL:
        raise ValueError("root_level out of 1..7")
    if root_full and root_level == MAX_LEVEL:
        raise ValueError("a full root at level 7 cannot grow")
    rng = np.random.default_rng([seed, root_level, int(root_full),
                                 sorted(PATH_CHILD).index(path)])
    # per level, top down: the kind of every page in key order
    kinds = {root_level: ["path" if root_full else "half"]}
    kids = {}
    for L in range(root_level, 0, -1):
        below, n_kids = [], []
        for kind in kinds[L]:
            if kind == "thin":
                n, hot = 2, -1
            else:
                n = (FULL_SEPS if kind == "path" else HALF_SEPS) + 1
                hot = int(round(PATH_CHILD[path] * (n - 1)))
            n_kids.append(n)
            below += ["path" if c == hot else "thin" for c in range(n)]
        kids[L], kinds[L - 1] = n_kids, below
    leaf_kind = np.array([k == "path" for k in kinds[0]])
    assert leaf_kind.sum() == 1
    per_leaf = np.where(leaf_kind, FULL_KEYS, THIN_KEYS)
    n_pos = int(per_leaf.sum())
    step = ((1 << 64) // (n_pos + 2)) & ~63
    keys = (np.arange(n_pos, dtype=U64) + U64(1)) * U64(step)
    vals = keys ^ U64(VALUE_XOR)
    first = np.concatenate([[0], np.cumsum(per_leaf)[:-1]]).astype(np.int64)
    leaf_low = keys[first].copy()
    leaf_low[0] = 0
    img, page, low, high = _write_levels([None] + [kids[L] for L in range(1, root_level + 1)],
                                         leaf_low, page_ver, node_id, rng)
    # the entries: which leaf, which slot, deleted or not
    leaf_of = np.repeat(np.arange(per_leaf.size), per_leaf)
    slot = np.empty(n_pos, dtype=np.int64)
    thin_rank = np.cumsum(~leaf_kind) - 1  # the how-manyth thin leaf
    dead_leaf = ~leaf_kind & (thin_rank % DELETED_EVERY == DELETED_EVERY - 1)
    for i in range(per_leaf.size):
        slot[first[i]:first[i] + per_leaf[i]] = rng.permutation(LEAF_SLOTS)[:per_leaf[i]]
    dead = dead_leaf[leaf_of]
    _put_entries(img, page[0][leaf_of], slot, keys, np.where(dead, U64(0), vals),
                 entry_ver, entry_ver)
    hot = int(np.nonzero(leaf_kind)[0][0])
    on_path = {0: hot}
    for L in range(1, root_level + 1):  # the parent of the path page below
        on_path[L] = int(np.searchsorted(np.cumsum(kids[L]), on_path[L - 1], side="right"))
    info = {
        "keys": keys[~dead], "vals": vals[~dead], "deleted": keys[dead],
        "hot_lo": int(low[0][hot]), "hot_hi": int(high[0][hot]), "hot_page": int(page[0][hot]),
        "path": {L: (int(page[L][i]), int(low[L][i]), int(high[L][i]))
                 for L, i in on_path.items()},
        "leaf_lo": low[0], "leaf_live": np.bincount(leaf_of[~dead], minlength=per_leaf.size),
        "leaves": int(per_leaf.size),
        "internal": int(sum(len(kids[L]) for L in kids)),
        "n_keys": int((~dead).sum()), "root_level": root_level, "step": step,
    }
    assert on_path[root_level] == 0
    root_ptr = int(_ga(page[root_level][0], node_id))
    return img.reshape(-1), root_ptr, info


# slot kinds of build_entry_states
VALID, DELETED, STALE_COPY, TORN, VALID15 = "valid", "deleted", "stale_copy", "torn", "valid15"


def build_entry_states(seed=0, page_ver=1, node_id=0):
    """A tree of root level 2 with 40 leaves (5 level-1 pages of 8 leaves).

    Every leaf has 6 to 20 valid entries in random slots.  Every third leaf
    also has deleted slots (value 0): some with the stale bytes of a key
    stored nowhere, and two with a stale copy of a key that is valid in
    another slot of the same leaf, one in a lower and one in a higher slot
    than the live entry.  Leaves 1, 10, 19, 28, 37 also hold torn entries
    (value != 0, f and r differing in the low nibble) of keys stored nowhere
    else, and in leaves 4, 13, 22, 31 every valid entry has f = r = 15.  The
    last leaf is full of deleted slots and holds no valid entry.

    Returns (image, root_ptr, info): info["slots"] = {"page", "slot", "key",
    "value", "kind"} arrays naming every written slot; "keys" / "vals" the
    valid pairs sorted by key; "torn", "deleted" (keys stored nowhere as valid)
    and "stale_copy" key arrays; "torn_pages", "v15_pages"; "v15_keys";
    "leaves", "internal", "n_valid", "n_torn"."""
    rng = np.random.default_rng([seed, 0xE5])
    n_leaves, fan = 40, 8
    torn_leaves = set(range(1, n_leaves, 9))
    v15_leaves = set(range(4, n_leaves, 9))
    # 40 leaves tile 2^64 unevenly: the last one takes the rest
    at = np.arange(n_leaves, dtype=U64)
    leaf_low = at * U64(1 << 58) + at * at * U64(1 << 50)
    kids = [None, [fan] * (n_leaves // fan), [n_leaves // fan]]
    img, page, low, high = _write_levels(kids, leaf_low, page_ver, node_id, rng)
    rows = []  # (page, slot, key, value, kind, f, r)
    for i in range(n_leaves):
        lo = max(int(low[0][i]), 64)
        hi = min(int(high[0][i]), lo + (1 << 57))
        pg = int(page[0][i])
        slots = [int(s) for s in rng.permutation(LEAF_SLOTS)]
        # distinct keys inside the fences, 64 apart at least
        draws = np.unique(rng.integers(0, (hi - lo) // 64 - 1, 80))
        assert draws.size >= 60
        pool = [lo + 64 * int(x) for x in rng.permutation(draws)[:60]]
        if i == n_leaves - 1:
            for s in slots[:FULL_KEYS + 1]:
                rows.append((pg, s, pool.pop(), 0, DELETED, 3, 3))
            continue
        n_valid = int(rng.integers(6, 21))
        live = []
        for _ in range(n_valid):
            k = pool.pop()
            if i in v15_leaves:
                rows.append((pg, slots.pop(), k, k ^ VALUE_XOR, VALID15, 15, 15))
            else:
                f = int(rng.integers(0, 16))
                rows.append((pg, slots.pop(), k, k ^ VALUE_XOR, VALID, f, f))
            live.append(rows[-1])
        if i % 3 == 1:
            for _ in range(4):
                f = int(rng.integers(0, 16))
                rows.append((pg, slots.pop(), pool.pop(), 0, DELETED, f, f))
            # a stale copy below and one above its live slot
            a, b = live[0], live[1]
            for src, side in ((a, -1), (b, 1)):
                free = [s for s in slots if (s - src[1]) * side > 0]
                if free:
                    slots.remove(free[0])
                    rows.append((pg, free[0], src[2], 0, STALE_COPY, 7, 7))
        if i in torn_leaves:
            for j in range(5):
                k = pool.pop()
                f = int(rng.integers(0, 16))
                r = (f + 1 + j * 3) & 0xF  # differs from f in the low nibble
                rows.append((pg, slots.pop(), k, k ^ 0x2222, TORN, f, r))
    pg, sl, k, v, kind, f, r = zip(*rows)
    pg, sl, f, r = (np.array(c, dtype=np.int64) for c in (pg, sl, f, r))
    k, v, kind = np.array(k, dtype=U64), np.array(v, dtype=U64), np.array(kind)
    assert np.all((f[kind == TORN] ^ r[kind == TORN]) & 0xF)
    _put_entries(img, pg, sl, k, v, f, r)
    ok = (kind == VALID) | (kind == VALID15)
    o = np.argsort(k[ok])
    copies = k[kind == STALE_COPY]
    assert copies.size >= 4 and np.isin(copies, k[ok]).all()
    info = {
        "slots": {"page": pg, "slot": sl, "key": k, "value": v, "kind": kind},
        "keys": k[ok][o], "vals": v[ok][o],
        "torn": np.sort(k[kind == TORN]), "deleted": np.sort(k[kind == DELETED]),
        "stale_copy": np.sort(copies),
        "torn_pages": sorted(int(page[0][i]) for i in torn_leaves),
        "v15_pages": sorted(int(page[0][i]) for i in v15_leaves),
        "v15_keys": np.sort(k[kind == VALID15]),
        "leaf_lo": low[0],
        "leaves": n_leaves, "internal": len(kids[1]) + 1,
        "n_valid": int(ok.sum()), "n_torn": int((kind == TORN).sum()), "root_level": 2,
    }
    return img.reshape(-1), int(_ga(page[2][0], node_id)), info
