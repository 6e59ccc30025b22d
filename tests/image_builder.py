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


# ---- soil: pages the tree does not reach -------------------------------------------
# slot kinds of soil_pages
ABSENT, SHADOW, OUTSIDE, NULL = "absent", "shadow", "outside", "null"
SOIL_KINDS = (ABSENT, SHADOW, DELETED, OUTSIDE, TORN, NULL)
SOIL_XOR = 0x5011  # a soil entry's value is key ^ SOIL_XOR: never the tree's key ^ VALUE_XOR


def soil_pages(n, keys_by_kind, seed, node_id=0, first_page=1, page_ver=1):
    """n pages that look like current pages of a tree and are linked from
    nowhere: what a page sweep over [1, next_page) meets below next_page after
    a failed take, a shrinking reload or a load of such an image.

    keys_by_kind maps a kind to its keys (a kind left out has none):
      "absent"   valid entries (f == r, value != 0) of keys the tree never held
      "shadow"   valid entries of keys the tree holds, with another value
      "deleted"  valid entries of keys the tree holds as deleted slots
      "outside"  valid entries of keys outside the tree's key range hint
      "torn"     entries with a value whose f and r differ in the low nibble
      "null"     entries with value 0
    A valid or torn entry's value is key ^ SOIL_XOR.  With n >= 2 page 0 of the
    soil looks internal: level 1, a leftmost pointer and (key, pointer) records
    of the valid keys, pointing at the soil's leaves as if the soil were
    appended at page `first_page`; read as a leaf its slots would hold valid
    entries, and only its level and leftmost say it is none.  Every other page
    is a leaf to a sweep: level 0, leftmost 0, front == rear version, sibling 0,
    fences around its own keys, last_index -1 as the other builders write it.
    The entries are dealt over the leaves in turn, into random slots.

    Returns (pages, info): pages (n, 1024) uint8; info["slots"] = {"page" (the
    index into pages), "slot", "key", "value", "kind"} of every leaf entry,
    info[kind] the sorted keys of each kind, "leaf_pages" / "internal_pages"
    the indices into pages."""
    rng = np.random.default_rng([seed, 0x5011, n])
    unknown = set(keys_by_kind) - set(SOIL_KINDS)
    if unknown:
        raise ValueError(f"unknown soil kinds {sorted(unknown)}")
    pages = np.zeros((n, PAGE), dtype=np.uint8)
    internal = [0] if n >= 2 else []
    leaves = np.array([p for p in range(n) if p not in internal], dtype=np.int64)
    kinds = [k for k in SOIL_KINDS if len(keys_by_kind.get(k, ()))]
    key = np.concatenate([np.asarray(keys_by_kind[k], dtype=U64) for k in kinds] or
                         [np.zeros(0, dtype=U64)])
    kind = np.concatenate([np.full(len(keys_by_kind[k]), k) for k in kinds] or
                          [np.zeros(0, dtype="<U8")])
    if key.size > leaves.size * LEAF_SLOTS:
        raise ValueError("more soil entries than slots")
    if np.any(key == U64(0)) or np.any(key == U64(KEY_MAX)) or np.any(key == U64(SOIL_XOR)):
        raise ValueError("a soil key a valid entry cannot hold")
    o = rng.permutation(key.size)  # the kinds mixed over the pages
    key, kind = key[o], kind[o]
    pg = leaves[np.arange(key.size) % leaves.size] if key.size else np.zeros(0, dtype=np.int64)
    slot = np.empty(key.size, dtype=np.int64)
    for p in leaves:
        mine = np.nonzero(pg == p)[0]
        slot[mine] = rng.permutation(LEAF_SLOTS)[:mine.size]
    value = np.where(kind == NULL, U64(0), key ^ U64(SOIL_XOR))
    f = rng.integers(0, 16, key.size)
    r = np.where(kind == TORN, (f + 1 + rng.integers(0, 14, key.size)) & 0xF, f)
    assert np.all(((f ^ r) & 0xF != 0) == (kind == TORN))
    _put_entries(pages, pg, slot, key, value, f, r)
    pages[leaves, OFF_FRONT_VER] = page_ver
    pages[leaves, OFF_LEAF_REAR] = page_ver
    pages[leaves, OFF_LEVEL] = 0
    pages[leaves, OFF_LAST_INDEX:OFF_LAST_INDEX + 2] = np.array([-1], dtype="<i2").view(np.uint8)
    for p in leaves:
        mine = key[pg == p]
        lo, hi = (int(mine.min()), int(mine.max()) + 1) if mine.size else (64, 128)
        _put64(pages, [p], OFF_LOWEST, [lo])
        _put64(pages, [p], OFF_HIGHEST, [hi])
    for p in internal:
        valid = np.sort(key[(kind != TORN) & (kind != NULL)])[:INTERNAL_SLOTS - 1]
        if valid.size == 0:
            valid = np.array([64], dtype=U64)
        pages[p, OFF_FRONT_VER] = page_ver
        pages[p, OFF_INTERNAL_REAR] = page_ver
        pages[p, OFF_LEVEL] = 1
        pages[p, OFF_LAST_INDEX:OFF_LAST_INDEX + 2] = \
            np.array([valid.size - 1], dtype="<i2").view(np.uint8)
        _put64(pages, [p], OFF_LEFTMOST, _ga([first_page + int(leaves[0])], node_id))
        _put64(pages, [p], OFF_LOWEST, [0])
        _put64(pages, [p], OFF_HIGHEST, [KEY_MAX])
        to = first_page + leaves[np.arange(valid.size) % leaves.size]
        for j in range(valid.size):
            _put64(pages, [p], OFF_RECORDS + INTERNAL_ENTRY * j, [valid[j]])
            _put64(pages, [p], OFF_RECORDS + INTERNAL_ENTRY * j + 8, _ga([to[j]], node_id))
    info = {"slots": {"page": pg, "slot": slot, "key": key, "value": value, "kind": kind},
            "leaf_pages": leaves, "internal_pages": np.array(internal, dtype=np.int64)}
    for k in SOIL_KINDS:
        info[k] = np.sort(key[kind == k])
    return pages, info


def with_soil(img, pages):
    """the image with the soil pages appended (the root pointer stays)"""
    img = np.asarray(img, dtype=np.uint8).reshape(-1)
    assert img.size % PAGE == 0
    return np.concatenate([img, np.asarray(pages, dtype=np.uint8).reshape(-1)])


def soil_sizes(n):
    """(keys per valid kind, keys per torn / null kind) that fill the leaves
    of n soil pages: at most 32 and 16, and 17 and 1 for a single leaf"""
    slots = LEAF_SLOTS * max(n - 1, 1)
    per_kind = min(32, (slots - 2) // 3)
    return per_kind, min(16, (slots - 3 * per_kind) // 2)


def soil_keys(info, per_kind=32, per_bad=16, hint=(0, 64)):
    """Soil keys for an image of this module, by kind, from its info: shadow
    keys are stored keys outside the hot leaf (every leaf of these images but
    the hot one is thin against a bucket of the key-value table: a few keys
    in a span of 2^55 and more), absent / torn / null keys lie 8, 40 and 48
    above other stored keys (every key the builders write, valid or not, is a
    multiple of 64 above a fence that is one), deleted keys come from
    info["deleted"], and outside keys lie 56 above stored keys outside the key
    range hint (lo, bits); none with the full range."""
    k = np.asarray(info["keys"], dtype=U64)
    if "hot_lo" in info:
        k = k[(k < U64(info["hot_lo"])) | (k >= U64(info["hot_hi"]))]

    def spread(a, m):
        a = np.asarray(a, dtype=U64)
        return a[np.unique(np.linspace(0, a.size - 1, min(m, a.size)).astype(np.int64))]

    lo, bits = hint

    def inside(a):
        a = np.asarray(a, dtype=U64)
        if bits >= 64:
            return np.ones(a.size, dtype=bool)
        return (a >= U64(lo)) & (a - U64(lo) < U64(1 << bits))

    kin, kout = k[inside(k)], k[~inside(k)]
    dele = np.asarray(info["deleted"], dtype=U64)
    out = {SHADOW: spread(kin[0::3], per_kind), ABSENT: spread(kin[1::3], per_kind) + U64(8),
           TORN: spread(kin[2::3], per_bad) + U64(40),
           NULL: spread(kin[2::3], per_bad) + U64(48),
           DELETED: spread(dele[inside(dele)], per_kind),
           OUTSIDE: spread(kout, per_kind) + U64(56)}
    return out


# ---- what a page sweep takes, and what the tree reaches ------------------------------
def sweep_leaf(pages):
    """the sweepers' leaf test on (n, 1024) uint8 pages: level byte 0 and no
    leftmost pointer"""
    leftmost = np.ascontiguousarray(pages[:, OFF_LEFTMOST:OFF_LEFTMOST + 8]).view("<u8").ravel()
    return (pages[:, OFF_LEVEL] == 0) & (leftmost == 0)


def sweep_entries(pages):
    """(page, slot, key, value) of every entry a sweep would take from the
    pages: the valid entries (value != 0, f == r in the low nibble) of the
    pages sweep_leaf accepts"""
    rec = pages[:, OFF_RECORDS:OFF_RECORDS + LEAF_SLOTS * LEAF_ENTRY]
    rec = rec.reshape(-1, LEAF_SLOTS, LEAF_ENTRY)
    k = np.ascontiguousarray(rec[:, :, 1:9]).view("<u8").reshape(-1, LEAF_SLOTS)
    v = np.ascontiguousarray(rec[:, :, 9:17]).view("<u8").reshape(-1, LEAF_SLOTS)
    ok = (v != 0) & (((rec[:, :, 0] ^ rec[:, :, 17]) & 0xF) == 0) & sweep_leaf(pages)[:, None]
    pg, sl = np.nonzero(ok)
    return pg, sl, k[pg, sl], v[pg, sl]


def reached_pages(img, root_ptr):
    """Mask over the image's pages: the pages reached from the root through
    the leftmost pointer and the records of internal pages and the sibling
    pointer of every page (a page that hangs on its left sibling alone is
    reached, as for every reader)."""
    pg = np.asarray(img, dtype=np.uint8).reshape(-1, PAGE)

    def f64(p, off):
        return int(np.ascontiguousarray(pg[p, off:off + 8]).view("<u8")[0])

    seen = np.zeros(pg.shape[0], dtype=bool)
    todo = [int(root_ptr) >> 26]
    while todo:
        p = todo.pop()
        if not 0 < p < pg.shape[0] or seen[p]:
            continue
        seen[p] = True
        todo.append(f64(p, OFF_SIBLING) >> 26)
        if f64(p, OFF_LEFTMOST):
            todo.append(f64(p, OFF_LEFTMOST) >> 26)
            last = int(np.ascontiguousarray(pg[p, OFF_LAST_INDEX:OFF_LAST_INDEX + 2]).view("<i2")[0])
            for j in range(min(max(last + 1, 0), INTERNAL_SLOTS)):
                todo.append(f64(p, OFF_RECORDS + INTERNAL_ENTRY * j + 8) >> 26)
    return seen
