"""The bulk loader's tree in numpy: the plan and the exact page bytes.

A second statement of the rules in include/sherman_amd.h (shm_bulk_plan,
shm_bulk_load), sharing no code with the library: the byte offsets of
sherman_amd/csrc/layout.h are restated below.

plan(n, lf, inf): P0 = ceil(n / lf) leaves (one empty leaf for n == 0),
ceil(P / (inf + 1)) pages on each level above, the first level with one page
the root.  Every level deals the C items below it (pairs for leaves, children
above) over its P pages evenly: q = C // P, r = C % P, page p takes items
[p q + min(p, r), (p + 1) q + min(p + 1, r)).

build(): the root is page 1; below a root that is not a leaf, level 0 sits at
pages 2 .. 2 + P0 - 1 in key order, then level 1, and so on.  Every page: lock
word 0, front == rear version 1, sibling = the next page of the level (0 for
the last), lowest = the first key under the page (0 for a level's first page),
highest = the next page's lowest (KEY_MAX for the last).  A leaf: last_index
-1, entries {f = 1, key, value, r = 1} in slots 0 .. cnt - 1 in key order.  An
internal page: leftmost = child 0, record j = (lowest of child j + 1, its
address), last_index = children - 2.  Every other byte is 0.
"""
import numpy as np

U64 = np.uint64
PAGE = 1024
KEY_MAX = (1 << 64) - 1
MAX_LEVEL = 7
DEFAULT_LEAF_FILL, DEFAULT_INTERNAL_FILL = 36, 40
MAX_LEAF_FILL, MAX_INTERNAL_FILL = 53, 60

OFF_FRONT_VER, OFF_LEFTMOST, OFF_SIBLING, OFF_LEVEL, OFF_LAST_INDEX = 8, 9, 17, 25, 26
OFF_LOWEST, OFF_HIGHEST, OFF_RECORDS = 28, 36, 44
OFF_LEAF_REAR, OFF_INTERNAL_REAR = 1016, 1020
LEAF_ENTRY, INTERNAL_ENTRY = 18, 16


def fills(lf, inf):
    lf = lf or DEFAULT_LEAF_FILL
    inf = inf or DEFAULT_INTERNAL_FILL
    if not (1 <= lf <= MAX_LEAF_FILL and 2 <= inf <= MAX_INTERNAL_FILL):
        raise ValueError("fill out of range")
    return lf, inf


def plan(n, lf=0, inf=0):
    """{"pages", "root_level", "level_pages"}; ValueError for fills out of
    range or a root above level 7."""
    lf, inf = fills(lf, inf)
    level_pages = [max(1, -(-n // lf))]
    while level_pages[-1] > 1:
        level_pages.append(-(-level_pages[-1] // (inf + 1)))
    if len(level_pages) - 1 > MAX_LEVEL:
        raise ValueError("tree too tall")
    return {"pages": sum(level_pages), "root_level": len(level_pages) - 1,
            "level_pages": level_pages}


def deal(items, pages):
    """first item of every page, and one past the last page's: pages + 1 starts"""
    q, r = divmod(items, pages)
    p = np.arange(pages + 1, dtype=np.int64)
    return p * q + np.minimum(p, r)


def _put64(img, pages, off, vals):
    v = np.ascontiguousarray(np.asarray(vals, dtype=U64).astype("<u8"))
    img[pages, off:off + 8] = v.view(np.uint8).reshape(-1, 8)


def _ga(page, node_id):
    return (np.asarray(page, dtype=U64) << U64(26)) | U64(node_id)


def build(keys, vals, lf=0, inf=0, node_id=0):
    """(image, root_ptr, plan): the image as a flat uint8 array of plan.pages
    + 1 pages whose page 0 is zero."""
    keys = np.asarray(keys, dtype=U64)
    vals = np.asarray(vals, dtype=U64)
    n = keys.size
    assert vals.size == n and (n < 2 or (keys[1:] > keys[:-1]).all())
    pl = plan(n, lf, inf)
    top = pl["root_level"]
    counts = pl["level_pages"]
    img = np.zeros((pl["pages"] + 1, PAGE), dtype=np.uint8)
    # page indices per level: the root at 1, the levels below it from 2 on
    page, at = [], 2
    for L, c in enumerate(counts):
        if L == top:
            page.append(np.array([1], dtype=np.int64))
        else:
            page.append(np.arange(at, at + c, dtype=np.int64))
            at += c
    assert at == pl["pages"] + 1 or top == 0
    low = None
    for L, c in enumerate(counts):
        pg = page[L]
        first = deal(n if L == 0 else counts[L - 1], c)
        if L == 0:
            low_here = keys[first[:-1]] if n else np.zeros(1, dtype=U64)
        else:
            low_here = low[first[:-1]]
        low_here = low_here.copy()
        low_here[0] = 0
        high = np.concatenate([low_here[1:], np.array([KEY_MAX], dtype=U64)])
        img[pg, OFF_FRONT_VER] = 1
        img[pg, OFF_LEAF_REAR if L == 0 else OFF_INTERNAL_REAR] = 1
        img[pg, OFF_LEVEL] = L
        _put64(img, pg, OFF_SIBLING, np.concatenate([_ga(pg[1:], node_id), [U64(0)]]))
        _put64(img, pg, OFF_LOWEST, low_here)
        _put64(img, pg, OFF_HIGHEST, high)
        cnt = np.diff(first)
        last = np.full(c, -1, dtype="<i2") if L == 0 else (cnt - 2).astype("<i2")
        img[pg, OFF_LAST_INDEX:OFF_LAST_INDEX + 2] = last.view(np.uint8).reshape(-1, 2)
        if L == 0:
            if n:
                leaf_of = np.repeat(np.arange(c), cnt)
                slot = np.arange(n) - first[leaf_of]
                base = OFF_RECORDS + LEAF_ENTRY * slot
                kb = np.ascontiguousarray(keys.astype("<u8")).view(np.uint8).reshape(-1, 8)
                vb = np.ascontiguousarray(vals.astype("<u8")).view(np.uint8).reshape(-1, 8)
                img[pg[leaf_of], base] = 1
                img[pg[leaf_of], base + 17] = 1
                for b in range(8):
                    img[pg[leaf_of], base + 1 + b] = kb[:, b]
                    img[pg[leaf_of], base + 9 + b] = vb[:, b]
        else:
            kid = page[L - 1]
            _put64(img, pg, OFF_LEFTMOST, _ga(kid[first[:-1]], node_id))
            for j in range(int(cnt.max()) - 1):  # record j names child j + 1
                has = cnt > j + 1
                ch = first[:-1][has] + j + 1
                _put64(img, pg[has], OFF_RECORDS + INTERNAL_ENTRY * j, low[ch])
                _put64(img, pg[has], OFF_RECORDS + INTERNAL_ENTRY * j + 8, _ga(kid[ch], node_id))
        low = low_here
    return img.reshape(-1), int(_ga(1, node_id)), pl


def counts(pl, n):
    """what a structural check counts on the plan's tree"""
    return {"leaves": pl["level_pages"][0], "internal": pl["pages"] - pl["level_pages"][0],
            "keys": n}


# the issue's shapes (n, leaf_fill, internal_fill)
SHAPES = [(0, 0, 0), (1, 0, 0), (53, 53, 60), (54, 53, 60), (53 * 61, 53, 60),
          (53 * 61 + 1, 53, 60), (2187, 1, 2), (1000, 1, 2), (5000, 0, 0)]


def shape_keys(n, kind, seed=0):
    """n ascending keys: "spread" over the whole u64 range on both sides of
    2^63, "dense" 1..n, "ends" spread and including key 0 and KEY_MAX - 1."""
    if kind == "dense":
        return np.arange(1, n + 1, dtype=U64)
    rng = np.random.default_rng([seed, n])
    k = np.unique(rng.integers(1, KEY_MAX - 1, n + n // 8 + 16, dtype=np.uint64))
    k = k[rng.permutation(k.size)[:n]]
    if kind == "ends" and n >= 2:
        k[0], k[1] = 0, KEY_MAX - 1
    k = np.sort(k)
    assert k.size == n and np.unique(k).size == n
    return k


def shape_kind(n, lf, inf):
    """which key set a shape gets: one dense, one with both ends, the rest spread"""
    if (n, lf, inf) == (54, 53, 60):
        return "dense"
    if (n, lf, inf) == (1000, 1, 2):
        return "ends"
    return "spread"


def shape_vals(keys):
    return (keys * U64(0x9E3779B97F4A7C15)) | U64(1)
