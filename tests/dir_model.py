"""A host-side reference for the leaf directory, in numpy.

The batched get and the insert path's locate trust a directory entry for
results (an exact directory answers "absent" from a usable entry, and a
value-form entry answers the get from its inline copy), and the only other
check of the entries, shm__dir_verify, is device code that shares
dir_exact_entry() with the repair that writes them.  This module shares
nothing with the library: it restates the documented formats (layout.h, the
head of leafdir.hip) as constants of its own and checks a raw dump of the
directory (Tree.dir_dump()) against a raw dump of the pages
(Tree.dump_image()).

What an entry claims, by form (u32 words w[0..15] of the 64 B entry, count
word cw = w[7]: leaf count in bits 0..7, flags, pair count in bits 16..23):

  pair form, usable: PAIRS set, PAIRS_BAD clear, pair count np <= 16.  The
    leaf list w[0..nl) names, in key order, the leaves that cover the prefix;
    split point t_i = w[3 + i] = (lowest fence of leaf i - first key of the
    prefix) >> max(shift - 32, 0).  The u16 pairs at bytes 32.. are
    fp | slot << 8 | leaf << 14.  Every valid key of the prefix has its pair
    among the first np (more pairs, those of deleted keys, are allowed).
    With VALS set the bytes of pairs 8..15 hold an inline entry: np <= 8.
  value form, usable: VALS | PAIRS set, PAIRS_BAD and FIX clear, np <= 2,
    nl <= 2.  The prefix holds exactly np valid keys, pair q's (key, value)
    inline: q = 0 key in w[2..3], value in w[5..6]; q = 1 key in w[12..13],
    value in w[14..15].
  fingerprint form: FP set.  One leaf, w[0], holds every valid key of the
    prefix, and the byte at 4 + s (s < 24) or 8 + s is key_fp of slot s's key.

Any other entry makes no claim and is not checked.
"""
import numpy as np

U64 = np.uint64
U32 = np.uint32

# the page (Sherman's packed layout): 1 KB, header fields by byte offset
PAGE = 1024
OFF_LEFTMOST, OFF_SIBLING, OFF_LEVEL = 9, 17, 25
OFF_LOWEST, OFF_HIGHEST, OFF_RECORDS = 28, 36, 44
LEAF_SLOTS, LEAF_ENTRY = 54, 18  # {f, key[8], value[8], r}
KEY_MAX = (1 << 64) - 1

# the directory entry's count word
FP, PAIRS, PAIRS_BAD, FIX, VALS = 0x100, 0x200, 0x400, 0x800, 0x1000
PAIR_MAX, VAL_MAX, LIST_MAX = 16, 2, 4

_M64 = (1 << 64) - 1


def key_fp(k):
    """the 8-bit fingerprint of a key (array of uint64): the top byte of
    k * 0x9E3779B97F4A7C15 mod 2^64, with 0 mapped to 1"""
    k = np.asarray(k, dtype=U64)
    with np.errstate(over="ignore"):
        f = ((k * U64(0x9E3779B97F4A7C15)) >> U64(56)).astype(U32)
    return np.where(f == 0, U32(1), f).astype(U32)


def page_of(ga):
    """page index of a GlobalAddress {node:16, byte offset:48}"""
    return int(ga) >> 26


class Image:
    """The reachable leaves of a page image and their valid entries.

    leaves: page index, lowest, highest of every leaf on the sibling chain
    from the leftmost leaf, in key order.  keys / vals / page / slot: every
    valid entry (value != 0 and (f ^ r) & 0xF == 0) of those leaves, sorted
    by key."""

    def __init__(self, image, root):
        img = np.frombuffer(np.ascontiguousarray(image, dtype=np.uint8), dtype=np.uint8)
        pg = img[:(img.size // PAGE) * PAGE].reshape(-1, PAGE)
        self.n_pages = pg.shape[0]

        def f64(off):
            return np.ascontiguousarray(pg[:, off:off + 8]).view("<u8").ravel()

        leftmost, sibling = f64(OFF_LEFTMOST), f64(OFF_SIBLING)
        lowest, highest = f64(OFF_LOWEST), f64(OFF_HIGHEST)
        level = pg[:, OFF_LEVEL]
        # from the root down the leftmost pointers, then along the siblings
        p = page_of(root)
        for _ in range(16):
            assert 0 < p < self.n_pages, ("bad page on the leftmost path", p)
            if leftmost[p] == 0:
                break
            p = page_of(leftmost[p])
        assert leftmost[p] == 0 and level[p] == 0, ("no leaf under the root", p)
        chain = []
        while True:
            assert 0 < p < self.n_pages and len(chain) <= self.n_pages, ("bad sibling chain", p)
            assert leftmost[p] == 0 and level[p] == 0, ("a non-leaf on the leaf chain", p)
            chain.append(p)
            if sibling[p] == 0:
                break
            p = page_of(sibling[p])
        self.leaf_page = np.array(chain, dtype=np.int64)
        self.leaf_lo = lowest[self.leaf_page]
        self.leaf_hi = highest[self.leaf_page]
        # the fences tile the key space
        assert self.leaf_lo[0] == 0 and self.leaf_hi[-1] == U64(KEY_MAX), "outer fences"
        assert np.array_equal(self.leaf_lo[1:], self.leaf_hi[:-1]), "fences do not tile"
        assert np.all(self.leaf_lo < self.leaf_hi), "empty fence range"
        rec = pg[self.leaf_page, OFF_RECORDS:OFF_RECORDS + LEAF_SLOTS * LEAF_ENTRY]
        rec = rec.reshape(-1, LEAF_SLOTS, LEAF_ENTRY)
        f, r = rec[:, :, 0], rec[:, :, 17]
        k = np.ascontiguousarray(rec[:, :, 1:9]).view("<u8").reshape(-1, LEAF_SLOTS)
        v = np.ascontiguousarray(rec[:, :, 9:17]).view("<u8").reshape(-1, LEAF_SLOTS)
        valid = (v != 0) & (((f ^ r) & 0xF) == 0)
        self.leaf_valid = valid.sum(axis=1)  # valid entries per leaf, chain order
        li, sl = np.nonzero(valid)
        kk, vv = k[li, sl], v[li, sl]
        # every valid key lies inside its leaf's fences
        assert np.all((kk >= self.leaf_lo[li]) & (kk < self.leaf_hi[li])), "a key outside its fences"
        o = np.argsort(kk, kind="stable")
        self.keys, self.vals = kk[o].astype(U64), vv[o].astype(U64)
        self.leaf = li[o]  # index into the chain
        self.page = self.leaf_page[li[o]].astype(np.int64)
        self.slot = sl[o].astype(np.int64)
        assert np.all(self.keys[1:] != self.keys[:-1]), "a key stored twice"

    def assert_equals(self, okeys, ovals):
        """the valid key -> value map equals the oracle's dump"""
        okeys, ovals = np.asarray(okeys, dtype=U64), np.asarray(ovals, dtype=U64)
        o = np.argsort(okeys, kind="stable")
        assert self.keys.size == okeys.size, (self.keys.size, okeys.size)
        assert np.array_equal(self.keys, okeys[o]), "stored keys differ from the oracle's"
        assert np.array_equal(self.vals, ovals[o]), "stored values differ from the oracle's"


class Directory:
    """A raw directory dump: ent (n, 16) uint32, entry p covering the keys
    [lo + (p << shift), lo + ((p + 1) << shift))."""

    def __init__(self, ent, lo, shift):
        self.ent = np.ascontiguousarray(ent, dtype=U32).reshape(-1, 16)
        self.n, self.lo, self.shift = self.ent.shape[0], int(lo), int(shift)
        self.cw = self.ent[:, 7]
        self.nl = (self.cw & U32(0xFF)).astype(np.int64)
        self.np_ = ((self.cw >> U32(16)) & U32(0xFF)).astype(np.int64)
        self.pairs16 = self.ent[:, 8:16].copy().view("<u2").reshape(-1, 16)
        self.bytes = self.ent.view(np.uint8).reshape(-1, 64)
        self.pair_usable = ((self.cw & U32(PAIRS)) != 0) & ((self.cw & U32(PAIRS_BAD)) == 0) & \
            (self.np_ <= PAIR_MAX)
        self.val_usable = ((self.cw & U32(VALS | PAIRS | PAIRS_BAD | FIX)) == U32(VALS | PAIRS)) & \
            (self.np_ <= VAL_MAX) & (self.nl <= 2)
        self.fp_form = (self.cw & U32(FP)) != 0

    def prefix_of(self, keys):
        """(prefix, covered) of each key: covered is False for a key outside
        the directory's range (and for the never-stored maximum key)"""
        keys = np.asarray(keys, dtype=U64)
        cov = (keys >= U64(self.lo)) & (keys != U64(KEY_MAX))
        with np.errstate(over="ignore"):
            p = (keys - U64(self.lo)) >> U64(self.shift)
        cov &= p < U64(self.n)
        return np.where(cov, p, U64(0)).astype(np.int64), cov

    def bounds(self, p):
        """first and last key of each prefix (uint64; the last one clamped to
        the maximum key)"""
        p = np.atleast_1d(np.asarray(p, dtype=np.int64))
        span = U64((1 << self.shift) - 1)
        assert self.lo + (self.n << self.shift) <= 1 << 64, "a directory past the key space"
        a = U64(self.lo) + (p.astype(U64) << U64(self.shift))
        with np.errstate(over="ignore"):
            b = np.where(a > U64(_M64) - span, U64(_M64), a + span)
        return a, b

    def inline(self, q):
        """pair q's inline (key, value) of every entry"""
        w = self.ent.astype(U64)
        if q == 0:
            return w[:, 2] | (w[:, 3] << U64(32)), w[:, 5] | (w[:, 6] << U64(32))
        return w[:, 12] | (w[:, 13] << U64(32)), w[:, 14] | (w[:, 15] << U64(32))


def prefix_tables(im, d):
    """idx: the valid keys the directory covers (indices into im.keys, in
    key order); pk: their prefixes; per prefix its key count and the rank
    (in idx) of its first key"""
    p, cov = d.prefix_of(im.keys)
    idx = np.nonzero(cov)[0]
    pk = p[idx]
    count = np.bincount(pk, minlength=d.n)
    first = np.zeros(d.n, dtype=np.int64)
    if idx.size:  # the keys are sorted: a prefix's keys are one run
        starts = np.nonzero(np.r_[True, pk[1:] != pk[:-1]])[0]
        first[pk[starts]] = starts
    return idx, pk, count, first


def covering_leaves(im, d, p):
    """index (into the chain) of the first and the last leaf whose fences
    intersect each prefix"""
    a, b = d.bounds(p)
    first = np.searchsorted(im.leaf_lo, a, side="right") - 1
    last = np.searchsorted(im.leaf_lo, b, side="right") - 1
    return first, last


def fresh_usable(im, d, p):
    """whether a fresh build would make each prefix a usable pair-form
    entry: at most four leaves cover it and it holds at most 16 valid keys"""
    p = np.atleast_1d(np.asarray(p, dtype=np.int64))
    first, last = covering_leaves(im, d, p)
    _, _, count, _ = prefix_tables(im, d)
    return (last - first + 1 <= LIST_MAX) & (count[p] <= PAIR_MAX)


def check_trusted(im, d, okeys=None, ovals=None, limit=16):
    """Every entry a get would trust against the pages (and the oracle's
    values for the inline copies; the image's own when none are given).
    Returns (violations, checked): a list of (kind, prefix, text), at most
    `limit` spelled out per kind, and the number of entries checked per
    class {"pair", "value", "fp"}."""
    out = []
    seen = {}

    def report(kind, prefixes, text):
        for x in np.unique(np.asarray(prefixes, dtype=np.int64)):
            seen[kind] = seen.get(kind, 0) + 1
            if seen[kind] <= limit:
                out.append((kind, int(x), f"{text}: entry {d.ent[x].tolist()}"))
            elif seen[kind] == limit + 1:
                out.append((kind, int(x), "... and more"))

    idx, pk, count, first = prefix_tables(im, d)
    keys, page, slot = im.keys[idx], im.page[idx], im.slot[idx]
    vals = im.vals[idx]
    if okeys is not None:
        okeys, ovals = np.asarray(okeys, dtype=U64), np.asarray(ovals, dtype=U64)
        o = np.argsort(okeys, kind="stable")
        at = np.searchsorted(okeys[o], keys)
        at = np.minimum(at, max(okeys.size - 1, 0))
        same = okeys.size > 0 and np.array_equal(okeys[o][at], keys)
        assert same, "the oracle does not hold every stored key"
        vals = ovals[o][at]
    fp = key_fp(keys)
    checked = {"pair": int(d.pair_usable.sum()), "value": int(d.val_usable.sum()),
               "fp": int(d.fp_form.sum())}

    # -- pair form: every valid key of a usable entry's prefix has its pair --
    ku = d.pair_usable[pk]
    found = np.zeros(keys.size, dtype=bool)
    for j in range(PAIR_MAX):
        pr = d.pairs16[pk, j].astype(np.int64)
        leaf = pr >> 14
        named = d.ent[pk, np.minimum(leaf, 3)].astype(np.int64)
        found |= (j < d.np_[pk]) & ((pr & 0xFF) == fp) & (((pr >> 8) & 63) == slot) & \
            (leaf < np.minimum(d.nl[pk], LIST_MAX)) & (named == page)
    report("pair", pk[ku & ~found], "a valid key of the prefix has no pair")
    report("pair-inline", np.nonzero(d.pair_usable & ((d.cw & U32(VALS)) != 0) & (d.np_ > 8))[0],
           "more than 8 pairs beside an inline entry")
    # the leaf list: the leaves covering the prefix, in key order, and their
    # split points (a usable entry's leaf count is 1..4)
    up = np.nonzero(d.pair_usable)[0]
    if up.size:
        lf, ll = covering_leaves(im, d, up)
        want_n = ll - lf + 1
        bad = (want_n != d.nl[up]) | (d.nl[up] < 1) | (d.nl[up] > LIST_MAX)
        a, _ = d.bounds(up)
        sh = U64(max(d.shift - 32, 0))
        for i in range(LIST_MAX):
            use = ~bad & (i < want_n)
            li = np.minimum(lf + i, im.leaf_page.size - 1)
            bad |= use & (d.ent[up, i].astype(np.int64) != im.leaf_page[li])
            if i:
                with np.errstate(over="ignore"):
                    t = ((im.leaf_lo[li] - a) >> sh) & U64(0xFFFFFFFF)
                bad |= use & (d.ent[up, 3 + i].astype(U64) != t)
        report("list", up[bad], "the leaf list is not the leaves covering the prefix")

    # -- value form: exactly the prefix's keys, with their values, inline --
    vp = np.nonzero(d.val_usable)[0]
    if vp.size:
        c, n = count[vp], d.np_[vp]
        report("value-count", vp[c != n], "pair count differs from the prefix's valid keys")
        k0, v0 = d.inline(0)
        k1, v1 = d.inline(1)
        ok = c == n
        one = ok & (c == 1)
        if keys.size:
            rank = first[vp]
            r0 = np.minimum(rank, keys.size - 1)
            r1 = np.minimum(rank + 1, keys.size - 1)
            A = (keys[r0], vals[r0])
            B = (keys[r1], vals[r1])
            e0 = (k0[vp], v0[vp])
            e1 = (k1[vp], v1[vp])

            def eq(x, y):
                return (x[0] == y[0]) & (x[1] == y[1])

            bad1 = one & ~eq(e0, A)
            two = ok & (c == 2)
            bad2 = two & ~((eq(e0, A) & eq(e1, B)) | (eq(e0, B) & eq(e1, A)))
            report("value", vp[bad1 | bad2], "inline (key, value) differ from the prefix's keys")

    # -- fingerprint form: one leaf holds the prefix, a byte per valid slot --
    kf = d.fp_form[pk]
    if kf.any():
        byte = np.where(slot < 24, 4 + slot, 8 + slot)
        got = d.bytes[pk, byte].astype(U32)
        report("fp-leaf", pk[kf & (d.ent[pk, 0].astype(np.int64) != page)],
               "a valid key of the prefix lies in another leaf")
        report("fp", pk[kf & (d.ent[pk, 0].astype(np.int64) == page) & (got != fp)],
               "a valid slot's fingerprint byte differs")
    return out, checked


def check_tree(tree, okeys=None, ovals=None):
    """check_trusted on a tree's own dumps (tree.dump_image(), tree.dir_dump());
    nothing to check while it has no valid directory"""
    ent, info = tree.dir_dump()
    if ent.shape[0] == 0:
        return [], {"pair": 0, "value": 0, "fp": 0}
    im = Image(*tree.dump_image())
    if okeys is not None:
        im.assert_equals(okeys, ovals)
    return check_trusted(im, Directory(ent, info["lo"], info["shift"]), okeys, ovals)
