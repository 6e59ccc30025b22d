"""The structural check (check_image, behind Tree.check() and every
t.check() of the suite) shown sound and broken images, without a GPU.

The images the builders make, and the odd but sound states a tree can be in,
are accepted with the right counts.  A table of minimal mutations, one field
each, is rejected with the code the check gives that invariant.  A seeded run
of random single-byte changes closes the file: the check and its independent
restatement (state_model.structure) must agree on accept or reject for every
one.  No broken image is loaded into a tree."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import export_model as em  # noqa: E402
import image_builder as ib  # noqa: E402
import sherman_amd as shm  # noqa: E402
import state_model as sm  # noqa: E402

U64 = np.uint64
KEY_MAX = ib.KEY_MAX

# check_image's codes (tree_image.cpp)
ROOT, SIBLING, LEVEL, LEAF_KIND, VERSION, FENCES, KEY, FULL, LAST_INDEX, LEFTMOST, SEPS, CHILD, \
    CHILD_LEVEL, LAST_HIGHEST, DUP, OFF_CHAIN = -1, -2, -3, -4, -5, -6, -7, -8, -9, -10, -11, \
    -12, -13, -14, -15, -16
# -20, the walk's page-count guard, cannot be reached: a walk goes on only
# from a page whose lowest fence equals the highest of the page before it and
# whose own highest is above that, so the fences ascend strictly along it and
# no page is visited twice; a sibling pointer that turns back gives -6
ALL_CODES = set(range(-16, 0))


def ga(page, node=0):
    return (int(page) << 26) | node


def get64(img, page, off):
    return int.from_bytes(bytes(img[page * ib.PAGE + off:page * ib.PAGE + off + 8]), "little")


def put64(img, page, off, val):
    img[page * ib.PAGE + off:page * ib.PAGE + off + 8] = np.frombuffer(
        int(val).to_bytes(8, "little"), dtype=np.uint8)


def put8(img, page, off, val):
    img[page * ib.PAGE + off] = val


def copy_page(img, src, dst):
    img[dst * ib.PAGE:(dst + 1) * ib.PAGE] = img[src * ib.PAGE:(src + 1) * ib.PAGE].copy()


def put16(img, page, off, val):
    img[page * ib.PAGE + off:page * ib.PAGE + off + 2] = np.frombuffer(
        int(val).to_bytes(2, "little", signed=True), dtype=np.uint8)


def chains(img, root):
    """the pages of every level in key order, by level: down the leftmost
    pointers of the first pages, along the siblings"""
    out = {}
    p = root >> 26
    while True:
        lvl = int(img[p * ib.PAGE + ib.OFF_LEVEL])
        chain, q = [], p
        while q:
            chain.append(q)
            q = get64(img, q, ib.OFF_SIBLING) >> 26
        out[lvl] = chain
        if lvl == 0:
            return out
        p = get64(img, p, ib.OFF_LEFTMOST) >> 26


def entry(slot, field):
    """byte offset of a leaf entry's key (1) or value (9)"""
    return ib.OFF_RECORDS + ib.LEAF_ENTRY * slot + field


def rec(j, field=0):
    """byte offset of an internal record's separator (0) or pointer (8)"""
    return ib.OFF_RECORDS + ib.INTERNAL_ENTRY * j + field


@functools.lru_cache(maxsize=None)
def entries():
    img, root, info = ib.build_entry_states()
    img.setflags(write=False)
    return img, root, info


def soiled(img, info, n, seed):
    per_kind, per_bad = ib.soil_sizes(n)
    soil, _ = ib.soil_pages(n, ib.soil_keys(info, per_kind, per_bad), seed,
                            first_page=img.size // ib.PAGE)
    return ib.with_soil(img, soil)


def root_leaf(slots=()):
    """a tree that is one leaf: page 1, fences 0 and 2^64 - 1; slots: (slot,
    key, value)"""
    img = np.zeros((2, ib.PAGE), dtype=np.uint8)
    img[1, ib.OFF_FRONT_VER] = img[1, ib.OFF_LEAF_REAR] = 1
    put16(img.reshape(-1), 1, ib.OFF_LAST_INDEX, -1)
    put64(img.reshape(-1), 1, ib.OFF_HIGHEST, KEY_MAX)
    if slots:
        s, k, v = zip(*slots)
        ib._put_entries(img, np.ones(len(s), dtype=np.int64), s, k, v, 2, 2)
    return img.reshape(-1), ga(1)


def both(img, root, node=0):
    code, counts = shm.check_image(img, root, node)
    bad, mcounts = sm.structure(img, root, node)
    assert (code == 0) == (bad == []), (code, bad)
    if code == 0:
        assert counts == mcounts, (counts, mcounts)
    return code, counts, bad


# ---- sound images ----------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 3, 7])
def test_tall_images_are_accepted(level):
    img, root, info = ib.build_tall(level, "middle", level < 7)
    code, counts, _ = both(img, root)
    assert code == 0
    assert counts == {"leaves": info["leaves"], "internal": info["internal"], "keys": info["n_keys"]}


def test_entry_states_are_accepted():
    """deleted slots, stale copies of live keys (value 0), torn entries (a
    value, so counted), an all-deleted leaf; and with soil pages appended the
    counts stay"""
    img, root, info = entries()
    want = {"leaves": 40, "internal": 6, "keys": info["n_valid"] + info["n_torn"]}
    assert info["n_torn"] == 25 and info["stale_copy"].size >= 4
    code, counts, _ = both(img, root)
    assert code == 0 and counts == want
    code, counts, _ = both(soiled(img, info, 6, 5), root)
    assert code == 0 and counts == want


def test_node_id_is_part_of_every_pointer():
    img, root, info = ib.build_tall(3, "left", True, node_id=3)
    assert both(img, root, node=3)[0] == 0
    assert both(img, root, node=0)[0] == ROOT


def test_empty_and_all_deleted_root_leaf():
    img, root = root_leaf()
    code, counts, _ = both(img, root)
    assert code == 0 and counts == {"leaves": 1, "internal": 0, "keys": 0}
    img, root = root_leaf([(s, 64 * (s + 1), 0) for s in range(54)])
    code, counts, _ = both(img, root)
    assert code == 0 and counts == {"leaves": 1, "internal": 0, "keys": 0}
    img, root = root_leaf([(5, 640, 7), (9, 640, 0), (53, KEY_MAX - 1, 1), (0, 0, 9)])
    code, counts, _ = both(img, root)
    assert code == 0 and counts == {"leaves": 1, "internal": 0, "keys": 3}


@pytest.mark.parametrize("in_root,in_level1", [(True, False), (False, True), (True, True)])
def test_a_dropped_separator_is_accepted(in_root, in_level1):
    """the last child of a page reachable through its left sibling alone: on
    the chain, named by no record"""
    img, root, info = entries()
    img = em.drop_last_separators(img, root, in_root=in_root, in_level1=in_level1)
    code, counts, _ = both(img, root)
    assert code == 0
    assert counts == {"leaves": 40, "internal": 6, "keys": info["n_valid"] + info["n_torn"]}


# ---- one broken field each ---------------------------------------------------------------
def _held_slot(img, page, nth=0):
    v = sm._slots(img.reshape(-1, ib.PAGE)[page:page + 1])[1][0]
    return int(np.nonzero(v != 0)[0][nth])


def mutations():
    """name -> (expected code, model kind, function(img, root, chains, info)
    -> root or None) on a copy of the entry-states image with a copy of leaf
    10 and of level-1 page 2 appended (pages n and n + 1, named by nothing)"""
    n_img = entries()[0].size // ib.PAGE
    m = {}

    def case(name, code, kind):
        def reg(f):
            m[name] = (code, kind, f)
            return f
        return reg

    # the root pointer
    case("root off a page boundary", ROOT, sm.BAD_ROOT)(lambda i, r, c, o: r + (8 << 16))
    case("root on another node", ROOT, sm.BAD_ROOT)(lambda i, r, c, o: r | 1)
    case("root past the image", ROOT, sm.BAD_ROOT)(lambda i, r, c, o: ga(i.size // ib.PAGE))
    case("root null", ROOT, sm.BAD_ROOT)(lambda i, r, c, o: 0)
    case("root the superblock", ROOT, sm.BAD_ROOT)(lambda i, r, c, o: ga(0))
    # sibling pointers
    case("sibling off a page boundary", SIBLING, sm.BAD_SIBLING)(
        lambda i, r, c, o: put64(i, c[0][3], ib.OFF_SIBLING, ga(c[0][4]) + (2 << 16)))
    case("sibling on another node", SIBLING, sm.BAD_SIBLING)(
        lambda i, r, c, o: put64(i, c[1][1], ib.OFF_SIBLING, ga(c[1][2], 9)))
    case("sibling past the image", SIBLING, sm.BAD_SIBLING)(
        lambda i, r, c, o: put64(i, c[0][38], ib.OFF_SIBLING, ga(i.size // ib.PAGE)))
    # child pointers
    case("child off a page boundary", CHILD, sm.BAD_CHILD)(
        lambda i, r, c, o: put64(i, c[1][1], rec(2, 8), ga(c[0][11]) + (512 << 16)))
    case("child on another node", CHILD, sm.BAD_CHILD)(
        lambda i, r, c, o: put64(i, c[2][0], rec(0, 8), ga(c[1][1], 1)))
    case("child past the image", CHILD, sm.BAD_CHILD)(
        lambda i, r, c, o: put64(i, c[1][4], rec(6, 8), ga(1 << 20)))
    case("child null", CHILD, sm.BAD_CHILD)(lambda i, r, c, o: put64(i, c[1][0], rec(0, 8), 0))
    case("leftmost off a page boundary", LEFTMOST, sm.BAD_CHILD)(
        lambda i, r, c, o: put64(i, c[1][3], ib.OFF_LEFTMOST, ga(c[0][24]) + (1 << 16)))
    case("leftmost on another node", LEFTMOST, sm.BAD_CHILD)(
        lambda i, r, c, o: put64(i, c[2][0], ib.OFF_LEFTMOST, ga(c[1][0], 2)))
    # level and kind
    case("level byte of a first page", LEVEL, sm.LEVEL)(
        lambda i, r, c, o: put8(i, c[1][0], ib.OFF_LEVEL, 2))
    case("level byte of the first leaf", LEVEL, sm.LEVEL)(
        lambda i, r, c, o: put8(i, c[0][0], ib.OFF_LEVEL, 1))
    case("level byte of a leaf a record names", CHILD_LEVEL, sm.CHILD_LEVEL)(
        lambda i, r, c, o: put8(i, c[0][5], ib.OFF_LEVEL, 1))
    case("level byte of the root", CHILD_LEVEL, sm.CHILD_LEVEL)(
        lambda i, r, c, o: put8(i, c[2][0], ib.OFF_LEVEL, 3))
    case("leaf with a leftmost pointer", LEAF_KIND, sm.LEAF_KIND)(
        lambda i, r, c, o: put64(i, c[0][7], ib.OFF_LEFTMOST, ga(c[0][8])))
    case("internal page without a leftmost pointer", LEAF_KIND, sm.LEAF_KIND)(
        lambda i, r, c, o: put64(i, c[1][2], ib.OFF_LEFTMOST, 0))
    # versions
    case("leaf front != rear", VERSION, sm.VERSION)(
        lambda i, r, c, o: put8(i, c[0][12], ib.OFF_LEAF_REAR, 2))
    case("internal front != rear", VERSION, sm.VERSION)(
        lambda i, r, c, o: put8(i, c[1][3], ib.OFF_FRONT_VER, 0))
    # fences
    case("lowest != the left neighbour's highest", FENCES, sm.FENCES)(
        lambda i, r, c, o: put64(i, c[0][8], ib.OFF_HIGHEST, get64(i, c[0][8], ib.OFF_HIGHEST) - 1))
    case("level 1: lowest != the left neighbour's highest", FENCES, sm.FENCES)(
        lambda i, r, c, o: put64(i, c[1][1], ib.OFF_HIGHEST, get64(i, c[1][1], ib.OFF_HIGHEST) + 1))
    case("first lowest != 0", LEFTMOST, sm.CHILD_LOWEST)(
        lambda i, r, c, o: put64(i, c[0][0], ib.OFF_LOWEST, 1))
    case("highest == lowest", FENCES, sm.FENCES)(
        lambda i, r, c, o: put64(i, c[0][39], ib.OFF_HIGHEST, get64(i, c[0][39], ib.OFF_LOWEST)))
    case("highest < lowest", FENCES, sm.FENCES)(
        lambda i, r, c, o: put64(i, c[0][39], ib.OFF_HIGHEST, 5))
    case("last leaf's highest != 2^64 - 1", LAST_HIGHEST, sm.LAST_HIGHEST)(
        lambda i, r, c, o: put64(i, c[0][39], ib.OFF_HIGHEST, KEY_MAX - 1))
    case("last level-1 page's highest != 2^64 - 1", LAST_HIGHEST, sm.LAST_HIGHEST)(
        lambda i, r, c, o: put64(i, c[1][4], ib.OFF_HIGHEST, KEY_MAX - 1))
    case("a chain cut short", LAST_HIGHEST, sm.LAST_HIGHEST)(
        lambda i, r, c, o: put64(i, c[0][20], ib.OFF_SIBLING, 0))
    case("last sibling back to the first page", FENCES, sm.FENCES)(
        lambda i, r, c, o: put64(i, c[0][39], ib.OFF_SIBLING, ga(c[0][0])))
    case("a sibling that skips a page", FENCES, sm.FENCES)(
        lambda i, r, c, o: put64(i, c[0][13], ib.OFF_SIBLING, ga(c[0][15])))
    # leaf entries
    case("a held key equal to the highest fence", KEY, sm.KEY_OUTSIDE)(
        lambda i, r, c, o: put64(i, c[0][4], entry(_held_slot(i, c[0][4]), 1),
                                 get64(i, c[0][4], ib.OFF_HIGHEST)))
    case("a held key equal to lowest - 1", KEY, sm.KEY_OUTSIDE)(
        lambda i, r, c, o: put64(i, c[0][6], entry(_held_slot(i, c[0][6], 2), 1),
                                 get64(i, c[0][6], ib.OFF_LOWEST) - 1))
    case("a torn key outside the fences", KEY, sm.KEY_OUTSIDE)(
        lambda i, r, c, o: put64(i, int(o["slots"]["page"][o["slots"]["kind"] == ib.TORN][0]),
                                 entry(int(o["slots"]["slot"][o["slots"]["kind"] == ib.TORN][0]), 1),
                                 KEY_MAX))

    @case("a key held in two slots of a leaf", DUP, sm.DUPLICATE)
    def _(i, r, c, o):
        s = o["slots"]
        j = int(np.nonzero(s["kind"] == ib.STALE_COPY)[0][0])  # the stale copy gets a value
        put64(i, int(s["page"][j]), entry(int(s["slot"][j]), 9), 77)

    @case("a key held in two slots, the copy above", DUP, sm.DUPLICATE)
    def _(i, r, c, o):
        s = o["slots"]
        j = int(np.nonzero(s["kind"] == ib.STALE_COPY)[0][1])
        put64(i, int(s["page"][j]), entry(int(s["slot"][j]), 9), 1 << 63)

    # internal pages
    case("last_index 60", LAST_INDEX, sm.LAST_INDEX)(
        lambda i, r, c, o: put16(i, c[1][1], ib.OFF_LAST_INDEX, 60))
    case("last_index -2", LAST_INDEX, sm.LAST_INDEX)(
        lambda i, r, c, o: put16(i, c[2][0], ib.OFF_LAST_INDEX, -2))
    case("leftmost child's lowest", LEFTMOST, sm.CHILD_LOWEST)(
        lambda i, r, c, o: put64(i, c[0][8], ib.OFF_LOWEST, get64(i, c[0][8], ib.OFF_LOWEST) + 1))
    case("leftmost names the second child", LEFTMOST, sm.CHILD_LOWEST)(
        lambda i, r, c, o: put64(i, c[1][1], ib.OFF_LEFTMOST, ga(c[0][9])))
    case("separators equal", SEPS, sm.SEPARATORS)(
        lambda i, r, c, o: put64(i, c[1][1], rec(1), get64(i, c[1][1], rec(0))))
    case("separators descending", SEPS, sm.SEPARATORS)(
        lambda i, r, c, o: put64(i, c[1][1], rec(1), get64(i, c[1][1], rec(0)) - 1))
    case("first separator == lowest", SEPS, sm.SEPARATORS)(
        lambda i, r, c, o: put64(i, c[1][1], rec(0), get64(i, c[1][1], ib.OFF_LOWEST)))
    case("last separator == highest", SEPS, sm.SEPARATORS)(
        lambda i, r, c, o: put64(i, c[1][2], rec(6), get64(i, c[1][2], ib.OFF_HIGHEST)))
    case("child's lowest != its separator", CHILD, sm.CHILD_LOWEST)(
        lambda i, r, c, o: put64(i, c[1][1], rec(2), get64(i, c[1][1], rec(2)) + 1))
    case("a named child's lowest changed", CHILD, sm.CHILD_LOWEST)(
        lambda i, r, c, o: put64(i, c[0][9], ib.OFF_LOWEST, get64(i, c[0][9], ib.OFF_LOWEST) - 1))
    case("a record names the next child", CHILD, sm.CHILD_LOWEST)(
        lambda i, r, c, o: put64(i, c[1][3], rec(1, 8), ga(c[0][27])))
    case("a level-2 record names the grandchild leaf", CHILD_LEVEL, sm.CHILD_LEVEL)(
        lambda i, r, c, o: put64(i, c[2][0], rec(1, 8), ga(c[0][16])))
    # a stale copy with the right lowest fence and level, off the chain
    case("a record names a stale copy of a leaf", OFF_CHAIN, sm.CHILD_OFF_CHAIN)(
        lambda i, r, c, o: put64(i, c[1][1], rec(1, 8), ga(n_img)))
    case("leftmost names a stale copy of a leaf", OFF_CHAIN, sm.CHILD_OFF_CHAIN)(
        lambda i, r, c, o: (copy_page(i, c[0][16], n_img),
                            put64(i, c[1][2], ib.OFF_LEFTMOST, ga(n_img))))
    case("the root names a stale copy of a level-1 page", OFF_CHAIN, sm.CHILD_OFF_CHAIN)(
        lambda i, r, c, o: put64(i, c[2][0], rec(1, 8), ga(n_img + 1)))
    return m


MUTATIONS = mutations()


def mutable():
    """the entry-states image with a copy of leaf 10 and of level-1 page 2
    appended, named by nothing: still sound"""
    img, root, info = entries()
    c = chains(img, root)
    img = np.concatenate([img, img[c[0][10] * ib.PAGE:(c[0][10] + 1) * ib.PAGE],
                          img[c[1][2] * ib.PAGE:(c[1][2] + 1) * ib.PAGE]])
    return img, root, c, info


def test_the_mutable_image_is_sound():
    img, root, c, info = mutable()
    assert [len(c[lvl]) for lvl in (0, 1, 2)] == [40, 5, 1]
    code, counts, _ = both(img, root)
    assert code == 0 and counts["leaves"] == 40 and counts["internal"] == 6


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_one_broken_field_is_rejected(name):
    want, kind, f = MUTATIONS[name]
    img, root, c, info = mutable()
    before = img.copy()
    new_root = f(img, root, c, info)
    if isinstance(new_root, int):
        root = new_root
        assert np.array_equal(img, before)
    else:
        assert not np.array_equal(img, before), "the mutation changed nothing"
    code, counts = shm.check_image(img, root)
    bad, _ = sm.structure(img, root)
    assert code == want, (name, code, bad)
    assert counts == {"leaves": 0, "internal": 0, "keys": 0}
    assert bad and {b[0] for b in bad} == {kind}, (name, bad)


def test_54_held_entries_are_rejected():
    """the hot leaf of a tall image holds 53: one more entry in its free slot"""
    img, root, info = ib.build_tall(1, "middle", True)
    img = img.copy()
    p = info["hot_page"]
    v = sm._slots(img.reshape(-1, ib.PAGE)[p:p + 1])[1][0]
    free = np.nonzero(v == 0)[0]
    assert free.size == 1
    put64(img, p, entry(int(free[0]), 1), info["hot_lo"] + 1)
    put64(img, p, entry(int(free[0]), 9), 5)
    code, _ = shm.check_image(img, root)
    bad, _ = sm.structure(img, root)
    assert code == FULL and [b[0] for b in bad] == [sm.LEAF_FULL]


def test_every_code_is_hit():
    hit = {code for code, _, _ in MUTATIONS.values()} | {FULL}
    assert hit == ALL_CODES, sorted(ALL_CODES - hit)


def test_random_single_byte_changes_agree():
    """2,000 seeded single-byte changes of the header fields and records
    (bytes 8..1023) of the pages the root reaches: the check and the model
    accept or reject together.  Half flip one bit, half write a random byte;
    half land in the 36 header bytes.  (With fewer than 64 pages a page pointer
    is one byte, so single bytes do turn pointers to other pages and to 0.)"""
    img0, root, info = entries()
    img0 = soiled(img0, info, 3, 9)
    reached = np.nonzero(ib.reached_pages(img0, root))[0]
    assert reached.size == 46
    rng = np.random.default_rng(0xC4EC)
    rejected = accepted = 0
    codes = set()
    for i in range(2000):
        p = int(rng.choice(reached))
        b = int(rng.integers(8, 44)) if i % 2 else int(rng.integers(44, ib.PAGE))
        old = int(img0[p * ib.PAGE + b])
        new = old ^ (1 << int(rng.integers(0, 8))) if i % 4 < 2 else int(rng.integers(0, 256))
        if new == old:
            new ^= 0x80
        img = img0.copy()
        img[p * ib.PAGE + b] = new
        code, counts = shm.check_image(img, root)
        bad, mcounts = sm.structure(img, root)
        assert (code == 0) == (bad == []), (p, b, old, new, code, bad)
        if code == 0:
            assert counts == mcounts, (p, b, old, new, counts, mcounts)
            accepted += 1
        else:
            rejected += 1
            codes.add(code)
    print(f"accepted {accepted}, rejected {rejected}, codes {sorted(codes)}")
    assert accepted >= 300 and rejected >= 300 and len(codes) >= 10
