"""The host-side directory model (tests/dir_model.py) can fail: a page image
of three leaves and a directory of sixteen entries, both written here byte by
byte from the documented formats, are accepted; every single mutation of an
entry a get would trust is reported.  No GPU: this is what shows that a clean
report from the model on the GPU tests means something."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dir_model as dm  # noqa: E402

U64 = np.uint64
SHIFT = 60  # sixteen prefixes over the 64-bit key space
L0, L1, L2, ROOT = 2, 3, 4, 1  # page indices (page 0: the superblock)
SEP1, SEP2 = 0x3000 << 48, 0x9800 << 48


def ga(page):
    return (page * 1024) << 16


def put64(pg, off, x):
    pg[off:off + 8] = np.frombuffer(int(x).to_bytes(8, "little"), dtype=np.uint8)


def leaf_page(lowest, highest, sibling, entries):
    """entries: slot -> (key, value, f, r)"""
    pg = np.zeros(1024, dtype=np.uint8)
    put64(pg, 17, sibling)
    pg[25] = 0
    put64(pg, 28, lowest)
    put64(pg, 36, highest)
    for s, (k, v, f, r) in entries.items():
        o = 44 + 18 * s
        pg[o] = f
        put64(pg, o + 1, k)
        put64(pg, o + 9, v)
        pg[o + 17] = r
    return pg


def K(prefix, low):
    return (prefix << SHIFT) | low


# slot -> (key, value, f, r) per leaf; torn (f != r) and deleted (value 0)
# entries are not valid keys
LEAVES = {
    L0: {0: (K(0, 5), 50, 1, 1), 1: (K(0, 9), 90, 2, 2), 2: (K(0, 77), 770, 3, 3),
         3: (K(1, 1), 11, 1, 1), 7: (K(1, 2), 12, 1, 1),
         9: (K(1, 3), 0, 1, 1),      # deleted
         10: (K(2, 4), 99, 1, 2)},   # torn
    L1: {0: (K(3, 0), 30, 1, 1), 5: (K(4, 8), 48, 4, 4), 30: (K(4, 9), 49, 5, 5),
         24: (K(5, 1), 51, 1, 1), 25: (K(5, 2), 52, 1, 1),
         40: (K(9, 3), 93, 1, 1)},
    L2: {2: (K(9, 0x0900 << 48), 94, 1, 1), 3: (K(10, 1), 101, 1, 1), 53: (K(15, 7), 157, 6, 6)},
}
# seventeen keys in prefix 12: more than an entry has pairs
LEAVES[L2].update({10 + i: (K(12, 100 + i), 1000 + i, 1, 1) for i in range(17)})


def build_image():
    img = np.zeros((5, 1024), dtype=np.uint8)
    root = img[ROOT]
    put64(root, 9, ga(L0))  # leftmost
    root[25] = 1
    root[26] = 1  # last_index: two records
    put64(root, 36, dm.KEY_MAX)
    put64(root, 44, SEP1)
    put64(root, 52, ga(L1))
    put64(root, 60, SEP2)
    put64(root, 68, ga(L2))
    img[L0] = leaf_page(0, SEP1, ga(L1), LEAVES[L0])
    img[L1] = leaf_page(SEP1, SEP2, ga(L2), LEAVES[L1])
    img[L2] = leaf_page(SEP2, dm.KEY_MAX, 0, LEAVES[L2])
    return img.ravel(), ga(ROOT)


def fp1(k):
    return int(dm.key_fp(np.array([k], dtype=U64))[0])


def pair(k, slot, leaf):
    return fp1(k) | (slot << 8) | (leaf << 14)


def set_pairs(e, prs):
    h = e[8:16].view("<u2")
    for j, p in enumerate(prs):
        h[j] = p


def set_inline(e, q, k, v):
    kw, vw = (2, 5) if q == 0 else (12, 14)
    e[kw], e[kw + 1] = k & 0xFFFFFFFF, k >> 32
    e[vw], e[vw + 1] = v & 0xFFFFFFFF, v >> 32


def build_dir():
    ent = np.zeros((16, 16), dtype=np.uint32)
    for p in range(16):  # plain entries (no claim): the covering leaf
        ent[p, 0] = L0 if p < 3 else L1 if p < 9 else L2
        ent[p, 7] = 1
    # p0: plain pair form, three keys in L0 (and the pair of a deleted key)
    set_pairs(ent[0], [pair(K(0, 77), 2, 0), pair(K(0, 5), 0, 0), pair(K(0, 1234), 20, 0),
                       pair(K(0, 9), 1, 0)])
    ent[0, 7] = 1 | dm.PAIRS | (4 << 16)
    # p1: value form, two keys
    set_pairs(ent[1], [pair(K(1, 2), 7, 0), pair(K(1, 1), 3, 0)])
    set_inline(ent[1], 0, K(1, 2), 12)
    set_inline(ent[1], 1, K(1, 1), 11)
    ent[1, 7] = 1 | dm.PAIRS | dm.VALS | (2 << 16)
    # p2: value form, empty (its one entry is torn)
    ent[2, 7] = 1 | dm.PAIRS | dm.VALS
    # p3: value form, one key, the first key of L1
    set_pairs(ent[3], [pair(K(3, 0), 0, 0)])
    set_inline(ent[3], 0, K(3, 0), 30)
    ent[3, 7] = 1 | dm.PAIRS | dm.VALS | (1 << 16)
    # p4: fingerprint form: every valid slot of L1
    b = ent[4].view(np.uint8)
    for s, (k, v, f, r) in LEAVES[L1].items():
        b[4 + s if s < 24 else 8 + s] = fp1(k)
    ent[4, 0], ent[4, 7] = L1, 1 | dm.FP
    # p5: unusable (bad pairs): garbage that makes no claim
    set_pairs(ent[5], [0xFFFF, 0x1234])
    ent[5, 7] = 1 | dm.PAIRS | dm.PAIRS_BAD | (2 << 16)
    # p9: pair form over two leaves, a key in each
    ent[9, 0], ent[9, 1] = L1, L2
    ent[9, 4] = (SEP2 - (9 << SHIFT)) >> (SHIFT - 32)
    set_pairs(ent[9], [pair(K(9, 3), 40, 0), pair(K(9, 0x0900 << 48), 2, 1)])
    ent[9, 7] = 2 | dm.PAIRS | (2 << 16)
    # p10: unusable by its count (17 pairs)
    ent[10, 7] = 1 | dm.PAIRS | (17 << 16)
    return ent


def stored():
    kv = [(k, v) for lf in LEAVES.values() for (k, v, f, r) in lf.values()
          if v != 0 and (f ^ r) & 0xF == 0]
    ks = np.array([k for k, _ in kv], dtype=U64)
    vs = np.array([v for _, v in kv], dtype=U64)
    return ks, vs


def check(ent):
    img, root = build_image()
    im = dm.Image(img, root)
    d = dm.Directory(ent, 0, SHIFT)
    return dm.check_trusted(im, d, *stored())


def test_key_fp_matches_its_definition():
    ks = [0, 1, 2, 0xDEADBEEF, (1 << 64) - 2, 0x9E3779B97F4A7C15]
    # a key whose raw hash byte is 0 maps to 1
    zero = next(k for k in range(1, 100000) if ((k * 0x9E3779B97F4A7C15) % (1 << 64)) >> 56 == 0)
    ks.append(zero)
    want = [(((k * 0x9E3779B97F4A7C15) % (1 << 64)) >> 56) or 1 for k in ks]
    assert dm.key_fp(np.array(ks, dtype=U64)).tolist() == want
    assert want[0] == 1 and want[-1] == 1


def test_the_image_parse_finds_the_valid_entries():
    img, root = build_image()
    im = dm.Image(img, root)
    assert im.leaf_page.tolist() == [L0, L1, L2]
    ks, vs = stored()
    assert ks.size == 31
    im.assert_equals(ks, vs)
    with pytest.raises(AssertionError):
        im.assert_equals(ks, vs ^ U64(1))
    with pytest.raises(AssertionError):
        im.assert_equals(ks[1:], vs[1:])
    assert im.leaf_valid.tolist() == [5, 6, 20]


def test_the_image_parse_reads_the_oracles_pages(oracle):
    """the CPU oracle writes the same page layout: the parse of its image
    equals its own dump (splits, deletes and updates included)"""
    orc = oracle.OracleTree(8 << 20)
    rng = np.random.default_rng(5)
    ks = np.unique(rng.integers(1, 1 << 63, 5000, dtype=np.int64).astype(U64))
    orc.apply_batch(ks, ks ^ U64(0x33))
    orc.apply_batch(ks[::7], np.zeros(ks[::7].size, dtype=U64))  # deletes
    orc.apply_batch(ks[1::7], ks[1::7] ^ U64(0x44))  # updates
    im = dm.Image(orc.image(), orc.root_ptr)
    im.assert_equals(*orc.dump())
    rc, oc = orc.check()
    assert rc == 0 and im.keys.size == oc["keys"] and im.leaf_page.size == oc["leaves"]
    orc.close()


def test_the_model_accepts_a_correct_directory():
    bad, checked = check(build_dir())
    assert bad == [], bad
    # p0..3, p9 usable pair entries (p1..3 in value form), p4 fingerprints;
    # p5, p10 and the plain entries make no claim
    assert checked == {"pair": 5, "value": 3, "fp": 1}, checked


def test_fresh_usable():
    img, root = build_image()
    im = dm.Image(img, root)
    d = dm.Directory(build_dir(), 0, SHIFT)
    # at most two leaves and three keys each, but prefix 12 holds seventeen
    assert dm.fresh_usable(im, d, np.arange(16)).tolist() == [p != 12 for p in range(16)]
    # two prefixes of 2^63 keys: ten keys in two leaves, twenty-one in two
    d2 = dm.Directory(np.zeros((2, 16), dtype=np.uint32), 0, 63)
    assert dm.fresh_usable(im, d2, [0, 1]).tolist() == [True, False]


def mut_slot(e):
    h = e[0, 8:16].view("<u2")
    h[1] += 1 << 8  # K(0, 5)'s slot 0 -> 1


def mut_drop(e):
    e[0, 7] -= 1 << 16  # the last pair (K(0, 9)'s) is no longer counted


def mut_value_bit(e):
    e[1, 14] ^= 1 << 9  # value1 of p1


def mut_key_bit(e):
    e[3, 3] ^= 1 << 31  # key0 of p3


def mut_leaf(e):
    e[9, 1] = L0  # the second leaf of p9


def mut_leaf_first(e):
    e[0, 0] = L1  # the only leaf of p0: every pair then names the wrong page


def mut_split_point(e):
    e[9, 4] += 1


def mut_fp(e):
    e[4].view(np.uint8)[8 + 30] = 0  # slot 30 of L1: K(4, 9)


def mut_fp_leaf(e):
    e[4, 0] = L2


def mut_np_small(e):
    e[1, 7] -= 1 << 16


def mut_np_large(e):
    e[3, 7] += 1 << 16  # claims two keys, the prefix holds one


def mut_pair_fp(e):
    h = e[9, 8:16].view("<u2")
    h[1] ^= 0x10


def mut_revive(e):
    e[5, 7] &= ~np.uint32(dm.PAIRS_BAD)  # the garbage entry becomes trusted


def mut_inline_overlap(e):
    e[1, 7] = 1 | dm.PAIRS | dm.VALS | (9 << 16)  # pairs 8.. lie over the inline entry


@pytest.mark.parametrize("mutate,kind,prefix", [
    (mut_slot, "pair", 0), (mut_drop, "pair", 0), (mut_value_bit, "value", 1),
    (mut_key_bit, "value", 3), (mut_leaf, "list", 9), (mut_leaf_first, "pair", 0),
    (mut_split_point, "list", 9), (mut_fp, "fp", 4), (mut_fp_leaf, "fp-leaf", 4),
    (mut_np_small, "value-count", 1), (mut_np_large, "value-count", 3), (mut_pair_fp, "pair", 9),
    (mut_revive, "pair", 5), (mut_inline_overlap, "pair-inline", 1),
], ids=lambda x: x.__name__ if callable(x) else None)
def test_every_single_mutation_is_reported(mutate, kind, prefix):
    ent = build_dir()
    mutate(ent)
    bad, _ = check(ent)
    assert (kind, prefix) in [(k, p) for k, p, _ in bad], bad
    assert {p for _, p, _ in bad} == {prefix}, bad  # and nothing else is blamed


def test_unusable_entries_make_no_claim():
    """garbage in an entry with bad pairs, a count past 16, or no form flag
    is not a violation"""
    ent = build_dir()
    ent[5, 0:7] = 0xDEAD
    ent[10, 8:16] = 0xFFFFFFFF
    ent[12, 0:7] = 7
    ent[12, 8:16] = 0x12345678
    ent[12, 7] = 3
    bad, checked = check(ent)
    assert bad == [] and checked["pair"] == 5, (bad, checked)
