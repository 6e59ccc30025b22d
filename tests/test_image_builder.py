"""The built page images (tests/image_builder.py) read by two independent
readers, on the CPU: the oracle (the reference's search, insert and
structural check in C) and tests/dir_model.Image (numpy).  Both must find
exactly the pairs the builder says it stored, and the oracle's inserts into
the hot leaf must split what the GPU tests rely on being split."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dir_model  # noqa: E402
import image_builder as ib  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402

U64 = np.uint64
SPARE = 1 << 20

SHAPES = [(lvl, path, full) for lvl in range(1, 8) for path in ("left", "middle", "right")
          for full in (True, False) if not (full and lvl == 7)]


def hot_chunk(info, n=40):
    """n absent keys inside the hot leaf's fences (stored keys + 7)"""
    k = info["keys"]
    hot = k[(k >= U64(info["hot_lo"])) & (k < U64(info["hot_hi"]))]
    assert hot.size == ib.FULL_KEYS
    new = hot[:n] + U64(7)
    assert not np.isin(new, k).any() and (new < U64(info["hot_hi"])).all()
    return new


@pytest.mark.parametrize("root_level,path,root_full", SHAPES)
def test_tall_image_read_by_the_oracle_and_the_model(root_level, path, root_full):
    img, root, info = ib.build_tall(root_level, path, root_full)
    assert img[:ib.PAGE].sum() == 0 and img.size % ib.PAGE == 0
    assert img.size // ib.PAGE == 1 + info["leaves"] + info["internal"]
    orc = OracleTree(image=img, root_ptr=root, spare_bytes=SPARE)
    rc, shape = orc.check()
    assert rc == 0, rc
    assert shape == {"leaves": info["leaves"], "internal": info["internal"],
                     "keys": info["n_keys"], "height": root_level + 1}
    ks, vs = orc.dump()  # in leaf order, then slot order
    o = np.argsort(ks)
    assert np.array_equal(ks[o], info["keys"]) and np.array_equal(vs[o], info["vals"])
    im = dir_model.Image(img, root)
    assert np.array_equal(im.keys, info["keys"]) and np.array_equal(im.vals, info["vals"])
    # what the description promises
    k = info["keys"]
    assert (k[1:] > k[:-1]).all() and info["step"] % 64 == 0 and info["step"] >= 64 * 24
    assert k[-1] >= U64(1 << 63) and k[0] < U64(1 << 63) and k[-1] != U64(ib.KEY_MAX)
    assert np.array_equal(info["vals"], k ^ U64(0x1111))
    assert im.leaf_valid.max() == 53 and (np.sort(im.leaf_valid)[:-1] <= 2).all()
    assert info["deleted"].size == 2 * ((info["leaves"] - 1) // 17)
    _, of = orc.search_batch(info["deleted"])
    assert not of.any()
    pg, lo, hi = info["path"][0]
    assert (pg, lo, hi) == (info["hot_page"], info["hot_lo"], info["hot_hi"])
    for lvl in range(1, root_level + 1):  # the path pages nest
        _, plo, phi = info["path"][lvl]
        assert plo <= lo and hi <= phi
        lo, hi = plo, phi
    assert (lo, hi) == (0, ib.KEY_MAX)
    orc.close()


def test_tall_image_is_deterministic_and_seeded():
    a = ib.build_tall(3, "middle", True, seed=5)
    b = ib.build_tall(3, "middle", True, seed=5)
    c = ib.build_tall(3, "middle", True, seed=6)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert not np.array_equal(a[0], c[0])
    assert np.array_equal(a[2]["keys"], c[2]["keys"])


def test_versions_and_node_id_reach_the_bytes():
    img, root, info = ib.build_tall(2, "right", True, page_ver=255, entry_ver=15, node_id=3)
    assert root & 0xFFFF == 3
    orc = OracleTree(image=img, root_ptr=root, node_id=3, spare_bytes=SPARE)
    rc, shape = orc.check()
    assert rc == 0 and shape["keys"] == info["n_keys"]
    pages = img.reshape(-1, ib.PAGE)[1:]
    assert (pages[:, ib.OFF_FRONT_VER] == 255).all()
    leaf = pages[:, ib.OFF_LEVEL] == 0
    assert (pages[leaf, ib.OFF_LEAF_REAR] == 255).all()
    assert (pages[~leaf, ib.OFF_INTERNAL_REAR] == 255).all()
    hot = img.reshape(-1, ib.PAGE)[info["hot_page"]]
    e = hot[ib.OFF_RECORDS:ib.OFF_RECORDS + 54 * 18].reshape(54, 18)
    used = e[:, 9:17].any(axis=1)
    assert used.sum() == 53 and (e[used, 0] == 15).all() and (e[used, 17] == 15).all()
    # the new keys split the leaf and the root: the page versions wrap to 0
    new = hot_chunk(info)
    orc.apply_batch(new, new)
    rc, shape = orc.check()
    assert rc == 0 and shape["height"] == 4
    after = orc.image().reshape(-1, ib.PAGE)
    assert after[info["hot_page"], ib.OFF_FRONT_VER] == 0
    orc.close()


def test_a_full_root_at_level_7_is_refused():
    with pytest.raises(ValueError):
        ib.build_tall(7, "left", True)
    with pytest.raises(ValueError):
        ib.build_tall(8, "left", False)


@pytest.mark.parametrize("root_level,path,root_full", [s for s in SHAPES if s[0] <= 6])
def test_forty_keys_in_the_hot_leaf_split_every_level(root_level, path, root_full):
    """The precondition of the GPU writer tests, on the oracle alone: 40 new
    keys in the hot leaf split the path page of every level; a full root
    grows by one level, a half-full root absorbs the separator.

    Root level 7 is not here: the oracle, like the reference (its path stack
    has one entry per level 0..6), cannot hand a separator to a level-7 page
    and asserts."""
    img, root, info = ib.build_tall(root_level, path, root_full)
    orc = OracleTree(image=img, root_ptr=root, spare_bytes=SPARE)
    new = hot_chunk(info)
    orc.apply_batch(new, new ^ U64(0x2222))
    rc, shape = orc.check()
    assert rc == 0, rc
    grown = 1 if root_full else 0
    assert orc.root_level == root_level + grown and shape["height"] == root_level + 1 + grown
    assert shape["keys"] == info["n_keys"] + new.size
    assert shape["leaves"] == info["leaves"] + 1
    # one new page per level below the root, and two where the root grew
    assert shape["internal"] == info["internal"] + (root_level - 1) + 2 * grown
    ks, vs = orc.dump()
    o = np.argsort(ks)
    want_k = np.concatenate([info["keys"], new])
    want_v = np.concatenate([info["vals"], new ^ U64(0x2222)])
    w = np.argsort(want_k)
    assert np.array_equal(ks[o], want_k[w]) and np.array_equal(vs[o], want_v[w])
    orc.close()


def test_entry_states_image():
    img, root, info = ib.build_entry_states()
    s = info["slots"]
    kinds = set(s["kind"].tolist())
    assert kinds == {ib.VALID, ib.DELETED, ib.STALE_COPY, ib.TORN, ib.VALID15}
    assert info["n_torn"] >= 20 and info["v15_keys"].size >= 20
    assert not set(info["torn_pages"]) & set(info["v15_pages"])
    # the bytes say what info says
    pg = img.reshape(-1, ib.PAGE)
    for i in range(s["page"].size):
        e = pg[s["page"][i], ib.OFF_RECORDS + 18 * s["slot"][i]:][:18]
        key, val = e[1:9].view("<u8")[0], e[9:17].view("<u8")[0]
        assert key == s["key"][i] and val == s["value"][i]
        torn = ((e[0] ^ e[17]) & 0xF) != 0
        kind = s["kind"][i]
        assert torn == (kind == ib.TORN)
        assert (val == 0) == (kind in (ib.DELETED, ib.STALE_COPY))
        if kind == ib.VALID15:
            assert e[0] == 15 and e[17] == 15
    orc = OracleTree(image=img, root_ptr=root)
    rc, shape = orc.check()
    assert rc == 0, rc
    assert shape == {"leaves": info["leaves"], "internal": info["internal"],
                     "keys": info["n_valid"] + info["n_torn"], "height": 3}
    ok = (s["kind"] == ib.VALID) | (s["kind"] == ib.VALID15)
    ks, vs = orc.dump()
    o, w = np.argsort(ks), np.argsort(s["key"][ok])
    assert np.array_equal(ks[o], s["key"][ok][w]) and np.array_equal(vs[o], s["value"][ok][w])
    assert np.array_equal(ks[o], info["keys"]) and np.array_equal(vs[o], info["vals"])
    assert np.array_equal(info["vals"], info["keys"] ^ U64(ib.VALUE_XOR))
    im = dir_model.Image(img, root)
    assert np.array_equal(im.keys, info["keys"]) and np.array_equal(im.vals, info["vals"])
    for name in ("torn", "deleted"):
        assert not np.isin(info[name], info["keys"]).any()
        ov, of = orc.search_batch(info[name])
        assert not of.any() and not ov.any(), name
    # a stale copy beside its live slot: the key is found once, with its value
    ov, of = orc.search_batch(info["stale_copy"])
    at = np.searchsorted(info["keys"], info["stale_copy"])
    assert of.all() and np.array_equal(ov, info["vals"][at])
    live_slot = {(int(p), int(k)): int(sl) for p, k, sl in
                 zip(s["page"][ok], s["key"][ok], s["slot"][ok])}
    c = s["kind"] == ib.STALE_COPY
    side = [np.sign(int(sl) - live_slot[(int(p), int(k))])
            for p, k, sl in zip(s["page"][c], s["key"][c], s["slot"][c])]
    assert -1 in side and 1 in side
    orc.close()
