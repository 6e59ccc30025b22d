"""The soil builder (tests/image_builder.soil_pages) on the CPU: pages that
pass a page sweep's leaf test and that the tree does not reach.

The oracle walks an image from its root, so soil must change nothing it says:
the same shape, the same dump, no soil key found that the tree does not hold,
the tree's value for every key it does hold.  The three device builders that
sweep the arena by page (k_vt_build, k_dir_pairs, k_sum_rebuild) test a page
with `level == 0 and leftmost == 0` at most; that predicate is restated here
in numpy and must accept every soil leaf, so a sweep that trusts it reads the
soil.  The soil keys are also held to what the GPU tests need of them: enough
keys of each kind in buckets of the key-value table that stay alive."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dir_model  # noqa: E402
import image_builder as ib  # noqa: E402
import valtab_model  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402

U64 = np.uint64

# The table of a read phase's build over an arena of at most 1024 pages: the
# directory has 2^(10 + 4) entries over the key range hint, the table half as
# many buckets (tree_dir.cpp dir_bits_for, vt_build).
TABLE_BITS = 13
HINTS = {"full": (0, 64), "narrow": (1 << 62, 63)}
VALID_KINDS = (ib.ABSENT, ib.SHADOW, ib.DELETED)


sweep_leaf, sweep_entries = ib.sweep_leaf, ib.sweep_entries


def live_buckets(tree_keys, soil, lo, bits, kind):
    """the soil keys of `kind` whose bucket holds at most 8 keys, the soil's
    valid keys counted (valtab_model.counts)"""
    shift, n = bits - TABLE_BITS, 1 << TABLE_BITS
    swept = np.concatenate([soil[k] for k in (ib.ABSENT, ib.SHADOW, ib.DELETED, ib.OUTSIDE)])
    cnt = valtab_model.counts(np.unique(np.concatenate([tree_keys, swept])), lo, shift, n)
    b = valtab_model.bucket_of(soil[kind], lo, shift)
    inside = (b >= 0) & (b < n)
    return soil[kind][inside][cnt[b[inside]] <= valtab_model.SLOTS]


# (a narrow hint holds too few of the tall image's 20 deleted keys)
CASES = [(w, n, "full") for w in ("tall-left", "tall-middle", "tall-right", "entry-states")
         for n in (0, 3)] + [("entry-states", 3, "narrow")]


@pytest.mark.parametrize("which,node_id,hint", CASES)
def test_soil_changes_nothing_the_oracle_says(which, node_id, hint):
    if which == "entry-states":
        img, root, info = ib.build_entry_states(node_id=node_id)
    else:
        img, root, info = ib.build_tall(2, which[5:], True, node_id=node_id)
    lo, bits = HINTS[hint]
    n_img = img.size // ib.PAGE
    keys = ib.soil_keys(info, hint=HINTS[hint])
    pages, soil = ib.soil_pages(6, keys, seed=1, node_id=node_id, first_page=n_img)
    both = ib.with_soil(img, pages)
    assert both.size == img.size + 6 * ib.PAGE and np.array_equal(both[:img.size], img)

    # the kinds are what they claim to be
    held = dict(zip(info["keys"].tolist(), info["vals"].tolist()))
    written = np.concatenate([info["keys"], info["deleted"]] +
                             [info[k] for k in ("torn", "stale_copy") if k in info])
    for kind in (ib.ABSENT, ib.OUTSIDE, ib.TORN, ib.NULL):
        assert not np.isin(soil[kind], written).any(), kind
    assert np.isin(soil[ib.SHADOW], info["keys"]).all()
    assert np.isin(soil[ib.DELETED], info["deleted"]).all()
    assert not np.isin(soil[ib.DELETED], info["keys"]).any()
    if hint == "full":
        assert soil[ib.OUTSIDE].size == 0
    else:
        out = soil[ib.OUTSIDE]
        assert out.size >= 16 and np.all((out < U64(lo)) | (out - U64(lo) >= U64(1 << bits)))
        for kind in VALID_KINDS:
            k = soil[kind]
            assert np.all((k >= U64(lo)) & (k - U64(lo) < U64(1 << bits))), kind
    s = soil["slots"]
    valid = np.isin(s["kind"], VALID_KINDS + (ib.OUTSIDE,))
    assert np.all(s["value"][valid] == s["key"][valid] ^ U64(ib.SOIL_XOR))
    shadow = s["kind"] == ib.SHADOW
    assert all(held[int(k)] != int(v) for k, v in zip(s["key"][shadow], s["value"][shadow]))

    # a sweep takes every soil leaf and exactly the valid soil entries; it
    # skips the page that looks internal, which would give entries as a leaf
    leaf = sweep_leaf(pages)
    assert leaf[soil["leaf_pages"]].all() and not leaf[soil["internal_pages"]].any()
    assert soil["internal_pages"].size == 1 and soil["leaf_pages"].size == 5
    front = pages[soil["leaf_pages"], ib.OFF_FRONT_VER]
    assert np.array_equal(front, pages[soil["leaf_pages"], ib.OFF_LEAF_REAR])
    pg, sl, k, v = sweep_entries(pages)
    want = np.lexsort((s["slot"][valid], s["page"][valid]))
    assert np.array_equal(pg, s["page"][valid][want]) and np.array_equal(sl, s["slot"][valid][want])
    assert np.array_equal(k, s["key"][valid][want]) and np.array_equal(v, s["value"][valid][want])
    as_leaf = pages[soil["internal_pages"]].copy()
    as_leaf[:, ib.OFF_LEVEL] = 0
    as_leaf[:, ib.OFF_LEFTMOST:ib.OFF_LEFTMOST + 8] = 0
    assert sweep_entries(as_leaf)[0].size > 0

    # the oracle: same check, same shape, same dump, the tree's answers
    a = OracleTree(image=img, root_ptr=root, node_id=node_id)
    b = OracleTree(image=both, root_ptr=root, node_id=node_id)
    ra, rb = a.check(), b.check()
    assert ra[0] == 0 and ra == rb, (ra, rb)
    assert ra[1]["leaves"] == info["leaves"] and ra[1]["internal"] == info["internal"]
    da, db = a.dump(), b.dump()
    assert np.array_equal(da[0], db[0]) and np.array_equal(da[1], db[1])
    for kind in (ib.ABSENT, ib.DELETED, ib.OUTSIDE, ib.TORN, ib.NULL):
        assert not b.search_batch(soil[kind])[1].any(), kind
    sv, sf = b.search_batch(soil[ib.SHADOW])
    assert sf.all() and np.array_equal(sv, soil[ib.SHADOW] ^ U64(ib.VALUE_XOR))
    im = dir_model.Image(both, root)
    assert np.array_equal(im.keys, info["keys"]) and np.array_equal(im.vals, info["vals"])
    # the numpy walk the GPU tests find unreached pages with: every page of
    # the tree, no page of the soil (its internal page points at soil leaves)
    reach = ib.reached_pages(both, root)
    assert reach[1:n_img].all() and not reach[0] and not reach[n_img:].any()
    assert reach.sum() == info["leaves"] + info["internal"]
    assert np.isin(im.leaf_page, np.nonzero(reach)[0]).all()
    a.close()
    b.close()

    # what the GPU tests need: 16 keys of each kind in buckets that stay alive
    for kind in VALID_KINDS:
        ok = live_buckets(info["keys"], soil, lo, bits, kind)
        assert ok.size >= 16, (kind, ok.size, soil[kind].size)


@pytest.mark.parametrize("n", range(1, 8))
def test_soil_of_every_size_a_failed_take_can_leave(n):
    """1 .. 7 pages (the spares of an exact arena): the keys fit the leaves, a
    single page is a leaf, and each leaf holds keys of every valid kind"""
    img, root, info = ib.build_tall(2, "middle", True)
    per_kind, per_bad = ib.soil_sizes(n)
    assert per_kind >= 17 and per_bad >= 1
    keys = ib.soil_keys(info, per_kind, per_bad)
    pages, soil = ib.soil_pages(n, keys, seed=n, first_page=img.size // ib.PAGE)
    assert pages.shape == (n, ib.PAGE)
    assert soil["leaf_pages"].size == max(n - 1, 1)
    assert sweep_leaf(pages)[soil["leaf_pages"]].all()
    for kind in VALID_KINDS:
        assert live_buckets(info["keys"], soil, 0, 64, kind).size >= 16, kind
        for p in soil["leaf_pages"]:
            assert ((soil["slots"]["page"] == p) & (soil["slots"]["kind"] == kind)).any(), (p, kind)
    b = OracleTree(image=ib.with_soil(img, pages), root_ptr=root)
    rc, shape = b.check()
    assert rc == 0 and shape["leaves"] == info["leaves"], (rc, shape)
    b.close()
