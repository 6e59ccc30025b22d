"""The numpy model of the bulk loader's tree (tests/bulk_model.py) against the
CPU oracle, without a GPU: the images the GPU tests compare byte for byte are
themselves sound trees with the planned shape and the given contents, and
they take later inserts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bulk_model as bm  # noqa: E402

U64 = np.uint64
KEY_MAX = bm.KEY_MAX


def test_plan_by_hand():
    assert bm.plan(0) == {"pages": 1, "root_level": 0, "level_pages": [1]}
    assert bm.plan(53, 53, 60) == {"pages": 1, "root_level": 0, "level_pages": [1]}
    assert bm.plan(54, 53, 60) == {"pages": 3, "root_level": 1, "level_pages": [2, 1]}
    assert bm.plan(53 * 61, 53, 60) == {"pages": 62, "root_level": 1, "level_pages": [61, 1]}
    assert bm.plan(53 * 61 + 1, 53, 60) == {"pages": 65, "root_level": 2,
                                            "level_pages": [62, 2, 1]}
    assert bm.plan(2187, 1, 2)["level_pages"] == [3 ** (7 - i) for i in range(8)]
    assert bm.plan(1000, 1, 2)["level_pages"] == [1000, 334, 112, 38, 13, 5, 2, 1]
    assert bm.plan(5000) == {"pages": 139 + 4 + 1, "root_level": 2, "level_pages": [139, 4, 1]}
    for bad in ((2188, 1, 2), (10, 54, 0), (10, 0, 1), (10, 0, 61)):
        with pytest.raises(ValueError):
            bm.plan(*bad)


def test_the_deal_is_even_and_gives_every_internal_page_two_children():
    for items, pages in ((0, 1), (5, 5), (7, 3), (1000, 334), (61, 1), (62, 2)):
        first = bm.deal(items, pages)
        cnt = np.diff(first)
        assert first[0] == 0 and first[-1] == items and cnt.max() - cnt.min() <= 1
        assert np.all(cnt[:-1] >= cnt[1:])  # the larger shares first
    for inf in (2, 3, 40, 60):
        for below in range(2, 400):
            cnt = np.diff(bm.deal(below, -(-below // (inf + 1))))
            assert cnt.min() >= 2 and cnt.max() <= inf + 1, (inf, below)


@pytest.mark.parametrize("n,lf,inf", bm.SHAPES)
def test_model_image_is_a_sound_tree(oracle, n, lf, inf):
    keys = bm.shape_keys(n, bm.shape_kind(n, lf, inf))
    vals = bm.shape_vals(keys)
    img, root, pl = bm.build(keys, vals, lf, inf)
    assert img.size == (pl["pages"] + 1) * bm.PAGE and not img[:bm.PAGE].any()
    assert root == 1 << 26
    orc = oracle.OracleTree(image=img, root_ptr=root, spare_bytes=4 << 20)
    rc, shape = orc.check()
    assert rc == 0, rc
    assert shape == dict(bm.counts(pl, n), height=pl["root_level"] + 1)
    assert orc.root_level == pl["root_level"]
    # every key with its value; misses at key +- 1
    v, f = orc.search_batch(keys)
    assert f.all() and np.array_equal(v, vals)
    near = np.concatenate([keys + U64(1), keys - U64(1)]) if n else np.array([0, 5], dtype=U64)
    near = near[~np.isin(near, keys) & (near != U64(KEY_MAX))]
    v, f = orc.search_batch(near)
    assert not f.any() and not v.any()
    got, cnt = orc.range_query(0, KEY_MAX - 1, cap=max(n, 1))
    assert cnt == n and np.array_equal(got, vals)  # key order: slots ascend inside a leaf
    # the tree takes inserts
    rng = np.random.default_rng([7, n])
    new = rng.integers(1, KEY_MAX - 1, 260, dtype=np.uint64)
    new = np.unique(new[~np.isin(new, keys)])[:200]
    new = new[rng.permutation(new.size)]
    assert new.size == 200
    orc.apply_batch(new, new ^ U64(0x7777))
    rc, shape = orc.check()
    assert rc == 0 and shape["keys"] == n + 200, (rc, shape)
    v, f = orc.search_batch(np.concatenate([keys, new]))
    assert f.all() and np.array_equal(v, np.concatenate([vals, new ^ U64(0x7777)]))
    orc.close()


def test_model_with_a_node_id(oracle):
    keys = bm.shape_keys(300, "spread")
    img, root, pl = bm.build(keys, bm.shape_vals(keys), 7, 3, node_id=3)
    assert root == (1 << 26) | 3
    orc = oracle.OracleTree(image=img, root_ptr=root, node_id=3)
    rc, shape = orc.check()
    assert rc == 0 and shape["keys"] == 300 and shape["height"] == pl["root_level"] + 1
    orc.close()
