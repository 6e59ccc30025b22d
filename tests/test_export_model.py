"""The export model (tests/export_model.py) against the CPU oracle, without a
GPU: on every image the model's whole-tree export equals
OracleTree(image=...).dump() sorted by key, and its ranges are slices of it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bulk_model as bm  # noqa: E402
import export_model as em  # noqa: E402
import image_builder as ib  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402

U64 = np.uint64
KEY_MAX = (1 << 64) - 1


def oracle_sorted(img, root):
    orc = OracleTree(image=np.array(img, dtype=np.uint8), root_ptr=root)
    rc, shape = orc.check()
    k, v = orc.dump()
    orc.close()
    o = np.argsort(k, kind="stable")
    return rc, shape, k[o], v[o]


def assert_model(img, root, what):
    rc, shape, ok, ov = oracle_sorted(img, root)
    assert rc == 0, (what, rc)
    k, v = em.export(img, root)
    assert np.array_equal(k, ok) and np.array_equal(v, ov), (what, k.size, ok.size)
    # ranges are slices of the whole
    rng = np.random.default_rng(k.size)
    ends = [0, 1, KEY_MAX - 1, KEY_MAX]
    if k.size:
        ends += [int(k[0]), int(k[-1]), int(k[k.size // 2]), int(k[k.size // 2]) + 1]
    ends += [int(x) for x in rng.integers(0, KEY_MAX, 6, dtype=np.uint64)]
    for lo in ends:
        for hi in ends:
            rk, rv = em.export(img, root, lo, hi)
            a = np.searchsorted(k, U64(lo), side="left")
            b = max(a, np.searchsorted(k, U64(hi), side="right")) if lo != KEY_MAX else a
            assert np.array_equal(rk, k[a:b]) and np.array_equal(rv, v[a:b]), (what, lo, hi)
    return shape, k, v


@pytest.mark.parametrize("n,lf,inf", bm.SHAPES)
def test_model_on_the_loaded_shapes(n, lf, inf):
    keys = bm.shape_keys(n, bm.shape_kind(n, lf, inf))
    vals = bm.shape_vals(keys)
    img, root, pl = bm.build(keys, vals, lf, inf)
    shape, k, v = assert_model(img, root, (n, lf, inf))
    assert np.array_equal(k, keys) and np.array_equal(v, vals)


@pytest.mark.parametrize("level", [1, 3, 7])
def test_model_on_tall_images(level):
    img, root, info = ib.build_tall(level, "middle", level != 7)
    shape, k, v = assert_model(img, root, level)
    assert np.array_equal(k, info["keys"]) and np.array_equal(v, info["vals"])


def test_model_on_the_entry_states():
    img, root, info = ib.build_entry_states()
    shape, k, v = assert_model(img, root, "entry states")
    assert k.size == info["n_valid"] == 478
    assert np.array_equal(k, info["keys"]) and np.array_equal(v, info["vals"])
    # the structural check counts the torn entries as well
    assert shape["keys"] == info["n_valid"] + info["n_torn"] == 503


def test_model_on_an_oracle_grown_tree():
    rng = np.random.default_rng(12)
    orc = OracleTree(1 << 24)
    keys = np.unique(rng.integers(1, KEY_MAX - 1, 9000, dtype=np.uint64))
    keys = keys[rng.permutation(keys.size)]
    orc.apply_batch(keys, keys ^ U64(0x77))
    dele = keys[::3]
    orc.apply_batch(dele, np.zeros(dele.size, dtype=U64))
    over = keys[1::3][:1000]
    orc.apply_batch(over, over ^ U64(0x99))
    img, root = orc.image(), orc.root_ptr
    assert orc.root_level >= 1
    orc.close()
    shape, k, v = assert_model(img, root, "grown")
    assert k.size == keys.size - dele.size


@pytest.mark.parametrize("in_root,in_level1", [(True, True), (True, False), (False, True)])
def test_model_with_separators_dropped(in_root, in_level1):
    """The root's last_index decremented and / or every level-1 page's: the
    last child of each such page hangs on its left sibling alone.  The oracle
    accepts the image (check rc 0, 40 leaves) and finds and dumps all 478
    keys; so does the model."""
    base, root, info = ib.build_entry_states()
    img = em.drop_last_separators(base, root, in_root=in_root, in_level1=in_level1)
    assert not np.array_equal(img, base)
    rc, shape, ok, ov = oracle_sorted(img, root)
    assert rc == 0 and shape["leaves"] == 40, (rc, shape)
    assert np.array_equal(ok, info["keys"]) and ok.size == 478
    orc = OracleTree(image=img.copy(), root_ptr=root)
    v, f = orc.search_batch(info["keys"])
    orc.close()
    assert f.all() and np.array_equal(v, info["vals"])
    shape, k, v = assert_model(img, root, "dropped")
    assert np.array_equal(k, info["keys"]) and np.array_equal(v, info["vals"])
