"""classify_outcome (tests/arena_model.py) on hand-made cases, and the sizes
the arena tests rely on for the image of root level 2, under the CPU oracle.

The before-or-after rule of a failed chunk is permissive by design; these
cases show what it still rejects, so it cannot hide a failure.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena_model as am  # noqa: E402
import image_builder as ib  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402

U64 = np.uint64


def kv(d):
    k = np.array(list(d), dtype=U64)
    return k, np.array([d[int(x)] for x in k], dtype=U64)


# keys 10..50 stored; the chunk adds 60 and 70, overwrites 20, deletes 30
BEFORE = {10: 1, 20: 2, 30: 3, 40: 4, 50: 5}
AFTER = {10: 1, 20: 22, 40: 4, 50: 5, 60: 6, 70: 7}


def test_accepts_nothing_applied_and_all_applied():
    got = am.classify_outcome(kv(BEFORE), kv(AFTER), kv(BEFORE), [])
    assert got == {"applied": 0, "unapplied": 4, "new_stored": 0, "new_not_stored": 2}
    got = am.classify_outcome(kv(BEFORE), kv(AFTER), kv(AFTER), [20, 30, 60, 70])
    assert got == {"applied": 4, "unapplied": 0, "new_stored": 2, "new_not_stored": 0}


def test_accepts_a_mix_and_counts_it():
    T = dict(BEFORE)
    T[60] = 6  # one new key stored
    del T[30]  # the delete applied
    got = am.classify_outcome(kv(BEFORE), kv(AFTER), kv(T), [30])
    assert got == {"applied": 2, "unapplied": 2, "new_stored": 1, "new_not_stored": 1}


@pytest.mark.parametrize("change,kind,key", [
    ({20: 99}, "third_value", 20),    # neither the old nor the new value
    ({60: 99}, "third_value", 60),    # a new key with another value
    ({40: None}, "untouched", 40),    # a key the chunk does not touch is lost
    ({40: 44}, "untouched", 40),      # ... or changed
    ({80: 8}, "extra", 80),           # a key in neither state
])
def test_rejects(change, kind, key):
    for base in (BEFORE, AFTER):
        T = dict(base)
        for k, v in change.items():
            if v is None:
                T.pop(k, None)
            else:
                T[k] = v
        with pytest.raises(am.OutcomeError) as e:
            am.classify_outcome(kv(BEFORE), kv(AFTER), kv(T), [])
        assert e.value.kind == kind and list(e.value.keys) == [key], e.value


def test_rejects_an_unapplied_must_apply_op():
    for key in (20, 30, 60):  # an overwrite, a delete, a new key
        with pytest.raises(am.OutcomeError) as e:
            am.classify_outcome(kv(BEFORE), kv(AFTER), kv(BEFORE), [key])
        assert e.value.kind == "must_apply" and list(e.value.keys) == [key]
    # a must_apply op that changes nothing (the delete of an absent key)
    am.classify_outcome(kv(BEFORE), kv(AFTER), kv(BEFORE), [90])


def test_rejects_malformed_contents():
    k, v = kv(BEFORE)
    with pytest.raises(AssertionError):
        am.classify_outcome((np.append(k, k[:1]), np.append(v, v[:1])), kv(AFTER), kv(BEFORE), [])
    with pytest.raises(AssertionError):
        am.classify_outcome(kv(BEFORE), kv(AFTER), (k, np.zeros_like(v)), [])


@pytest.mark.parametrize("path", ["left", "middle", "right"])
def test_hot_chunk_on_the_level_2_image(path):
    """The image the exact arenas are sized from: a page per leaf and internal
    page after the superblock, and a hot chunk that takes at least a page per
    level and the new root (the oracle's count; the GPU's own count sizes the
    sweep)."""
    img, root, info = ib.build_tall(2, path, True)
    assert info["root_level"] == 2
    assert img.nbytes == (1 + info["leaves"] + info["internal"]) * ib.PAGE
    orc = OracleTree(image=img, root_ptr=root, spare_bytes=64 * ib.PAGE)
    before = orc.dump()
    keys, vals = am.hot_chunk(info)
    orc.apply_batch(keys, vals)
    rc, shape = orc.check()
    assert rc == 0 and shape["height"] == 4
    need = orc.image().nbytes // ib.PAGE - img.nbytes // ib.PAGE
    assert need >= info["root_level"] + 2, need
    # every op outside the hot leaf changes something (must_apply is not vacuous)
    after = orc.dump()
    outside = keys[(keys < U64(info["hot_lo"])) | (keys >= U64(info["hot_hi"]))]
    got = am.classify_outcome(before, after, after, outside)
    assert got["applied"] == 60 and got["new_stored"] == 40
    with pytest.raises(am.OutcomeError):
        am.classify_outcome(before, after, before, outside)
    orc.close()
