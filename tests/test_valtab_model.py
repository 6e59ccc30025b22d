"""The bucket table's host model (tests/valtab_model.py) on a hand-built
image: a correct image is clean, and each single wrong field is reported."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import valtab_model as vm  # noqa: E402

U64 = np.uint64
LO, SHIFT, N = 1 << 20, 8, 16  # bucket b: keys [LO + 256 b, LO + 256 (b + 1))


def image():
    """(buckets, keys, values): bucket 0 empty, 1 holds one key, 2 holds 8,
    3 holds 9 keys and is dead, 4 holds 3 keys around a freed slot, 5 is dead
    though it holds 2 keys (it overflowed before deletes)."""
    per = {1: [5], 2: [0, 1, 2, 3, 4, 5, 6, 255], 3: list(range(10, 19)), 4: [7, 9, 200], 5: [1, 2]}
    keys, vals = [], []
    b = np.zeros((N, 16), dtype=U64)
    for bi, offs in per.items():
        for j, o in enumerate(offs):
            k = LO + 256 * bi + o
            keys.append(k)
            vals.append(2 * k + 1)
            if bi == 4 and j >= 1:
                j += 1  # slot 1 was deleted: key and value 0
            if bi not in (3, 5):
                b[bi, 2 * j], b[bi, 2 * j + 1] = k, 2 * k + 1
    # dead buckets: the marker, anything behind it
    b[3, 0] = vm.KEY_MAX
    b[3, 1:] = 0x1234
    b[5, 0] = vm.KEY_MAX
    return b, np.array(keys, dtype=U64), np.array(vals, dtype=U64)


def test_clean_image_is_clean():
    b, k, v = image()
    assert vm.check(b, LO, SHIFT, k, v) == []
    assert vm.dead(b).tolist() == [i in (3, 5) for i in range(N)]
    assert vm.counts(k, LO, SHIFT, N)[:6].tolist() == [0, 1, 8, 9, 3, 2]


def _kinds(bad):
    return {(kind, bk) for kind, bk in bad}


def test_each_wrong_field_is_reported():
    b0, k, v = image()

    def run(edit):
        b = b0.copy()
        edit(b)
        return _kinds(vm.check(b, LO, SHIFT, k, v))

    # a wrong value
    def f(b): b[2, 3] += U64(1)
    assert ("wrong", 2) in run(f)
    # a wrong key (same bucket's range, not stored)
    def f(b): b[4, 0] += U64(1)
    assert ("wrong", 4) in run(f)
    # a stored key missing (its value cleared)
    def f(b): b[2, 15] = 0
    assert ("wrong", 2) in run(f)
    # a deleted key still live
    def f(b): b[4, 2], b[4, 3] = LO + 256 * 4 + 77, 5
    assert ("wrong", 4) in run(f)
    # a freed slot that kept its key: no writer could claim it again
    def f(b): b[4, 2] = LO + 256 * 4 + 77
    assert run(f) == {("stale", 4)}
    # a live key twice
    def f(b): b[1, 2], b[1, 3] = b[1, 0], b[1, 1]
    r = run(f)
    assert ("duplicate", 1) in r and ("wrong", 1) in r
    # a live key of another bucket's range
    def f(b): b[0, 0], b[0, 1] = b[1, 0], b[1, 1]
    r = run(f)
    assert ("misplaced", 0) in r and ("wrong", 0) in r
    # an overflowed bucket without its marker
    def f(b): b[3, 0] = LO + 256 * 3 + 10
    assert ("unmarked", 3) in run(f)
    # the marker anywhere but slot 0's key is no marker
    def f(b):
        b[3, 0] = LO + 256 * 3 + 10
        b[3, 2] = vm.KEY_MAX
    assert ("unmarked", 3) in run(f)
    # a marker on a bucket that fits is allowed (bucket 5), and hides nothing else
    def f(b): b[1, 0] = vm.KEY_MAX
    assert run(f) == set()


def test_stored_set_changes_are_reported():
    b, k, v = image()
    # the oracle gained a key the table does not hold
    k2 = np.append(k, U64(LO + 256 * 0 + 3))
    v2 = np.append(v, U64(9))
    assert ("wrong", 0) in _kinds(vm.check(b, LO, SHIFT, k2, v2))
    # the oracle lost one (deleted) that the table still shows live
    assert ("wrong", 1) in _kinds(vm.check(b, LO, SHIFT, k[1:], v[1:]))
    # keys outside the table's range, and key 0, are nobody's
    k3 = np.append(k, [U64(LO - 1), U64(LO + 256 * N), U64(0)])
    v3 = np.append(v, [U64(1), U64(1), U64(1)])
    assert vm.check(b, LO, SHIFT, k3, v3) == []
