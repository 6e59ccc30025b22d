"""The host model of the insert ordering (tests/order_model.py) checked on
its own: order() against a dict applied op by op, plan() on hand-made inputs
at each threshold, and the batches of tests/test_gpu_order.py against the
paths they are built for.  No GPU; the thresholds are the library's compiled
constants (sherman_amd.order_limits(), host code only).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import order_cases as oc  # noqa: E402
import order_model as om  # noqa: E402
import sherman_amd as shm  # noqa: E402

U64 = np.uint64
KEY_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def lim():
    return shm.order_limits()


def test_limits_are_the_documented_ones(lim):
    """the constants of the path table in DESIGN.md ("The ordering's paths")"""
    assert lim == {"tile": 2048, "max_tiles": 512, "uniq_cap": 6144, "sub_cap": 64,
                   "coarse": 256, "fine": 256}


@pytest.mark.parametrize("seed", range(8))
def test_order_equals_a_dict_applied_op_by_op(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 400))
    keys = rng.integers(0, 60, n, dtype=np.uint64) * U64(0x0123456789ABCDEF)  # wraps past 2^63
    if n > 3:
        keys[1] = KEY_MAX - 1
        keys[2] = 0
    vals = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    vals[rng.random(n) < 0.3] = 0
    d = {}
    for k, v in zip(keys.tolist(), vals.tolist()):
        d[k] = v
    uk, uv, dk = om.order(keys, vals)
    assert uk.tolist() == sorted(k for k, v in d.items() if v)
    assert uv.tolist() == [d[k] for k in uk.tolist()]
    assert dk.tolist() == sorted(k for k, v in d.items() if not v)
    # apply: a stored image updated by the chunk
    sk = np.unique(rng.integers(0, 60, 30, dtype=np.uint64) * U64(0x0123456789ABCDEF))
    sv = sk + U64(5)
    img = dict(zip(sk.tolist(), sv.tolist()))
    for k, v in d.items():
        if v:
            img[k] = v
        else:
            img.pop(k, None)
    ak, av = om.apply(sk, sv, uk, uv, dk)
    assert ak.tolist() == sorted(img) and av.tolist() == [img[k] for k in sorted(img)]


def test_rel_key_clamps_as_the_device_does():
    lo = 1 << 40
    k = np.array([0, lo - 1, lo, lo + 1, lo + (1 << 24) - 1, lo + (1 << 24), KEY_MAX - 1],
                 dtype=U64)
    r = om.rel_key(k, lo, 24).tolist()
    assert r == [0, 0, 0, 1 << 40, ((1 << 24) - 1) << 40, KEY_MAX, KEY_MAX]
    assert om.rel_key(k, lo, 64).tolist() == k.tolist()
    assert om.rel_key(k, lo, 1).tolist() == [0, 0, 0, 1 << 63, KEY_MAX, KEY_MAX, KEY_MAX]


def test_plan_mode_and_groups_at_the_tile_limit(lim):
    T, MT = lim["tile"], lim["max_tiles"]
    z = lambda n: np.zeros(n, dtype=U64)  # noqa: E731
    p = om.plan(z(T * MT), 0, 64, lim)
    assert (p.mode, p.tiles, p.groups, p.coarse_tiles) == ("tile", MT, 1, 0)
    p = om.plan(z(T * MT + 1), 0, 64, lim)
    assert (p.mode, p.tiles, p.groups, p.coarse_tiles, p.last_groups) == \
        ("coarse", MT + 1, 2, MT // 2 + 1, 1)
    assert p.cnt[0] == MT + 1 and p.distinct[0] == 1 and p.path[0] == "rank"
    p = om.plan(z(3 * T * MT + 77), 0, 64, lim)
    assert (p.groups, p.coarse_tiles, p.last_groups) == (4, 385, 1)
    assert om.plan(z(0), 0, 64, lim).tiles == 0


def test_plan_bin_paths_at_the_thresholds(lim):
    T, CAP, SUB = lim["tile"], lim["uniq_cap"], lim["sub_cap"]
    B = 0x21
    # CAP distinct keys, 24 per sub-bucket: the rank finish; one more op: radix
    k = (U64(B) << U64(56)) | (np.arange(CAP, dtype=U64) % U64(256) << U64(48)) | \
        np.arange(CAP, dtype=U64)
    p = om.plan(k, 0, 64, lim)
    assert p.cnt[B] == CAP and p.sub_max[B] == CAP // 256 and p.path[B] == "rank"
    p = om.plan(np.concatenate([k, k[:1]]), 0, 64, lim)  # a repeat in a fourth tile
    assert p.cnt[B] == CAP + 1 and p.distinct[B] == CAP and p.path[B] == "radix"
    assert p.radix_bytes[B] == (0, 1, 6)  # 6144 < 2^16 low values, the fine byte
    # a repeat inside one tile is no survivor
    p = om.plan(np.concatenate([k[:-1], k[-2:-1]]), 0, 64, lim)
    assert p.cnt[B] == CAP - 1 and p.path[B] == "rank"
    # SUB keys in one sub-bucket: rank; SUB + 1: bitonic, the network's width
    s = (U64(B) << U64(56)) | np.arange(SUB + 1, dtype=U64)
    assert om.plan(s[:SUB], 0, 64, lim).path[B] == "rank"
    p = om.plan(s, 0, 64, lim)
    assert p.path[B] == "bitonic" and p.bitonic_m[B] == 128
    p = om.plan((U64(B) << U64(56)) | np.arange(4097, dtype=U64), 0, 64, lim)
    assert p.path[B] == "bitonic" and p.bitonic_m[B] == 8192
    # padding is no op
    kp = np.concatenate([s[:SUB], np.full(T, KEY_MAX, dtype=U64)])
    p = om.plan(kp, 0, 64, lim, skip_pad=True)
    assert p.cnt.sum() == SUB and p.tiles == 2 and p.path[255] == "empty"


def test_plan_bins_by_the_hint(lim):
    lo = 1 << 40
    k = np.array([0, lo - 1, lo, lo + (1 << 23), lo + (1 << 24), KEY_MAX - 1], dtype=U64)
    p = om.plan(k, lo, 24, lim)
    assert p.cnt[0] == 3 and p.cnt[128] == 1 and p.cnt[255] == 2 and p.cnt.sum() == 6
    p = om.plan(k, 0, 64, lim)
    assert p.cnt[0] == 5 and p.cnt[255] == 1


def test_bin_overflow_test_takes_the_paths_its_docstring_names(lim):
    """tests/test_gpu_parity.py::test_insert_bin_overflow_reorders: its
    batches of 12000 and 16000 keys sort their bin by radix in two passes,
    the 5000-key batch takes the LDS bitonic finish"""
    rng = np.random.default_rng(11)
    got = []
    for n in (12000, 5000, 16000):
        ks = (np.arange(1, n + 1, dtype=U64) * U64(3))[rng.permutation(n)]
        ks = np.concatenate([ks, ks[: n // 10]])
        rng.random(ks.size)  # the test's delete draw
        p = om.plan(ks[:1 << 14], 0, 64, lim)  # the first chunk (max_batch 2^14)
        got.append((p.path[0], p.radix_bytes.get(0), p.bitonic_m.get(0)))
    assert got == [("radix", (0, 1), None), ("bitonic", None, 8192), ("radix", (0, 1), None)]


@pytest.mark.parametrize("name", list(oc.BUILDERS))
def test_gpu_cases_take_their_paths(lim, name):
    c = oc.BUILDERS[name](lim)
    assert c.name == name and c.keys.size == c.vals.size
    assert not (c.keys == U64(KEY_MAX)).any()
    lo, bits = c.hint or (0, 64)
    c.expect(om.plan(c.keys, lo, bits, lim))
    uk, uv, dk = om.order(c.keys, c.vals)
    if c.counts is not None:
        assert (uk.size, dk.size) == c.counts
    if c.keys.size > lim["tile"]:
        # the same key in different tiles, and a delete that is the later op
        tid = np.arange(c.keys.size) // lim["tile"]
        o = np.argsort(c.keys, kind="stable")
        same = c.keys[o][1:] == c.keys[o][:-1]
        assert (same & (tid[o][1:] != tid[o][:-1])).any()


def test_every_path_of_the_table_is_planned(lim):
    """each row of the path table, each threshold from both sides and both
    parities of the radix pass count are asserted by some case's expect()"""
    names = set(oc.BUILDERS)
    for need in ("size_2048", "size_2049", f"switch_{1 << 20}", f"switch_{(1 << 20) + 1}",
                 f"switch_{3 * (1 << 20) + 77}", "coarse_big_bin", "bin_cap_at", "bin_cap_over",
                 "bin_cap_repeat", "sub_64", "sub_65", "sub_full_bitonic", "radix_0", "radix_7",
                 "radix_01234567", "radix_036", "hint_1", "hint_24_coarse"):
        assert need in names
    passes = {len(k) - len("radix_") for k in names if k.startswith("radix_")}
    assert {p % 2 for p in passes} == {0, 1}
