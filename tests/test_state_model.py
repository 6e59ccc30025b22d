"""The side-state model (tests/state_model.py) on built images, without a GPU.

side_expected() of an image shows no violation; one changed byte of the
expected lines or occupancy bounds shows exactly the violation that byte
stands for, at its page and slot; and seeded random single-byte changes are
each reported, or neutral by a rule this file decides from the image alone."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import image_builder as ib  # noqa: E402
import state_model as sm  # noqa: E402

U64 = np.uint64
EXTRA = 5  # lines dumped past next_page


def soiled(img, info, n, seed):
    per_kind, per_bad = ib.soil_sizes(n)
    soil, _ = ib.soil_pages(n, ib.soil_keys(info, per_kind, per_bad), seed,
                            first_page=img.size // ib.PAGE)
    return ib.with_soil(img, soil)


@functools.lru_cache(maxsize=None)
def image(name):
    if name.startswith("tall"):
        img, root, info = ib.build_tall(int(name[4:]), "middle", int(name[4:]) < 7)
    else:
        img, root, info = ib.build_entry_states()
        if name == "entries_soil":
            img = soiled(img, info, 6, 21)
    img.setflags(write=False)
    return img, root


IMAGES = ["tall1", "tall3", "tall7", "entries", "entries_soil"]


def slots_of(img, page):
    return sm._slots(img.reshape(-1, ib.PAGE)[page:page + 1])


def test_key_fp_is_the_documented_hash():
    ks = [0, 1, 64, 0x9E3779B97F4A7C15, (1 << 64) - 2, 12345678901234567]
    want = [((k * 0x9E3779B97F4A7C15) % (1 << 64)) >> 56 or 1 for k in ks]
    assert sm.key_fp(np.array(ks, dtype=U64)).tolist() == want
    assert sm.key_fp(np.array([0], dtype=U64))[0] == 1  # 0 read as 1


@pytest.mark.parametrize("name", IMAGES)
def test_expected_state_has_no_violation(name):
    img, root = image(name)
    n = img.size // ib.PAGE
    lines = sm.side_expected(img, root, n + EXTRA)
    _, leaf = sm.reached_leaves(img, root)
    assert leaf.sum() > 0 and (lines[:n, sm.SUM_OFF_TAG] == sm.SUM_LEAF).sum() == leaf.sum()
    assert not lines[n:].any()
    for hw in (sm.hw_tight(img, root, n + EXTRA), np.full(n + EXTRA, 0xFF, dtype=np.uint8)):
        assert sm.side_violations(img, root, lines, hw, n) == []
    if name == "entries_soil":  # the soil's leaves look like leaves and get no line
        assert not lines[n - 6:n].any()
        assert ib.sweep_leaf(img.reshape(-1, ib.PAGE)[n - 6:]).sum() == 5


def test_expected_lines_of_the_entry_states():
    """torn entries carry their key's fingerprint; deleted slots and stale
    copies carry 0"""
    img, root, info = ib.build_entry_states()
    lines = sm.side_expected(img, root, img.size // ib.PAGE)
    s = info["slots"]
    fp = lines[s["page"], sm.SUM_OFF_FP + s["slot"]]
    holds = (s["kind"] == ib.VALID) | (s["kind"] == ib.VALID15) | (s["kind"] == ib.TORN)
    assert (s["kind"] == ib.TORN).sum() == 25 and (s["kind"] == ib.STALE_COPY).sum() >= 4
    assert np.array_equal(fp[holds], sm.key_fp(s["key"][holds]))
    assert not fp[~holds].any()
    assert int((lines[:, sm.SUM_OFF_FP:sm.SUM_OFF_FP + 54] != 0).sum()) == int(holds.sum())


def targets():
    """(kind, which array, page, byte, new value or None for "any other",
    expected slot) of one single-byte change per kind, on the soiled
    entry-states image"""
    img, root = image("entries_soil")
    n = img.size // ib.PAGE
    reached, leaf = sm.reached_leaves(img, root)
    pages = np.nonzero(leaf)[0]
    internal = int(np.nonzero(reached & ~leaf)[0][0])
    soil_leaf = n - 1
    assert not reached[soil_leaf]
    k, v = slots_of(img, int(pages[3]))
    held, free = int(np.nonzero(v[0] != 0)[0][0]), int(np.nonzero(v[0] == 0)[0][0])
    top = int(np.nonzero(v[0] != 0)[0][-1])
    return [
        (sm.UNTAGGED_LEAF, "lines", int(pages[0]), sm.SUM_OFF_TAG, 0, -1),
        (sm.UNTAGGED_LEAF, "lines", int(pages[1]), sm.SUM_OFF_TAG, 0xA4, -1),
        (sm.TAGGED_OTHER, "lines", internal, sm.SUM_OFF_TAG, sm.SUM_LEAF, -1),
        (sm.TAGGED_OTHER, "lines", soil_leaf, sm.SUM_OFF_TAG, sm.SUM_LEAF, -1),
        (sm.HIGHEST, "lines", int(pages[2]), sm.SUM_OFF_HIGHEST + 6, None, -1),
        (sm.FP_MISSING, "lines", int(pages[3]), sm.SUM_OFF_FP + held, None, held),
        (sm.FP_MISSING, "lines", int(pages[3]), sm.SUM_OFF_FP + held, 0, held),
        (sm.FP_STALE, "lines", int(pages[3]), sm.SUM_OFF_FP + free, 1, free),
        (sm.HW_HIDES, "hw", int(pages[3]), 0, top, top),
        (sm.LINE_PAST_END, "lines", n + 2, 17, 1, 17),
        (sm.LINE_PAST_END, "lines", n, sm.SUM_OFF_TAG, sm.SUM_LEAF, sm.SUM_OFF_TAG),
    ]


@pytest.mark.parametrize("case", range(11))
def test_one_changed_byte_is_one_violation(case):
    kind, which, page, byte, new, slot = targets()[case]
    img, root = image("entries_soil")
    n = img.size // ib.PAGE
    lines = sm.side_expected(img, root, n + EXTRA)
    hw = sm.hw_tight(img, root, n + EXTRA)
    arr = lines[page] if which == "lines" else hw[page:page + 1]
    old = int(arr[byte])
    arr[byte] = (old ^ 0x5A) if new is None else new
    assert int(arr[byte]) != old
    assert sm.side_violations(img, root, lines, hw, n) == [(kind, page, slot)]


def test_every_kind_has_a_target():
    assert {t[0] for t in targets()} == set(sm.SIDE_KINDS) and len(targets()) == 11


@pytest.mark.parametrize("name", ["tall3", "entries_soil"])
def test_random_single_byte_changes(name):
    """Every change of one byte of a reached leaf's line (bytes 0..62: byte
    63 belongs to no field) or occupancy bound is reported at that page, or
    is neutral: a new bound that is 0xFF or still >= 1 + the last slot with a
    value, which this test reads from the page itself."""
    img, root = image(name)
    n = img.size // ib.PAGE
    pg = img.reshape(-1, ib.PAGE)
    lines0 = sm.side_expected(img, root, n)
    hw0 = sm.hw_tight(img, root, n)
    _, leaf = sm.reached_leaves(img, root)
    pages = np.nonzero(leaf)[0]
    rng = np.random.default_rng([7, len(name)])
    seen = {k: 0 for k in sm.SIDE_KINDS}
    neutral = 0
    for i in range(600):
        p = int(rng.choice(pages))
        lines, hw = lines0.copy(), hw0.copy()
        if i % 3 == 2:
            new = int(rng.integers(0, 256))
            if new == hw0[p]:
                continue
            hw[p] = new
            need = 0
            for s in range(54):  # from the page's bytes: the value of slot s
                at = ib.OFF_RECORDS + ib.LEAF_ENTRY * s + 9
                if pg[p, at:at + 8].any():
                    need = s + 1
            got = sm.side_violations(img, root, lines, hw, n)
            if new == 0xFF or new >= need:
                neutral += 1
                assert got == [], (p, new, need, got)
            else:
                assert got and all(g[:2] == (sm.HW_HIDES, p) and new <= g[2] < need for g in got), \
                    (p, new, need, got)
                assert (sm.HW_HIDES, p, need - 1) in got
                seen[sm.HW_HIDES] += 1
            continue
        # the header bytes and the fingerprints in turn, held slots as often as free ones
        b = int(rng.integers(0, 9)) if i % 3 == 0 else int(rng.integers(9, 63))
        held = np.nonzero(lines0[p, 9:63])[0]
        if i % 6 == 1 and held.size:
            b = 9 + int(rng.choice(held))
        new = int(rng.integers(0, 256))
        if new == lines0[p, b]:
            continue
        lines[p, b] = new
        got = sm.side_violations(img, root, lines, hw, n)
        assert len(got) == 1 and got[0][1] == p, (p, b, new, got)
        if b < 8:
            assert got[0] == (sm.HIGHEST, p, -1)
        elif b == 8:
            assert got[0] == (sm.UNTAGGED_LEAF, p, -1)
        else:
            assert got[0][2] == b - 9 and got[0][0] in (sm.FP_MISSING, sm.FP_STALE)
            at = ib.OFF_RECORDS + ib.LEAF_ENTRY * (b - 9) + 9
            assert (got[0][0] == sm.FP_MISSING) == bool(pg[p, at:at + 8].any())
        seen[got[0][0]] += 1
    assert neutral > 20 and all(seen[k] > 5 for k in (sm.HIGHEST, sm.UNTAGGED_LEAF, sm.FP_MISSING,
                                                       sm.FP_STALE, sm.HW_HIDES)), (neutral, seen)
