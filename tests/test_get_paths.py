"""The model of the get's answering path (tests/get_paths.py) on hand-built
dumps: every rule of classify() decides at least one key here, and each
single change of one field moves exactly the keys it should."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dir_model as dm  # noqa: E402
import get_paths as gp  # noqa: E402
import valtab_model as vm  # noqa: E402

U64 = np.uint64
KEY_MAX = (1 << 64) - 1
T, V, L = gp.TABLE, gp.VALUE, gp.LEAF


def u64s(xs):
    return np.array([int(x) & KEY_MAX for x in xs], dtype=U64)


def cw(flags, np_=0, nl=1):
    return flags | (np_ << 16) | nl


VAL = dm.VALS | dm.PAIRS


def wide():
    """The whole key space: four buckets of 2^62 keys (bucket 1 dead) over
    eight prefixes of 2^61.  Prefixes 0, 2, 4 hold one key inline, 7 two keys
    in two leaves, 6 carries the flag beside FIX (not usable), 1, 3, 5 are
    plain pair entries of three keys.  Probes: key 0, KEY_MAX and
    (p << 61) + 5 of every prefix p."""
    b = np.zeros((4, 16), dtype=U64)
    b[1, 0] = vm.KEY_MAX
    table = (b, {"lo": 0, "shift": 62, "trusted": True})
    ent = np.zeros((8, 16), dtype=np.uint32)
    for p in (0, 2, 4):
        ent[p, 7] = cw(VAL, 1)
    ent[7, 7] = cw(VAL, 2, nl=2)
    ent[6, 7] = cw(VAL | dm.FIX, 1)
    for p in (1, 3, 5):
        ent[p, 7] = cw(dm.PAIRS, 3)
    directory = (ent, {"lo": 0, "shift": 61, "form": "pairs"})
    flags = {"exact": True, "page_check": False}
    keys = u64s([0, KEY_MAX] + [(p << 61) + 5 for p in range(8)])
    return keys, table, directory, flags


#            key 0, KEY_MAX, p0 p1 p2 p3 p4 p5 p6 p7
WIDE_BASE = [V, L, T, T, V, L, T, T, T, T]
# with every key left to the directory
WIDE_DIR = [V, L, V, L, V, L, V, L, L, V]


def got(keys, table, directory, flags):
    return gp.classify(keys, table, directory, flags).tolist()


def test_live_and_dead_buckets_key_zero_and_key_max():
    """A live bucket takes its keys whatever their entries say; the dead
    bucket's keys go by their entries; key 0 (bucket 0 is live, its entry in
    value form) never uses the table; KEY_MAX (the last bucket is live) uses
    neither."""
    assert got(*wide()) == WIDE_BASE


def edit_table(f):
    def go(keys, table, directory, flags):
        b, info = table[0].copy(), dict(table[1])
        b, info = f(b, info) or (b, info)
        return keys, (b, info), directory, flags
    return go


def edit_dir(f):
    def go(keys, table, directory, flags):
        ent, info = directory[0].copy(), dict(directory[1])
        f(ent, info)
        return keys, table, (ent, info), flags
    return go


def edit_flags(**kw):
    def go(keys, table, directory, flags):
        return keys, table, directory, dict(flags, **kw)
    return go


def setcw(p, word):
    def f(ent, info):
        ent[p, 7] = word
    return edit_dir(f)


def kill(bucket):
    def f(b, info):
        b[bucket, 0] = vm.KEY_MAX
    return edit_table(f)


def revive(bucket):
    def f(b, info):
        b[bucket, 0] = 0
    return edit_table(f)


def change(base, **at):
    """base with the probes at the given positions (k0, kmax, p0..p7) moved"""
    names = ["k0", "kmax"] + [f"p{p}" for p in range(8)]
    out = list(base)
    for n, c in at.items():
        out[names.index(n)] = c
    return out


SINGLE_CHANGES = {
    # the table's fields
    "untrusted": (edit_table(lambda b, i: i.update(trusted=False)), WIDE_DIR),
    "no table": (edit_table(lambda b, i: (b[:0], i)), WIDE_DIR),
    "bucket 2 dies": (kill(2), change(WIDE_BASE, p4=V, p5=L)),
    "bucket 3 dies": (kill(3), change(WIDE_BASE, p6=L, p7=V)),
    "bucket 0 dies": (kill(0), change(WIDE_BASE, p0=V, p1=L)),
    "bucket 1 lives": (revive(1), change(WIDE_BASE, p2=T, p3=T)),
    "a live slot 0 is no marker": (edit_table(lambda b, i: b.__setitem__((2, 0), 1 << 63)), WIDE_BASE),
    "the marker in slot 1 is none": (edit_table(lambda b, i: b.__setitem__((2, 2), vm.KEY_MAX)), WIDE_BASE),
    # the tree's flags
    "page check": (edit_flags(page_check=True), [L] * 10),
    "not exact": (edit_flags(exact=False), change(WIDE_BASE, k0=L, p2=L)),
    # the directory's fields
    "fingerprint form": (edit_dir(lambda e, i: i.update(form="fingerprints")),
                         change(WIDE_BASE, k0=L, p2=L)),
    "no directory": (edit_dir(lambda e, i: i.update(form="none")), change(WIDE_BASE, k0=L, p2=L)),
    "p2 loses the flag": (setcw(2, cw(dm.PAIRS, 1)), change(WIDE_BASE, p2=L)),
    "p2 is marked bad": (setcw(2, cw(VAL | dm.PAIRS_BAD, 1)), change(WIDE_BASE, p2=L)),
    "p2 waits for the repair": (setcw(2, cw(VAL | dm.FIX, 1)), change(WIDE_BASE, p2=L)),
    "p2 holds three pairs": (setcw(2, cw(VAL, 3)), change(WIDE_BASE, p2=L)),
    "p2 spans three leaves": (setcw(2, cw(VAL, 2, nl=3)), change(WIDE_BASE, p2=L)),
    "p2 is a fingerprint entry": (setcw(2, cw(dm.FP, 0)), change(WIDE_BASE, p2=L)),
    "p2 holds no key": (setcw(2, cw(VAL, 0)), WIDE_BASE),
    "p3 gains the flag at two pairs": (setcw(3, cw(VAL, 2, nl=2)), change(WIDE_BASE, p3=V)),
    "p3 gains the flag at three pairs": (setcw(3, cw(VAL, 3)), WIDE_BASE),
    "p0 loses the flag": (setcw(0, cw(dm.PAIRS, 1)), change(WIDE_BASE, k0=L)),
    "p4 loses the flag behind a live bucket": (setcw(4, cw(dm.PAIRS, 1)), WIDE_BASE),
}


@pytest.mark.parametrize("name", sorted(SINGLE_CHANGES))
def test_one_changed_field_moves_exactly_its_keys(name):
    edit, want = SINGLE_CHANGES[name]
    assert got(*edit(*wide())) == want, name


def test_two_changes_compose():
    """no table and no exact directory: every probe reads its leaf"""
    args = SINGLE_CHANGES["not exact"][0](*SINGLE_CHANGES["untrusted"][0](*wide()))
    assert got(*args) == [L] * 10


LO, BITS = 1 << 40, 12


def narrow(dir_entries=8):
    """A shard's range [LO, LO + 4096): four live buckets of 1024 keys over
    prefixes of 512, every entry in value form."""
    b = np.zeros((4, 16), dtype=U64)
    table = (b, {"lo": LO, "shift": 10, "trusted": True})
    ent = np.zeros((dir_entries, 16), dtype=np.uint32)
    ent[:, 7] = cw(VAL, 1)
    directory = (ent, {"lo": LO, "shift": 9, "form": "pairs"})
    keys = u64s([0, 1, LO - 1, LO, LO + 1023, LO + 1024, LO + 4095, LO + 4096, LO + 8191, LO + 8192,
                 KEY_MAX - 1, KEY_MAX])
    return keys, table, directory, {"exact": True, "page_check": False}


def test_range_limits_of_a_narrow_table():
    """Below lo and past the last bucket a key uses neither the table nor
    (past the directory's own end) a value-form entry."""
    assert got(*narrow()) == [L, L, L, T, T, T, T, L, L, L, L, L]
    # the buckets at both limits dead: their keys go to the entries
    args = kill(0)(*kill(3)(*narrow()))
    assert got(*args) == [L, L, L, V, V, T, V, L, L, L, L, L]


def test_the_table_ends_before_the_directory_does():
    """The two ranges are checked apart: with sixteen prefixes under four
    buckets the keys past the last bucket are the entries' to answer."""
    assert got(*narrow(16)) == [L, L, L, T, T, T, T, V, V, L, L, L]


def test_a_key_below_lo_is_not_wrapped_into_a_bucket():
    """lo = 2^63 with four buckets of 2^62: key 5 is below lo, and (5 - lo)
    mod 2^64 would index bucket 2; the directory (same lo) does not cover it
    either."""
    b = np.zeros((4, 16), dtype=U64)
    table = (b, {"lo": 1 << 63, "shift": 62, "trusted": True})
    ent = np.zeros((2, 16), dtype=np.uint32)
    ent[:, 7] = cw(VAL, 1)
    directory = (ent, {"lo": 1 << 63, "shift": 62, "form": "pairs"})
    keys = u64s([5, (1 << 63) - 1, 1 << 63, (1 << 63) + (1 << 62), KEY_MAX - 1])
    flags = {"exact": True, "page_check": False}
    assert got(keys, table, directory, flags) == [L, L, T, T, T]
    table[1]["trusted"] = False
    assert got(keys, table, directory, flags) == [L, L, V, V, V]


def test_an_empty_directory_dump():
    keys, table, _, flags = wide()
    none = (np.zeros((0, 16), dtype=np.uint32), {"lo": 0, "shift": 0, "form": "none"})
    assert got(keys, table, none, flags) == change(WIDE_BASE, k0=L, p2=L)


def test_ties():
    """A prefix of 2^61 keys in two leaves, the second from offset
    0x12345678 << 29: the keys whose top 32 offset bits equal that split
    point tie; a one-leaf entry, a fingerprint entry and a directory of
    narrow prefixes (the split points are then whole offsets) never do."""
    keys, table, directory, flags = wide()
    ent, info = directory
    ent[7, 4] = 0x12345678
    base = 7 << 61
    split = base + (0x12345678 << 29)
    probes = u64s([split - 1, split, split + (1 << 29) - 1, split + (1 << 29), base, (2 << 61) + 5])
    assert gp.ties(probes, directory).tolist() == [False, True, True, False, False, False]
    ent[7, 7] = cw(VAL, 2, nl=1)
    assert not gp.ties(probes, directory).any()
    ent[7, 7] = cw(dm.FP, 0, nl=2)
    assert not gp.ties(probes, directory).any()
    # three leaves: the tie is with the leaf after the one the key starts in
    ent[7, 7] = cw(dm.PAIRS, 5, nl=3)
    ent[7, 5] = 0x20000000
    second = base + (0x20000000 << 29)
    probes = u64s([split, second, second - 1, second + (1 << 29)])
    assert gp.ties(probes, directory).tolist() == [True, True, False, False]
    _, _, nd, _ = narrow()
    nd[0][:, 7] = cw(VAL, 2, nl=2)
    nd[0][:, 4] = 7
    assert not gp.ties(u64s([LO + 7, LO + 512 + 7]), nd).any()


def stats(**kw):
    st = {"gets": 0, "hits": 0, "entry_reads": 0, "dir_fp_hits": 0, "right_moves": 0}
    st.update(kw)
    return st


def test_rules():
    """Rule 1: no "leaf" probe, no entry read.  Rule 2: at least one entry
    read per stored "leaf" probe (absent ones need none)."""
    cls = np.array([T, V, T])
    found = np.array([1, 1, 0], dtype=np.uint8)
    assert gp.assert_rules(cls, found, stats(gets=3, hits=2, dir_fp_hits=3)) == {T: 2, V: 1, L: 0}
    with pytest.raises(AssertionError):
        gp.assert_rules(cls, found, stats(gets=3, hits=2, entry_reads=1))
    cls = np.array([T, L, L, L])
    found = np.array([1, 1, 1, 0], dtype=np.uint8)
    gp.assert_rules(cls, found, stats(gets=4, hits=3, entry_reads=2))
    gp.assert_rules(cls, found, stats(gets=4, hits=3, entry_reads=5))
    with pytest.raises(AssertionError):
        gp.assert_rules(cls, found, stats(gets=4, hits=3, entry_reads=1))


def test_without_table_sets_and_restores_the_switch():
    for before in (None, "1"):
        if before is None:
            os.environ.pop("SHM_VALTAB", None)
        else:
            os.environ["SHM_VALTAB"] = before
        try:
            assert gp.without_table(lambda: os.environ["SHM_VALTAB"]) == "0"
            assert os.environ.get("SHM_VALTAB") == before
            with pytest.raises(ZeroDivisionError):
                gp.without_table(lambda: 1 // 0)
            assert os.environ.get("SHM_VALTAB") == before
        finally:
            os.environ.pop("SHM_VALTAB", None)
