"""The leaf directory at the limits of its entry format, against a host-side
model that shares no code with the library (tests/dir_model.py).

An exact directory is trusted for results: a usable entry that does not lead
to a key answers "absent" (get_sum.hip exact_miss), a value-form entry answers
from its inline copy (layout.h kDirVals).  The other directory tests spread
hashed keys over 2^64 (about two per prefix), which never reaches the edges of
the upkeep's state machine (dir_upkeep.h): 2 -> 3 keys (the value form ends),
8 -> 9 (the second inline entry lies where pairs 8.. would), 16 -> 17 (more
keys than pairs), many new keys of one prefix in one launch, delete /
re-insert churn (pairs of deleted keys stay), equal fingerprints, both ends of
the key space, a range hint narrower than the keys (shift 0 included) and
packed keys that all fall into entry 0.  Here crafted keys (p << shift) | low
drive chosen prefixes through those edges on small trees (2^14 hashed keys,
about 500 pages, 2^14 entries).

Targets come from the dumped image: a prefix wholly inside one leaf's
fences, with a known key count, one per leaf, in a leaf with room for every
key the scenario adds (so the leaf does not split and the entry's state is
the upkeep's own).  A target whose leaf splits anyway leaves the state
assertions and stays in every other check.

After every chunk (Rig.check): (a) searches of the touched keys, their and
their neighbouring prefixes' stored and absent keys and a fixed sample equal
the oracle; (b) the model finds no entry that makes a false claim, and the
page image equals the oracle's contents; (c) shm__dir_verify is clean; (d) no
error bit; (e) no rebuild, and the directory is still exact; (f) where the
tree has a key-value bucket table (valtab.h; every default rig whose keys do
not crowd into a few buckets), it is still trusted and its raw dump holds
exactly the oracle's pairs (tests/valtab_model.py): the scenarios put 9, 16
and 17 new keys of one bucket into one launch, churn, and work at both ends
of a key range.

The table answers a get before the directory entry is read, so the tests that
prove "answered by the entry" from the index statistics run twice: on a tree
without a table (Rig(table=False): SHM_VALTAB=0), where the entry is all a get
has, and on the default tree, where the model of the answering path
(tests/get_paths.py) says which probes the table takes.
"""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dir_model as dm  # noqa: E402
import get_paths as gp  # noqa: E402
import valtab_model as vm  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import assert_same, dev, gen_keys, gpu_search, lib_ok, U64  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402

N0 = 1 << 14
ARENA = 64 << 20
MB = 1 << 14
MIN_TARGETS = 32
LEAF_SLOTS = 54


def u64s(xs):
    return np.array([int(x) & ((1 << 64) - 1) for x in xs], dtype=U64)


class Rig:
    """A small tree with the upkeep on for every chunk, its oracle, and the
    model's view of both (refreshed by check())."""

    def __init__(self, form="pairs", keys=None, key_lo=0, key_bits=64, room=None, table=True):
        def make():  # (SHM_VALTAB is read when the tree is created)
            return shm.Tree(arena_bytes=ARENA, max_batch=MB, key_lo=key_lo, key_bits=key_bits)

        self.table = table
        self.t = make() if table else gp.without_table(make)
        self.t.dir_config(maint="always")
        self.orc = OracleTree(ARENA)
        self.rng = np.random.default_rng(31)
        self.vseq = 1
        base = gen_keys(self.t, 1, N0) if keys is None else keys
        self.apply(base, self.values(base.size))
        if room is not None:
            # the scenario adds up to `room` keys to a leaf it must not split:
            # where the load leaves too few leaves with that much room, one
            # chunk of deletes makes it, before the read phase
            valid = dm.Image(*self.t.dump_image()).leaf_valid
            self.thinned = bool(np.mean(valid + room < LEAF_SLOTS) < 0.75)
            print(f"load: {valid.size} leaves of {valid.min()}..{valid.max()} keys (mean "
                  f"{valid.mean():.1f}), thinned for {room} more: {self.thinned}")
            if self.thinned:
                self.thin(LEAF_SLOTS - 1 - room)
        for _ in range(5 if form == "pairs" else 1):  # five: the read phase's pair form
            gpu_search(self.t, base[:1024])
        st = self.t.dir_stats()
        assert st["form"] == form and st["exact"] == 1, st
        self.builds = st["builds"]
        vs = self.t.vt_stats()
        self.has_table = bool(vs["trusted"])
        assert table or vs["buckets"] == 0, vs
        print(f"rig: form {form}, table {'on' if table else 'off'}: {vs}")
        stored, _ = self.orc.dump()
        self.sample = stored[self.rng.integers(0, stored.size, 512)]
        self.checked = {"pair": 0, "value": 0, "fp": 0}
        self.refresh()
        assert self.d.n == st["entries"] and self.info["form"] == form, (self.info, st)

    def close(self):
        self.orc.close()
        self.t.close()

    def values(self, n):
        """n fresh values (never 0, never repeated)"""
        v = np.arange(self.vseq, self.vseq + n, dtype=U64) * U64(2) + U64(1)
        self.vseq += n
        return v

    def apply(self, k, v):
        k, v = np.asarray(k, dtype=U64), np.asarray(v, dtype=U64)
        assert 0 < k.size <= MB
        self.t.insert_batch(dev(k), dev(v))
        self.orc.apply_batch(k, v)

    def thin(self, max_valid):
        """one chunk of deletes before the read phase: every leaf keeps at
        most max_valid keys (room for the keys a scenario adds)"""
        im = dm.Image(*self.t.dump_image())
        order = np.argsort(im.leaf, kind="stable")
        rank = np.arange(im.keys.size) - np.searchsorted(im.leaf[order], im.leaf[order])
        drop = im.keys[order][rank >= max_valid]
        if drop.size:
            self.t.del_batch(dev(drop))
            self.t.synchronize()
            self.orc.apply_batch(drop, np.zeros(drop.size, dtype=U64))

    def refresh(self):
        self.im = dm.Image(*self.t.dump_image())
        ent, self.info = self.t.dir_dump()
        self.d = dm.Directory(ent, self.info["lo"], self.info["shift"])
        self.shift = self.d.shift
        _, _, self.count, _ = dm.prefix_tables(self.im, self.d)

    def key(self, p, low):
        return (self.d.lo + (int(p) << self.shift)) | int(low)

    def probes(self, touched):
        """the touched keys and their neighbours, every stored key of their
        prefixes and the two prefixes beside each, absent keys inside all of
        those, and the fixed sample"""
        touched = np.asarray(touched, dtype=U64)
        d = self.d
        p, cov = d.prefix_of(touched)
        pn = np.unique(np.concatenate([p[cov] - 1, p[cov], p[cov] + 1]))
        pn = pn[(pn >= 0) & (pn < d.n)]
        stored, _ = self.orc.dump()
        sp, sc = d.prefix_of(stored)
        others = stored[sc & np.isin(sp, pn)]
        a, _ = d.bounds(pn) if pn.size else (np.zeros(0, dtype=U64), None)
        inside = []
        for _ in range(2):
            low = self.rng.integers(0, 1 << min(self.shift, 62), pn.size).astype(U64)
            inside.append(a | low)
        with np.errstate(over="ignore"):
            near = np.concatenate([touched + U64(1), touched - U64(1)])
        return np.unique(np.concatenate([touched, near, others, self.sample] + inside))

    def check(self, touched, expect=()):
        """checks (a)-(e) after a chunk; `expect`: the classes of entries
        ("pair", "value", "fp") the model must have found to check"""
        t = self.t
        probe = self.probes(touched)
        gv, gf = gpu_search(t, probe)  # (a)
        assert_same(probe, *self.orc.search_batch(probe), gv, gf)
        self.refresh()  # (b)
        okeys, ovals = self.orc.dump()
        self.im.assert_equals(okeys, ovals)
        bad, checked = dm.check_trusted(self.im, self.d, okeys, ovals)
        assert bad == [], bad
        self.checked = checked
        v = t.dir_verify()  # (c)
        assert (v["bad_lists"], v["bad_pairs"], v["bad_fps"], v["bad_vals"]) == (0, 0, 0, 0), v
        assert t.last_error()["bits"] == 0, t.last_error()  # (d)
        st = t.dir_stats()  # (e)
        assert t.stats()["pages_used"] < 1024, t.stats()  # (no denser directory is due)
        assert st["builds"] == self.builds and st["exact"] == 1, (st, self.builds, t.stats())
        for c in expect:
            assert checked[c] > 0, (c, checked)
        if self.has_table:  # (f)
            assert t.vt_stats()["trusted"], t.vt_stats()
            bad, _ = vm.check_tree(t, okeys, ovals)
            assert bad == [], bad[:8]

    def finish(self):
        rc, oc = self.orc.check()
        assert rc == 0 and self.t.check()["keys"] == oc["keys"], (rc, oc, self.t.check())
        self.close()

    # -- targets -----------------------------------------------------------

    def targets(self, classes, add, per_class=40):
        """{count: Targets}: for each key count in `classes` up to per_class
        prefixes holding exactly that many keys, each wholly inside one
        leaf's fences, one per leaf, the leaf holding fewer than 54 - add
        valid entries"""
        im, d = self.im, self.d
        span = 1 << self.shift
        inside = []  # per leaf: the prefixes wholly inside its fences
        for i in range(im.leaf_page.size):
            lo_i, hi_i = int(im.leaf_lo[i]), int(im.leaf_hi[i])
            first = max(0, -((d.lo - lo_i) // span))
            last = (hi_i - d.lo) // span - 1 if hi_i >= d.lo else -1
            room = int(im.leaf_valid[i]) + add < LEAF_SLOTS
            inside.append(np.arange(first, min(last, d.n - 1) + 1) if room else np.zeros(0, dtype=np.int64))
        free = set(range(im.leaf_page.size))
        # the rarest class first: each class takes leaves the others could use
        have = {c: sum(1 for i in free if np.any(self.count[inside[i]] == c)) for c in classes}
        out = {}
        for c in sorted(classes, key=lambda c: have[c]):
            ps, leaves = [], []
            for i in sorted(free):
                if len(ps) == per_class:
                    break
                m = inside[i][self.count[inside[i]] == c]
                if m.size:
                    ps.append(int(m[m.size // 2]))
                    leaves.append(i)
            free -= set(leaves)
            out[c] = Targets(self, np.array(ps, dtype=np.int64), np.array(leaves, dtype=np.int64))
        return out


class Targets:
    """prefixes under test, each with its leaf as it was when chosen"""

    def __init__(self, rig, prefixes, leaves):
        self.rig, self.p = rig, prefixes
        self.page = rig.im.leaf_page[leaves].copy()
        self.hi = rig.im.leaf_hi[leaves].copy()
        self.split = np.zeros(prefixes.size, dtype=bool)
        self.used = {int(p): set() for p in prefixes}

    def take(self, n):
        """the first n targets as a set of their own"""
        t = Targets.__new__(Targets)
        t.rig, t.p, t.page, t.hi = self.rig, self.p[:n], self.page[:n], self.hi[:n]
        t.split, t.used = self.split[:n].copy(), {int(p): set() for p in self.p[:n]}
        self.p, self.page, self.hi, self.split = self.p[n:], self.page[n:], self.hi[n:], self.split[n:]
        return t

    def keys(self):
        """the stored keys of the targets, as the model last saw them: a list
        per target"""
        im, d = self.rig.im, self.rig.d
        a, b = d.bounds(self.p) if self.p.size else (np.zeros(0, dtype=U64),) * 2
        i0, i1 = np.searchsorted(im.keys, a, side="left"), np.searchsorted(im.keys, b, side="right")
        return [im.keys[x:y] for x, y in zip(i0, i1)]

    def fresh(self, n, same_fp=None):
        """n keys per target that were never stored in it: an (targets, n)
        array"""
        rig = self.rig
        held = self.keys()
        out = np.zeros((self.p.size, n), dtype=U64)
        for i, p in enumerate(self.p):
            got = []
            while len(got) < n:
                low = int(rig.rng.integers(1, 1 << min(rig.shift, 62)))
                k = rig.key(p, low)
                if k in self.used[int(p)] or k in held[i] or k == dm.KEY_MAX:
                    continue
                self.used[int(p)].add(k)
                got.append(k)
            out[i] = u64s(got)
        return out

    def unsplit(self):
        """the targets whose leaf is still the page it was, with the same
        fences (a split keeps the left half in place and lowers its highest
        fence); once split, always split"""
        im, d = self.rig.im, self.rig.d
        f, l = dm.covering_leaves(im, d, self.p)
        self.split |= ~((f == l) & (im.leaf_page[f] == self.page) & (im.leaf_hi[f] == self.hi))
        return ~self.split

    def counts(self):
        return self.rig.count[self.p]


def expect_state(rig, tg, flagged, label):
    """scenario 1's state rules for the unsplit targets, from the raw count
    words: up to 2 keys in a flagged entry the value form is usable; from 3
    to 16 keys the pair form is, as a fresh build's would be; at 17 it is
    not.  Returns the number of targets held to them."""
    ok = tg.unsplit()
    p, c = tg.p[ok], tg.counts()[ok]
    d = rig.d
    fresh = dm.fresh_usable(rig.im, d, p) if p.size else np.zeros(0, dtype=bool)
    for i in range(p.size):
        cw = int(d.cw[p[i]])
        what = (label, int(p[i]), int(c[i]), hex(cw))
        if c[i] <= 2 and flagged:
            assert d.val_usable[p[i]], ("value form not usable", what)
        if c[i] <= 16:
            assert d.pair_usable[p[i]], ("pair form not usable", what)
            assert fresh[i], ("the model's fresh build disagrees", what)
        else:
            assert not d.pair_usable[p[i]] and not fresh[i], ("usable past 16 keys", what)
    return int(ok.sum())


def reads_no_leaf_entry(rig, keys, label=""):
    """a batch of stored keys answered by value-form entries alone: without
    a table the model gives every one of them to the value form; with one,
    to the value form or to a live bucket"""
    keys = np.asarray(keys, dtype=U64)
    gv, gf, st, cls = gp.searched(rig.t, keys)
    assert_same(keys, *rig.orc.search_batch(keys), gv, gf)
    n = gp.assert_rules(cls, gf, st, f"reads no leaf entry {label}")
    assert bool(gf.all()) and st["gets"] == keys.size, st
    assert n[gp.LEAF] == 0, n
    if not rig.table:
        assert n[gp.VALUE] == keys.size, n
    assert st["entry_reads"] == 0 and st["dir_fp_hits"] == st["gets"], st
    return n


def concat(parts):
    return np.concatenate([np.asarray(x, dtype=U64).ravel() for x in parts])


def _growth(form, table):
    """Scenario 1.  Prefixes that start with 0, 1, 2 (built in value form)
    and 3, 4 keys (plain pair form) each get one new key per chunk until
    they hold 17: across 2 -> 3 (the value form ends through the count),
    8 -> 9 (a flagged entry is handed to the repair) and 16 -> 17 (more keys
    than pairs: not usable).  The fingerprint form runs the same chunks
    under checks (a)-(e) (its entries carry a byte per slot, no count)."""
    t0 = time.time()
    rig = Rig(form, room=17, table=table)
    assert rig.has_table == (table and form == "pairs"), rig.t.vt_stats()
    seen = {gp.TABLE: 0, gp.VALUE: 0, gp.LEAF: 0}
    tgs = rig.targets([0, 1, 2, 3, 4], add=17)
    for c, tg in tgs.items():
        assert tg.p.size >= MIN_TARGETS, (c, tg.p.size)
        assert np.array_equal(tg.counts(), np.full(tg.p.size, c))
    done = {c: 0 for c in tgs}
    # A write phase whose chunks stop adding pages is rebuilt in the pair form
    # after kQuietChunks = 2 of them (tree_dir.cpp want_pairs).  To stay in the
    # fingerprint form each of its chunks also splits one leaf that holds no
    # target, with a run of 40 keys behind the leaf's lowest fence.
    taken = concat([tg.page for tg in tgs.values()])
    spare = np.nonzero(~np.isin(rig.im.leaf_page, taken.astype(np.int64)))[0][1:18]
    assert form == "pairs" or spare.size == 17
    runs = rig.im.leaf_lo[spare][:, None] + np.arange(1, 41, dtype=U64)[None, :]
    for step in range(17):
        new = [tg.fresh(1) for c, tg in tgs.items() if c + step < 17]
        if form != "pairs":
            new.append(runs[step])
        k = concat(new)
        rig.apply(k, rig.values(k.size))
        rig.check(k, expect=("pair", "value") if form == "pairs" else ("fp",))
        for c, tg in tgs.items():
            now = min(c + step + 1, 17)
            ok = tg.unsplit()
            assert np.all(tg.counts()[ok] == now), (c, step)
            if form != "pairs":
                done[c] = int(ok.sum())
                continue
            done[c] = expect_state(rig, tg, flagged=c <= 2, label=(c, step))
            if c <= 2 and now <= 2 and ok.any():
                n = reads_no_leaf_entry(rig, concat([x for x, o in zip(tg.keys(), ok) if o]),
                                        f"(scenario 1, class {c}, step {step})")
                seen = {x: seen[x] + n[x] for x in seen}
    if form == "pairs":  # with the table on nearly every such get is the table's
        print(f"scenario 1: keys of small prefixes per class {seen}")
        assert seen[gp.VALUE] > 0 if not table else seen[gp.TABLE] > 0.9 * sum(seen.values()), seen
    print(f"scenario 1 [{form}]: unsplit targets per class {done}, model checked {rig.checked}, "
          f"{time.time() - t0:.2f} s")
    for c, n in done.items():
        assert n >= MIN_TARGETS, (c, n)
    rig.finish()


@pytest.mark.parametrize("form", ["pairs", "fingerprints"])
def test_growth_across_the_limits_one_key_per_chunk(lib_ok, form):
    """scenario 1 on the default tree (a bucket table beside the pair form)"""
    _growth(form, True)


def test_growth_across_the_limits_one_key_per_chunk_without_the_table(lib_ok):
    """scenario 1 on a tree made without a bucket table: the value form answers"""
    _growth("pairs", False)


def _same_limits(k, table):
    """Scenario 2.  One chunk adds k keys to each target that held 0 keys or
    1 key: the lanes of one launch race for the pair positions and the
    inline entries; the states are scenario 1's for the resulting count."""
    t0 = time.time()
    rig = Rig(room=k, table=table)
    assert rig.has_table == table, rig.t.vt_stats()
    tgs = rig.targets([0, 1], add=k)
    new = concat([tg.fresh(k) for tg in tgs.values()])
    rig.rng.shuffle(new)
    rig.apply(new, rig.values(new.size))
    rig.check(new, expect=("pair", "value"))
    done = {}
    for c, tg in tgs.items():
        ok = tg.unsplit()
        assert np.all(tg.counts()[ok] == c + k), (c, k)
        done[c] = expect_state(rig, tg, flagged=True, label=(c, k))
        if c + k <= 2 and ok.any():
            reads_no_leaf_entry(rig, concat([x for x, o in zip(tg.keys(), ok) if o]),
                                f"(scenario 2, k={k}, class {c})")
    print(f"scenario 2 [k={k}]: unsplit targets per class {done}, model checked {rig.checked}, "
          f"{time.time() - t0:.2f} s")
    for c, n in done.items():
        assert n >= MIN_TARGETS, (c, n)
    rig.finish()


@pytest.mark.parametrize("k", [2, 3, 8, 9, 16, 17])
def test_the_same_limits_inside_one_launch(lib_ok, k):
    """scenario 2 on the default tree (with the bucket table)"""
    _same_limits(k, True)


@pytest.mark.parametrize("k", [2, 3, 8, 9, 16, 17])
def test_the_same_limits_inside_one_launch_without_the_table(lib_ok, k):
    """scenario 2 on a tree made without a bucket table"""
    _same_limits(k, False)


def _one_chunk_mixes_ops(table):
    """Scenario 3.  Prefixes {A, B} held inline; one chunk, a case per set
    of targets: delete A + new C; update A + new C; delete A and B + two new
    keys; A deleted and re-inserted; A updated twice (the last writer wins).
    Every entry stays usable.  Where the chunk only changed A the repair
    rebuilds the entry as a build would: two keys inline again, their gets
    read no leaf entry.  (Where it also added a key, the new key's lane may
    count its pair before A's lane looks: the entry then holds three or four
    pairs, A's dead one among them, and is served as a plain pair entry.)"""
    t0 = time.time()
    rig = Rig(room=2, table=table)
    assert rig.has_table == table, rig.t.vt_stats()
    all2 = rig.targets([2], add=2, per_class=5 * MIN_TARGETS + 40)[2]
    assert all2.p.size >= 5 * MIN_TARGETS, all2.p.size
    n = all2.p.size // 5
    cases = {name: all2.take(n) for name in ("del+new", "upd+new", "del2+new2", "del+reins", "upd2")}
    ks, vs = [], []

    def op(k, v):
        ks.append(np.asarray(k, dtype=U64).ravel())
        vs.append(np.asarray(v, dtype=U64).ravel())

    zero = np.zeros(n, dtype=U64)
    want = {}
    for name, tg in cases.items():
        held = np.array([x for x in tg.keys()], dtype=U64)
        assert held.shape == (n, 2)
        a, b = held[:, 0], held[:, 1]
        if name == "del+new":
            op(a, zero), op(tg.fresh(1), rig.values(n))
            want[name] = 2
        elif name == "upd+new":
            op(a, rig.values(n)), op(tg.fresh(1), rig.values(n))
            want[name] = 3
        elif name == "del2+new2":
            op(a, zero), op(b, zero), op(tg.fresh(2), rig.values(2 * n))
            want[name] = 2
        elif name == "del+reins":
            op(a, zero), op(a, rig.values(n))  # (batch order: the delete first)
            want[name] = 2
        else:
            op(a, rig.values(n)), op(a, rig.values(n))
            want[name] = 2
    k, v = concat(ks), concat(vs)
    rig.apply(k, v)
    rig.check(k, expect=("pair", "value"))
    done = {}
    for name, tg in cases.items():
        ok = tg.unsplit()
        assert np.all(tg.counts()[ok] == want[name]), name
        inline = name in ("del+reins", "upd2")
        done[name] = expect_state(rig, tg, flagged=inline, label=name)
        if inline:
            reads_no_leaf_entry(rig, concat([x for x, o in zip(tg.keys(), ok) if o]),
                                f"(scenario 3, {name})")
    print(f"scenario 3: unsplit targets per case {done}, model checked {rig.checked}, "
          f"{time.time() - t0:.2f} s")
    for name, m in done.items():
        assert m >= MIN_TARGETS, (name, m)
    rig.finish()


def test_one_chunk_mixes_ops_on_a_value_form_prefix(lib_ok):
    """scenario 3 on the default tree (with the bucket table)"""
    _one_chunk_mixes_ops(True)


def test_one_chunk_mixes_ops_on_a_value_form_prefix_without_the_table(lib_ok):
    """scenario 3 on a tree made without a bucket table"""
    _one_chunk_mixes_ops(False)


def _churn(table):
    """Scenario 4.  Sixteen rounds: a chunk deletes one key
    of every target, the next re-inserts it with a new value.  The pair of a
    deleted key is never removed, so a prefix of 3 keys reaches 16 pairs
    after 13 rounds.  The pair that does not fit hands the entry to the
    repair, which counts the valid keys again: at the end every target (3
    keys; 1 key, in value form) is usable and every get of its keys is
    answered through its entry.  (Before: the entry was marked bad for
    good, correct results through the summary walk.)"""
    t0 = time.time()
    rig = Rig(room=1, table=table)
    assert rig.has_table == table, rig.t.vt_stats()
    tgs = rig.targets([1, 3], add=1)
    for c, tg in tgs.items():
        assert tg.p.size >= MIN_TARGETS, (c, tg.p.size)
    victim = {c: np.array([x[0] for x in tg.keys()], dtype=U64) for c, tg in tgs.items()}
    vk = concat(victim.values())
    for r in range(16):
        rig.apply(vk, np.zeros(vk.size, dtype=U64))
        rig.check(vk, expect=("pair", "value"))
        rig.apply(vk, rig.values(vk.size))
        rig.check(vk, expect=("pair", "value"))
    done = {}
    for c, tg in tgs.items():
        ok = tg.unsplit()
        assert np.all(tg.counts()[ok] == c), c
        done[c] = expect_state(rig, tg, flagged=c <= 2, label=("churn", c))
        keys = concat([x for x, o in zip(tg.keys(), ok) if o])
        # a prefix of 3 keys is answered through its pairs, reading a leaf
        # entry per key, unless a live bucket holds it: the keys the model
        # does not give to the table are held to that on their own
        _, gf, st, cls = gp.check_paths(rig.t, rig.orc, keys, table, f"scenario 4, class {c}")
        assert bool(gf.all()) and st["dir_fp_hits"] == st["gets"] == keys.size, (c, st)
        want = gp.VALUE if c <= 2 else gp.LEAF
        assert np.all(cls[cls != gp.TABLE] == want), (c, gp.tally(cls))
        rest = keys[cls != gp.TABLE]
        if rest.size:
            gv, gf, st, _ = gp.searched(rig.t, rest)
            assert_same(rest, *rig.orc.search_batch(rest), gv, gf)
            assert bool(gf.all()) and st["dir_fp_hits"] == st["gets"] == rest.size, (c, st)
        assert table or rest.size == keys.size
    print(f"scenario 4: unsplit targets per class {done}, model checked {rig.checked}, "
          f"{time.time() - t0:.2f} s")
    for c, m in done.items():
        assert m >= MIN_TARGETS, (c, m)
    rig.finish()


def test_churn_keeps_small_prefixes_usable(lib_ok):
    """scenario 4 on the default tree (with the bucket table)"""
    _churn(True)


def test_churn_keeps_small_prefixes_usable_without_the_table(lib_ok):
    """scenario 4 on a tree made without a bucket table"""
    _churn(False)


def raw_fp_byte(k):
    return ((k * U64(0x9E3779B97F4A7C15)) >> U64(56)).astype(np.int64)


def test_twelve_keys_of_one_fingerprint(lib_ok):
    """Scenario 5.  Twelve keys that share one fingerprint in an empty
    prefix, nine in one chunk and three in the next: more candidates of one
    fingerprint than a get queues (8), so such a prefix cannot answer
    "absent" from its entry.  One prefix shares the raw hash byte 0 (which
    key_fp maps to 1), one the byte 1, one mixes both.  Probes: all twelve,
    absent keys of the prefix with the same fingerprint, and with others."""
    t0 = time.time()
    rig = Rig(room=12)
    tg = rig.targets([0], add=12)[0]
    assert tg.p.size >= MIN_TARGETS, tg.p.size
    own, same, other = [], [], []
    with np.errstate(over="ignore"):
        for i, p in enumerate(tg.p):
            low = np.unique(rig.rng.integers(1, 1 << min(rig.shift, 62), 1 << 14).astype(U64))
            cand = U64(rig.key(p, 0)) | low
            raw = raw_fp_byte(cand)
            want = [0] if i == 0 else [1] if i == 1 else [0, 1] if i == 2 else [int(raw[i])]
            hit = cand[np.isin(raw, want)]
            assert hit.size >= 16, (i, hit.size)
            assert np.unique(dm.key_fp(hit)).size == 1
            own.append(hit[:12])
            same.append(hit[12:20])
            other.append(cand[~np.isin(raw, want)][:8])
    own = np.array(own, dtype=U64)
    probe = concat([own, concat(same), concat(other)])
    for part in (own[:, :9], own[:, 9:]):
        k = part.ravel().copy()
        rig.rng.shuffle(k)
        rig.apply(k, rig.values(k.size))
        rig.check(probe, expect=("pair", "value"))
    ok = tg.unsplit()
    assert np.all(tg.counts()[ok] == 12)
    n = expect_state(rig, tg, flagged=True, label="fp12")
    gv, gf = gpu_search(rig.t, own.ravel())
    assert bool(gf.all())
    print(f"scenario 5: unsplit targets {n}, model checked {rig.checked}, {time.time() - t0:.2f} s")
    assert n >= MIN_TARGETS, n
    rig.finish()


@pytest.mark.parametrize("form", ["pairs", "fingerprints"])
def test_both_ends_of_the_key_space(lib_ok, form):
    """Scenario 6.  Keys 0 and 1, a descending run down to 0 and an
    ascending run of 200 keys ending at 2^64 - 2, over four chunks: the
    leftmost leaf (lowest fence 0) and the rightmost (highest fence: the
    maximum key, which is never stored) split again and again under the
    upkeep."""
    t0 = time.time()
    rig = Rig(form)
    top = (1 << 64) - 2
    asc = u64s(range(top - 199, top + 1))
    desc = u64s(range(400, -1, -1))  # 400, 399, ..., 0
    chunks = [concat([u64s([0, 1]), asc[:50]]),
              concat([desc[:140], asc[50:100]]),
              concat([desc[140:280], asc[100:150]]),
              concat([desc[280:], asc[150:]])]  # (ends ..., 1, 0: those two are updates)
    ends = u64s([0, 1, 2, 400, 401, 402, top - 200, top - 199, top, top + 1, top - 150, top - 149,
                 120, 121, 260, 261])
    pages0 = rig.t.stats()["pages_used"]
    for k in chunks:
        rig.apply(k, rig.values(k.size))
        rig.check(concat([k, ends]), expect=("pair",) if form == "pairs" else ())
    assert rig.t.stats()["pages_used"] >= pages0 + 8, (pages0, rig.t.stats())
    gv, gf = gpu_search(rig.t, concat([asc, desc]))
    assert bool(gf.all())
    print(f"scenario 6 [{form}]: model checked {rig.checked}, {time.time() - t0:.2f} s")
    rig.finish()


def test_range_hint_of_a_shard_with_strays_at_both_limits(lib_ok):
    """Scenario 7 (i).  The hint of shard 5 of 8; the load holds keys of the
    range and strays below and above it.  Chunks then add runs of 100
    sequential keys across each limit, so pages split with fences that
    straddle the first key and the end of the directory's range, and update
    and delete among them."""
    from sherman_amd.shard import shard_range
    t0 = time.time()
    lo, bits = shard_range(5, 8)
    end = lo + (1 << bits)
    h = gen_keys(shm_tree_for_keys(), 1, N0)
    mine = U64(lo) + (h[:N0 - 1024] >> U64(64 - bits))
    below = h[N0 - 1024:N0 - 512] % U64(lo)
    above = U64(end) + h[N0 - 512:] % U64((1 << 64) - 1 - end)
    rig = Rig(keys=np.unique(concat([mine, below, above])), key_lo=lo, key_bits=bits)
    assert rig.d.lo == lo and lo + (rig.d.n << rig.shift) == end, rig.info
    run_lo = u64s(range(lo - 50, lo + 50))
    run_hi = u64s(range(end - 50, end + 50))
    more = concat([u64s(range(lo - 150, lo - 50)), u64s(range(lo + 50, lo + 150)),
                   u64s(range(end - 150, end - 50)), u64s(range(end + 50, end + 150))])
    ends = u64s([lo - 151, lo - 1, lo, lo + 150, end - 151, end - 1, end, end + 150])
    pages0 = rig.t.stats()["pages_used"]
    chunks = [(run_lo, rig.values(100)), (run_hi, rig.values(100)), (more, rig.values(more.size)),
              (concat([run_lo[::3], run_hi[::3], run_lo[1::3], run_hi[1::3]]),
               concat([np.zeros(2 * run_lo[::3].size, dtype=U64), rig.values(2 * run_lo[1::3].size)]))]
    for k, v in chunks:
        rig.apply(k, v)
        rig.check(concat([k, ends, run_lo, run_hi]), expect=("pair", "value"))
    assert rig.t.stats()["pages_used"] >= pages0 + 6, (pages0, rig.t.stats())
    print(f"scenario 7i: model checked {rig.checked}, {time.time() - t0:.2f} s")
    rig.finish()


_KEYGEN = []


def shm_tree_for_keys():
    """a tiny tree whose only use is the device key generator"""
    if not _KEYGEN:
        _KEYGEN.append(shm.Tree(arena_bytes=1 << 20, max_batch=1 << 10))
    return _KEYGEN[0]


def test_range_hint_of_one_key_per_prefix(lib_ok):
    """Scenario 7 (ii).  key_lo = 2^40, key_bits = 12: the directory's bits
    are capped at the hint's, so shift == 0 and a prefix is one key.  All
    4096 keys of the range go in over four chunks with 500 strays on each
    side of it (the hashed load is all strays), then chunks update and
    delete them."""
    t0 = time.time()
    lo, bits = 1 << 40, 12
    rig = Rig(key_lo=lo, key_bits=bits)
    assert rig.shift == 0 and rig.d.n == 1 << bits and rig.d.lo == lo, rig.info
    inr = u64s(range(lo, lo + (1 << bits)))
    rig.rng.shuffle(inr)
    below = u64s(range(lo - 500, lo))
    above = u64s(range(lo + (1 << bits), lo + (1 << bits) + 500))
    ends = u64s([lo - 501, lo - 1, lo, lo + 4095, lo + 4096, lo + 4596])
    for c in range(4):
        k = concat([inr[c::4], below[c::4], above[c::4]])
        rig.apply(k, rig.values(k.size))
        rig.check(concat([k, ends]), expect=("pair", "value"))
        assert rig.count.max() <= 1
    upd = concat([inr[:1500], below[:100], above[:100]])
    rig.apply(upd, rig.values(upd.size))
    rig.check(concat([upd, ends]), expect=("pair", "value"))
    dele = concat([inr[1000:2500], below[50:150], above[50:150]])
    rig.apply(dele, np.zeros(dele.size, dtype=U64))
    rig.check(concat([dele, ends]), expect=("pair", "value"))
    back = inr[2000:3000]  # half of them deleted above
    rig.apply(back, rig.values(back.size))
    rig.check(concat([back, ends]), expect=("pair", "value"))
    print(f"scenario 7ii: model checked {rig.checked}, {time.time() - t0:.2f} s")
    rig.finish()


def test_packed_keys_all_in_entry_zero(lib_ok):
    """Scenario 8.  Keys packed below 2^26 under key_bits 64 (the keyspace
    of the C1 workload): every key lies in entry 0, whose prefix spans the
    whole tree (a cover-page entry), and every split page is shared.  2^14
    keys, then three chunks of 2^12 with searches between; about 9 % of the
    probes are absent.  No usable entry may make a false claim."""
    t0 = time.time()
    ks = 1 << 26
    gen = shm_tree_for_keys()
    rig = Rig(keys=gen_keys(gen, 1, N0, keyspace=ks))
    nid = N0 + 1
    for c in range(3):
        new = gen_keys(gen, nid, 1 << 12, keyspace=ks)
        nid += new.size
        rig.apply(new, rig.values(new.size))
        stored, _ = rig.orc.dump()  # (check() probes every stored key of entry 0)
        absent = gen_keys(gen, nid + (1 << 20) + (1 << 12) * c, stored.size // 10, keyspace=ks)
        rig.check(concat([new, absent]), expect=("pair",))
        stored, _ = rig.orc.dump()
        assert stored.max() <= ks and rig.d.prefix_of(stored)[0].max() == 0
        assert not rig.d.pair_usable[0] and not rig.d.fp_form[0], hex(int(rig.d.cw[0]))
    print(f"scenario 8: model checked {rig.checked}, {time.time() - t0:.2f} s")
    rig.finish()
