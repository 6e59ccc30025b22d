"""The get's three answering paths -- a live bucket of the key-value table
(valtab.h), a value-form directory entry behind a dead bucket (layout.h
kDirVals), the leaves -- each pinned by the host model of the paths
(tests/get_paths.py) on the tree's own raw dumps, and by the index statistics
of batches the model sends down one path only.

With a table, 95 % of the stored gets of a hashed load end at their bucket,
so a random probe barely reaches the directory code; the tests here build
the probes that do: every stored key the model classes "value" (its bucket is
dead, its prefix holds at most two keys), buckets that die while their small
prefixes are being read, the first keys of the leaves on a tree without a
table, and key 0 and both ends of the key range beside a table.

Trees are those of the neighbouring files: test_gpu_dir_vals.loaded() (2^18
hashed keys) and test_gpu_dir_edges.Rig (2^14).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dir_model as dm  # noqa: E402
import get_paths as gp  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import lib_ok, U64  # noqa: E402
import test_gpu_dir_edges as ed  # noqa: E402
import test_gpu_dir_vals as dv  # noqa: E402
import valtab_model as vm  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402

T, V, L = gp.TABLE, gp.VALUE, gp.LEAF


def directory_of(t):
    ent, info = t.dir_dump()
    return dm.Directory(ent, info["lo"], info["shift"])


def absent_inside(d, prefixes, rng, stored, per=2):
    """`per` keys per prefix that are not stored, inside the prefix"""
    a, _ = d.bounds(prefixes)
    out = []
    for _ in range(per):
        low = rng.integers(1, 1 << min(d.shift, 62), a.size).astype(U64)
        out.append(a | low)
    k = np.unique(np.concatenate(out))
    return k[~np.isin(k, stored) & (k != U64(shm.KEY_MAX))]


def test_value_form_behind_a_dead_bucket(lib_ok):
    """Table on, 2^18 hashed keys: every stored key the model classes
    "value" (318 by the hashed key set alone; at least 128 asserted from the
    dumps) and, for each of their prefixes, two absent keys inside it, in one
    batch: the model gives all of them to the value form, the answers equal
    the oracle, and no leaf entry is read.  A wrong inline value, or a wrong
    "absent" from the entry, has nowhere else to come from in this batch."""
    t, orc, base = dv.loaded()
    assert t.vt_stats()["trusted"], t.vt_stats()
    table, directory, flags = gp.dumps(t)
    cls = gp.classify(base, table, directory, flags)
    print(f"stored keys per class: {gp.tally(cls)}")
    stored = base[cls == V]
    assert stored.size >= 128, gp.tally(cls)
    d = directory_of(t)
    p, cov = d.prefix_of(stored)
    assert cov.all()
    absent = absent_inside(d, np.unique(p), np.random.default_rng(41), base)
    absent = absent[~gp.ties(absent, directory)]
    assert absent.size >= np.unique(p).size, (absent.size, np.unique(p).size)
    probe = np.concatenate([stored, absent])
    gv, gf, st, c2 = gp.searched(t, probe)
    gp.assert_equal(probe, *orc.search_batch(probe), gv, gf)
    n = gp.assert_rules(c2, gf, st, "value form behind dead buckets")
    assert n[V] == probe.size, n
    assert bool(gf[:stored.size].all()) and not gf[stored.size:].any()
    assert st["gets"] == probe.size and st["hits"] == stored.size, st
    assert st["entry_reads"] == 0 and st["right_moves"] == 0 and st["page_hops"] == 0, st
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()


def test_ties_with_no_table(lib_ok):
    """test_directory_ties_start_at_the_leaf's tree at 2^16 keys, made
    without a table: the model gives none of the leaves' first keys to a
    table, more than 200 of them tie with a split point of their entry, and
    their gets make no right move and equal the oracle."""
    def make():
        return shm.Tree(arena_bytes=128 << 20, max_batch=1 << 16)

    t = gp.without_table(make)
    orc = OracleTree(128 << 20)
    ks = dv.gen_keys(t, 1, 1 << 16)
    t.insert_batch(dv.dev(ks), dv.dev(ks ^ U64(0x55)))
    orc.apply_batch(ks, ks ^ U64(0x55))
    im = dm.Image(*t.dump_image())
    seps = im.leaf_lo[1:]
    seps = seps[np.isin(seps, ks)]  # every leaf's first key (stored)
    for _ in range(6):  # a read phase: the directory is rebuilt exact
        dv.gpu_search(t, ks[:4096])
    assert t.vt_stats()["buckets"] == 0, t.vt_stats()
    assert t.dir_stats()["form"] == "pairs", t.dir_stats()
    tie = gp.ties(seps, t.dir_dump())
    print(f"{seps.size} first keys, {int(tie.sum())} tie")
    assert int(tie.sum()) > 200, (seps.size, int(tie.sum()))
    gv, gf, st, cls = gp.searched(t, seps)
    gp.assert_equal(seps, *orc.search_batch(seps), gv, gf)
    n = gp.assert_rules(cls, gf, st, "first keys, no table")
    assert n[T] == 0, n
    assert bool(gf.all()) and st["gets"] == seps.size, st
    assert st["right_moves"] == 0, st
    near = np.concatenate([seps - U64(1), seps + U64(1)])
    gv, gf, st, cls = gp.searched(t, near)
    gp.assert_equal(near, *orc.search_batch(near), gv, gf)
    gp.assert_rules(cls, gf, st, "beside the first keys, no table")
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()


@pytest.mark.parametrize("keys", ["whole", "shard"])
def test_key_zero_and_the_range_ends_beside_a_table(lib_ok, keys):
    """Key 0, the first key a bucket can hold and a key of the last bucket,
    all stored, table on: over the whole key space (key 1, 2^64 - 2) and
    under the range hint of shard 5 of 8 (key_lo > 0: its first and last
    key).  Key 0 is never the table's (class "leaf", or "value" where the
    directory covers it), the other two are; gets equal the oracle as
    loaded, after an update of each and after a delete of each, under the
    rig's checks (the table's model among them)."""
    from sherman_amd.shard import shard_range
    if keys == "whole":
        lo, bits, end = 0, 64, 1 << 64
        base = ed.gen_keys(ed.shm_tree_for_keys(), 1, ed.N0)
        three = ed.u64s([0, 1, end - 2])
    else:
        lo, bits = shard_range(5, 8)
        end = lo + (1 << bits)
        h = ed.gen_keys(ed.shm_tree_for_keys(), 1, ed.N0)
        base = np.concatenate([U64(lo) + (h[:ed.N0 - 1024] >> U64(64 - bits)),
                               h[ed.N0 - 1024:ed.N0 - 512] % U64(lo),
                               U64(end) + h[ed.N0 - 512:] % U64((1 << 64) - 1 - end)])
        three = ed.u64s([0, lo, end - 1])
    load = np.unique(np.concatenate([base[3:], three]))  # (one chunk: at most 2^14 keys)
    rig = ed.Rig(keys=load, key_lo=lo, key_bits=bits)
    assert rig.has_table, rig.t.vt_stats()
    buckets, info = rig.t.vt_dump()
    assert info["lo"] == lo and lo + (buckets.shape[0] << info["shift"]) == end, info
    home = vm.bucket_of(three, info["lo"], info["shift"])
    assert home.tolist() == [-1, 0, buckets.shape[0] - 1], home

    def look(label, stored):
        gv, gf, st, cls = gp.searched(rig.t, three)
        gp.assert_equal(three, *rig.orc.search_batch(three), gv, gf)
        gp.assert_rules(cls, gf, st, f"{keys}: {label}")
        assert bool(gf.all()) == stored and bool(gf.any()) == stored, gf
        assert cls[0] in (L, V) and (cls[0] == L or keys == "whole"), cls
        assert not vm.dead(rig.t.vt_dump()[0])[[0, -1]].any()
        assert cls[1:].tolist() == [T, T], cls

    look("as loaded", True)
    rig.apply(three, rig.values(3))
    rig.check(three)
    look("updated", True)
    rig.apply(three, np.zeros(3, dtype=U64))
    rig.check(three)
    look("deleted", False)
    rig.apply(three, rig.values(3))
    rig.check(three)
    look("stored again", True)
    rig.finish()


def test_a_bucket_dies_under_its_readers(lib_ok):
    """Live buckets that hold a prefix of one or two keys (in value form)
    beside a prefix of six: while the bucket lives, the small prefix's keys,
    stored and absent, are the table's; one chunk brings the bucket to 9 keys
    and it dies; from then on the same keys are the value form's.  Both times
    they read no leaf entry and equal the oracle.  A chunk of deletes then
    takes the bucket back to 7 keys: it stays dead (until the next build),
    the model still says "value" for the small prefix and "leaf" for the
    large one, and every answer equals the oracle.

    (The hashed load alone has about thirty buckets with a prefix of five or
    six keys beside one of one or two, so a first chunk grows the larger
    prefix of each chosen bucket to six; the buckets stay live.)"""
    rig = ed.Rig(room=8)
    assert rig.has_table, rig.t.vt_stats()
    im, d = rig.im, rig.d
    buckets, info = rig.t.vt_dump()
    nb = buckets.shape[0]
    assert info["lo"] == d.lo and info["shift"] == d.shift + 1 and 2 * nb == d.n, (info, d.n)
    count = rig.count
    both = np.arange(d.n).reshape(-1, 2)  # bucket b: prefixes 2 b and 2 b + 1
    c = count[both]
    first, last = dm.covering_leaves(im, d, np.arange(d.n))
    one_leaf = (first == last)[both].all(axis=1) & (first[both[:, 0]] == first[both[:, 1]])
    leaf = first[both[:, 0]]
    room = im.leaf_valid[leaf] + 8 < ed.LEAF_SLOTS
    small_side = np.where((c[:, 0] >= 1) & (c[:, 0] <= 2), 0, 1)
    cs = c[np.arange(nb), small_side]
    cb = c[np.arange(nb), 1 - small_side]
    ok = one_leaf & room & (cs >= 1) & (cs <= 2) & (cb <= 6) & ~vm.dead(buckets)
    chosen, used = [], set()
    for b in np.nonzero(ok)[0][np.argsort(-cb[ok], kind="stable")]:  # the fullest first
        if int(leaf[b]) not in used and len(chosen) < 48:
            used.add(int(leaf[b]))
            chosen.append(int(b))
    chosen = np.array(chosen, dtype=np.int64)
    assert chosen.size >= ed.MIN_TARGETS, chosen.size
    small = ed.Targets(rig, both[chosen, small_side[chosen]], leaf[chosen])
    big = ed.Targets(rig, both[chosen, 1 - small_side[chosen]], leaf[chosen])
    s = cs[chosen]
    absent = np.array([[rig.key(p, low) for low in (3, (1 << min(rig.shift, 62)) - 5)] for p in small.p],
                      dtype=U64)
    held = ed.concat(small.keys())
    absent = absent.ravel()[~np.isin(absent.ravel(), held)]
    readers = np.concatenate([held, absent])

    def read(label, want, unsplit):
        """the small prefixes' keys: one class, no entry read, the oracle's
        answers; the class is asserted for the targets still unsplit"""
        gv, gf, st, cls = gp.searched(rig.t, readers)
        gp.assert_equal(readers, *rig.orc.search_batch(readers), gv, gf)
        gp.assert_rules(cls, gf, st, f"small prefixes, {label}")
        p, _ = rig.d.prefix_of(readers)
        mine = np.isin(p, small.p[unsplit])
        assert (cls[mine] == want).all(), (label, gp.tally(cls[mine]))
        assert bool(gf[:held.size].all()) and not gf[held.size:].any()
        _, _, st, _ = gp.searched(rig.t, readers[mine])
        assert st["entry_reads"] == 0 and st["gets"] == int(mine.sum()), (label, st)

    def bucket_state():
        return vm.dead(rig.t.vt_dump()[0])[chosen]

    # grow the larger prefix to 6: the bucket holds 7 or 8, alive
    fresh6 = big.fresh(6)
    add = ed.concat([fresh6[i, :6 - int(n)] for i, n in enumerate(cb[chosen])])
    if add.size:
        rig.apply(add, rig.values(add.size))
        rig.check(add, expect=("pair", "value"))
    ok_t = small.unsplit() & big.unsplit()
    assert np.all(big.counts()[ok_t] == 6) and np.all(small.counts()[ok_t] == s[ok_t])
    assert not bucket_state().any()
    read("bucket alive", T, ok_t)
    # the chunk that kills: to 9 keys per bucket
    more = big.fresh(3)
    kill = ed.concat([more[i, :3 - int(m)] for i, m in enumerate(s)])
    rig.apply(kill, rig.values(kill.size))
    rig.check(kill, expect=("pair", "value"))
    ok_t = small.unsplit() & big.unsplit()
    assert np.all(big.counts()[ok_t] + small.counts()[ok_t] == 9)
    assert bucket_state().all()
    read("bucket dead", V, ok_t)
    bigk = ed.concat([k for k, o in zip(big.keys(), ok_t) if o])
    gv, gf, st, cls = gp.searched(rig.t, bigk)
    gp.assert_equal(bigk, *rig.orc.search_batch(bigk), gv, gf)
    gp.assert_rules(cls, gf, st, "large prefixes, bucket dead")
    assert (cls == L).all() and bool(gf.all()) and st["entry_reads"] >= bigk.size, (gp.tally(cls), st)
    # two deletes in the larger prefix, back to 7 keys: dead all the same
    dele = ed.concat([k[:2] for k in big.keys()])
    rig.apply(dele, np.zeros(dele.size, dtype=U64))
    rig.check(dele, expect=("pair", "value"))
    ok_t = small.unsplit() & big.unsplit()
    assert np.all(big.counts()[ok_t] + small.counts()[ok_t] == 7)
    assert bucket_state().all()
    read("bucket dead, 7 keys", V, ok_t)
    bigk = np.concatenate([ed.concat([k for k, o in zip(big.keys(), ok_t) if o]), dele])
    gv, gf, st, cls = gp.searched(rig.t, bigk)
    gp.assert_equal(bigk, *rig.orc.search_batch(bigk), gv, gf)
    gp.assert_rules(cls, gf, st, "large prefixes, 7 keys")
    p, _ = rig.d.prefix_of(bigk)
    assert (cls[np.isin(p, big.p[ok_t])] == L).all(), gp.tally(cls)
    print(f"a bucket dies: {int(ok_t.sum())} unsplit targets of {chosen.size}")
    assert int(ok_t.sum()) >= ed.MIN_TARGETS, int(ok_t.sum())
    rig.finish()
