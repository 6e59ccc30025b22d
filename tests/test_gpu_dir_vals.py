"""The value form of the leaf directory (layout.h kDirVals): in a read phase
a pair-form entry of a prefix that holds at most two keys carries their
(key, value) inline, and an exact directory's get of such a prefix is
answered by its entry alone (get_sum.hip).  The copies must equal the tree for as
long as the flag is trusted: builds, repairs, split pages and the chunks'
upkeep (dir_upkeep.h) are checked here against the CPU oracle and by
shm__dir_verify, which compares every value-form entry with the tree.

Shapes follow test_gpu_dir.py's loaded(): 2^18 hashed keys, a 512 MB arena,
chunks of at most 2^18 ops; five searches reach the read phase (a directory
of 2^17 entries: two keys per prefix on average, C2's ratio).
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dir_model  # noqa: E402
import get_paths as gp  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import (assert_same, dev, gen_keys, gpu_search,  # noqa: E402
                         gpu_search_stats, host, lib_ok, U64)
from oracle.pyoracle import OracleTree  # noqa: E402

pytestmark = pytest.mark.gpu

N0 = 1 << 18
ARENA = 512 << 20


def loaded(maint="always", max_batch=1 << 18, **kw):
    """A tree of N0 hashed keys in its read phase (five searches), and its
    oracle."""
    t = shm.Tree(arena_bytes=ARENA, max_batch=max_batch, **kw)
    t.dir_config(maint=maint)
    orc = OracleTree(ARENA)
    base = gen_keys(t, 1, N0)
    bv = np.arange(1, N0 + 1, dtype=U64) * U64(2)
    for c in range(0, N0, max_batch):
        t.insert_batch(dev(base[c:c + max_batch]), dev(bv[c:c + max_batch]))
    orc.apply_batch(base, bv)
    for _ in range(5):
        gpu_search(t, base[:4096])
    d = t.dir_stats()
    assert d["form"] == "pairs", d
    return t, orc, base


def loaded_table(table, **kw):
    """loaded() with the key-value bucket table ("on": the default) or
    without one ("off": SHM_VALTAB=0 while the tree is created).  Off, the
    directory's entries are all a get has; on, they serve only the keys of
    dead buckets, and the tests ask the model (tests/get_paths.py) which."""
    t, orc, base = loaded(**kw) if table == "on" else gp.without_table(lambda: loaded(**kw))
    vs = t.vt_stats()
    assert vs["trusted"] if table == "on" else vs["buckets"] == 0, (table, vs)
    return t, orc, base


class Prefixes:
    """The directory's prefixes of a key set, on the host: key >> shift for a
    directory of `entries` prefixes over the 64-bit key space."""

    def __init__(self, t, keys):
        ent = t.dir_stats()["entries"]
        assert ent and ent & (ent - 1) == 0
        self.shift = U64(64 - (ent.bit_length() - 1))
        self.entries = ent
        self.keys = np.sort(keys)
        self.pref = self.keys >> self.shift
        self.count = np.bincount(self.pref.astype(np.int64), minlength=ent)

    def of(self, k):
        return (k >> self.shift).astype(np.int64)

    def held(self, k):
        """number of stored keys in each key's prefix"""
        return self.count[self.of(k)]

    def members(self, prefixes):
        """the stored keys of these prefixes and of their two neighbours"""
        p = np.unique(np.concatenate([prefixes - 1, prefixes, prefixes + 1]))
        p = p[(p >= 0) & (p < self.entries)]
        return self.keys[np.isin(self.pref.astype(np.int64), p)]

    def fresh_in(self, prefixes, rng, stored):
        """one key, not stored, inside each given prefix"""
        low = rng.integers(1, 1 << int(self.shift), prefixes.size).astype(U64)
        k = (prefixes.astype(U64) << self.shift) | low
        k = np.unique(k[~np.isin(k, stored)])
        return k[k != U64(shm.KEY_MAX)]


def verify_clean(t):
    v = t.dir_verify()
    assert (v["bad_lists"], v["bad_pairs"], v["bad_fps"], v["bad_vals"]) == (0, 0, 0, 0), v
    # and the host model on the raw dumps (tests/dir_model.py): the inline
    # copies against the pages, by code the library does not share
    bad, _ = dir_model.check_tree(t)
    assert bad == [], bad
    return v


def _small_prefixes(table):
    """Stored probes whose prefix holds at most two keys read no leaf entry:
    with q their share, a batch reads at most 1.05 (1 - q) entries per get
    (the 5 %: fingerprint false candidates), every get is still answered
    from its directory entry, absent keys are absent, and the verify finds
    value-form entries, none wrong.  Without the bucket table that is the
    whole batch; with it, the batch of the probes the model does not give to
    the table (a live bucket answers before the entry is read, and counts as
    a get answered from its entry with no entry read).  Both: at least one
    entry read per stored probe the model sends to the leaves, none in a
    batch it sends nowhere near them."""
    t, orc, base = loaded_table(table)
    px = Prefixes(t, base)
    rng = np.random.default_rng(21)
    probe = base[rng.integers(0, N0, 1 << 15)]
    q = float(np.mean(px.held(probe) <= 2))
    assert 0.3 < q < 0.5, q  # 1 + Poisson(2) keys in a key's prefix: 40.6 %

    def upper(st, keys, found):
        qk = float(np.mean(px.held(keys) <= 2))
        print(f"q={qk:.4f} gets={st['gets']} entry_reads={st['entry_reads']} "
              f"dir_fp_hits={st['dir_fp_hits']} bound={1.05 * (1 - qk) * st['gets']:.0f}")
        assert bool(found.all()) and st["dir_fp_hits"] == st["gets"], st
        assert st["entry_reads"] <= 1.05 * (1 - qk) * st["gets"], (qk, st)

    _, _, st, cls = gp.check_paths(t, orc, probe, table == "on", f"small prefixes, table {table}", upper)
    assert st["dir_fp_hits"] == st["gets"], st
    if table == "on":  # uniform keys, four per bucket: 94.8 % in live buckets
        assert np.mean(cls == gp.TABLE) > 0.9, gp.tally(cls)
    else:  # the value form's share is q: a prefix of at most two keys is held inline
        assert np.array_equal(cls == gp.VALUE, px.held(probe) <= 2), gp.tally(cls)
    absent = gen_keys(t, N0 + 1, 1 << 13)
    gv, gf = gpu_search(t, absent)
    assert_same(absent, *orc.search_batch(absent), gv, gf)
    v = verify_clean(t)
    assert v["vals_checked"] > 0, v
    orc.close()
    t.close()


def test_small_prefixes_are_answered_by_the_entry_alone(lib_ok):
    """with the bucket table (the default tree)"""
    _small_prefixes("on")


def test_small_prefixes_are_answered_by_the_entry_alone_without_the_table(lib_ok):
    """on a tree made without a bucket table: every probe goes through its entry"""
    _small_prefixes("off")


def _chunks_keep_the_copies(table):
    """Upkeep on for every chunk: in-place updates and deletes of keys held
    inline, new keys into prefixes of 0, 1 and 2 keys, and runs of 30 keys
    that split leaves, one chunk each.  After each: the touched keys and
    their prefixes' neighbours equal the oracle, the verify is clean, the
    directory was not rebuilt, and gets are still answered by value-form
    entries (fewer entry reads than hits: over the whole batch without the
    bucket table, over the probes the model does not give to the table with
    it), under the model's rules for each path (get_paths.check_paths)."""
    t, orc, base = loaded_table(table)
    px = Prefixes(t, base)
    rng = np.random.default_rng(22)
    builds = t.dir_stats()["builds"]
    small = px.keys[px.held(px.keys) <= 2]  # held inline
    pick = rng.permutation(small.size)
    upd, dele = small[pick[:3000]], small[pick[3000:6000]]
    # prefixes by their key count, away from the ones touched above
    taken = np.unique(np.concatenate([px.of(upd), px.of(dele)]))
    free = np.setdiff1d(np.arange(px.entries), taken)
    new_p = np.concatenate([rng.permutation(free[px.count[free] == c])[:1500] for c in (0, 1, 2)])
    new = px.fresh_in(new_p, rng, base)
    anchors = base[rng.integers(0, N0, 100)]
    runs = np.unique((anchors[:, None] + np.arange(1, 31, dtype=U64)[None, :]).ravel())
    runs = runs[~np.isin(runs, np.concatenate([base, new]))]
    sample = base[rng.integers(0, N0, 1 << 13)]
    chunks = [
        ("update", upd, upd ^ U64(0x5A5A5A)),
        ("delete", dele, np.zeros(dele.size, dtype=U64)),
        ("new", new, new ^ U64(0x1234567)),
        ("split", runs, runs ^ U64(0x77)),
    ]
    for name, k, v in chunks:
        t.insert_batch(dev(k), dev(v))
        orc.apply_batch(k, v)
        stored, _ = orc.dump()
        touched = np.unique(np.concatenate([k, Prefixes(t, stored).members(np.unique(px.of(k))),
                                            k + U64(1)]))
        # (+ a fixed sample of the first load: the split chunk's own keys sit
        # in prefixes of ~30 keys, which no pair-form entry lists)
        touched = np.unique(np.concatenate([touched, sample]))
        touched = touched[(touched != U64(shm.KEY_MAX)) & (touched != U64(0))]
        def upper(st, keys, found, name=name):  # value-form answers still occur
            assert st["entry_reads"] < st["hits"], (name, st)

        on, held_to_bound = table == "on", touched
        if on and name == "split":
            # The run keys sit in prefixes of ~30 keys, which no pair-form
            # entry lists: each is a summary walk with false candidates.
            # Without the table the sample's value-form hits (40 % of it)
            # outweigh those; with it the sample's share outside the table
            # is 5 %, so the bound is held on the other probes, and the runs
            # on the rules alone.
            gp.check_paths(t, orc, touched, True, f"{name}, table on, with the runs")
            held_to_bound = touched[~np.isin(touched, runs)]
        _, _, st, _ = gp.check_paths(t, orc, held_to_bound, on, f"{name}, table {table}", upper)
        v1 = verify_clean(t)
        print(name, st, v1)
        assert v1["vals_checked"] > 0, (name, v1)
        assert t.dir_stats()["builds"] == builds, (name, t.dir_stats())
        assert t.vt_stats()["trusted"] == (table == "on"), (name, t.vt_stats())
    assert t.last_error()["bits"] == 0
    rc, oc = orc.check()
    assert rc == 0 and t.check()["keys"] == oc["keys"]
    orc.close()
    t.close()


def test_chunks_keep_the_inline_copies_equal_to_the_tree(lib_ok):
    """with the bucket table (the default tree)"""
    _chunks_keep_the_copies("on")


def test_chunks_keep_the_inline_copies_equal_to_the_tree_without_the_table(lib_ok):
    """on a tree made without a bucket table"""
    _chunks_keep_the_copies("off")


def _chunks_without_upkeep(how, table):
    """Chunks that do not keep the directory -- the upkeep switched off after
    the build, or the default policy's chunk with no search before it --
    leave stale inline copies (and, with a bucket table, stale buckets)
    behind; the directory is then not exact and the gets ignore both:
    updated and deleted keys equal the oracle, the model sends every probe
    to the leaves, and every stored one does read a leaf entry."""
    t, orc, base = loaded_table(table, maint="always" if how == "off" else True)
    px = Prefixes(t, base)
    rng = np.random.default_rng(23)
    assert t.dir_verify()["vals_checked"] > 0
    small = px.keys[px.held(px.keys) <= 2]
    pick = rng.permutation(small.size)
    upd, dele = small[pick[:4000]], small[pick[4000:8000]]
    if how == "off":
        t.dir_config(maint=False)
    else:  # a searched chunk is kept; the next one, unsearched, is not
        warm = small[pick[8000:8100]]
        t.insert_batch(dev(warm), dev(warm ^ U64(3)))
        orc.apply_batch(warm, warm ^ U64(3))
    k = np.concatenate([upd, dele])
    v = np.concatenate([upd ^ U64(0xABCDEF), np.zeros(dele.size, dtype=U64)])
    t.insert_batch(dev(k), dev(v))
    orc.apply_batch(k, v)
    assert not t.dir_stats()["exact"] and not t.vt_stats()["trusted"]
    probe = np.concatenate([k, small[pick[8000:12000]]])
    _, gf, st, cls = gp.check_paths(t, orc, probe, False, f"unkept chunk ({how}), table {table}")
    assert (cls == gp.LEAF).all(), gp.tally(cls)
    assert st["entry_reads"] >= int(gf.sum()) == st["hits"] > 0, st
    assert not t.vt_stats()["trusted"]
    orc.close()
    t.close()


@pytest.mark.parametrize("how", ["off", "unsearched"])
def test_chunks_without_upkeep_end_the_trust(lib_ok, how):
    """with the bucket table: its trust ends with the directory's"""
    _chunks_without_upkeep(how, "on")


@pytest.mark.parametrize("how", ["off", "unsearched"])
def test_chunks_without_upkeep_end_the_trust_without_the_table(lib_ok, how):
    """on a tree made without a bucket table"""
    _chunks_without_upkeep(how, "off")


def _stored_batch_reads_every_hit(t, orc, base):
    rng = np.random.default_rng(24)
    probe = np.concatenate([base[rng.integers(0, N0, 1 << 15)], gen_keys(t, N0 + 1, 1 << 12)])
    gv, gf, st = gpu_search_stats(t, probe)
    assert_same(probe, *orc.search_batch(probe), gv, gf)
    assert st["hits"] == 1 << 15 and st["entry_reads"] >= st["hits"], st


def test_page_check_never_uses_the_form(lib_ok):
    """SHM_FLAG_PAGE_CHECK reads the hit's page versions: every hit reads its
    leaf entry, value form or not; same results."""
    t, orc, base = loaded(page_check=True)
    _stored_batch_reads_every_hit(t, orc, base)
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()


def test_switch_off_builds_plain_pair_entries(lib_ok):
    """SHM_DIR_VALS=0 (read when the tree is created): no value-form entry
    is built, every hit reads its leaf entry; same results."""
    old = os.environ.get("SHM_DIR_VALS")
    os.environ["SHM_DIR_VALS"] = "0"
    try:
        t, orc, base = loaded()
    finally:
        if old is None:
            del os.environ["SHM_DIR_VALS"]
        else:
            os.environ["SHM_DIR_VALS"] = old
    _stored_batch_reads_every_hit(t, orc, base)
    v = verify_clean(t)
    assert v["checked"] > 0 and v["vals_checked"] == 0, v
    orc.close()
    t.close()


def test_ordering_on_a_second_stream_does_not_reach_the_upkeep(lib_ok):
    """the upkeep of chunk i reads its op buffers after k_upper,
    while insert_order of chunk i + 2 (same buffer parity) may already be
    queued on another stream.  Eight rounds of insert_order(i + 1) on stream
    B, a search on stream A, insert_apply(i) on A; chunks mix new keys into
    populated prefixes with updates of keys held inline.  Every search
    equals the oracle's state at that point, and the directory verifies."""
    mb = 1 << 14
    t, orc, base = loaded(max_batch=mb)
    px = Prefixes(t, base)
    rng = np.random.default_rng(25)
    builds = t.dir_stats()["builds"]
    small = px.keys[px.held(px.keys) <= 2]
    populated = np.nonzero((px.count >= 1) & (px.count <= 2))[0]
    stored = base
    batches = []
    for r in range(9):
        new = px.fresh_in(rng.permutation(populated)[:6000], rng, stored)
        upd = np.unique(small[rng.integers(0, small.size, 6000)])
        k = np.concatenate([new, upd])
        v = rng.integers(1, 1 << 62, k.size).astype(U64)
        assert k.size <= mb
        stored = np.concatenate([stored, new])
        batches.append((dev(k), dev(v), k, v))
    probe_h = np.unique(np.concatenate([b[2] for b in batches] + [base[:4096]]))
    probe = dev(probe_h)
    torch.cuda.synchronize()
    s_ord, s_app = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    tickets = [t.insert_order(batches[0][0], batches[0][1], stream=s_ord)]
    for i in range(8):
        tickets.append(t.insert_order(batches[i + 1][0], batches[i + 1][1], stream=s_ord))
        v = torch.empty_like(probe)
        f = torch.empty(probe.numel(), dtype=torch.uint8, device="cuda")
        t.search_batch(probe, v, f, stream=s_app)
        outs.append((v, f))
        t.insert_apply(tickets[i], stream=s_app)
    t.insert_apply(tickets[8], stream=s_app)
    t.synchronize()
    torch.cuda.synchronize()
    for i, (gv, gf) in enumerate(outs):  # search i saw chunks 0 .. i - 1
        ov, of = orc.search_batch(probe_h)
        assert_same(probe_h, ov, of, host(gv), gf.cpu().numpy())
        orc.apply_batch(batches[i][2], batches[i][3])
    orc.apply_batch(batches[8][2], batches[8][3])
    gv, gf = gpu_search(t, probe_h)
    assert_same(probe_h, *orc.search_batch(probe_h), gv, gf)
    v1 = verify_clean(t)
    assert v1["vals_checked"] > 0, v1
    assert t.dir_stats()["builds"] == builds
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()
