"""Pages below next_page that the tree does not reach, and every reader.

The rule (include/sherman_amd.h): no reader and no builder takes
data from a page the tree does not reach from its root.  The walks obey it by
construction.  The builders of a read phase (the pair-form directory, the
key-value bucket table) sweep the arena page by page, and the arena does hold
pages that look like leaves and belong to no tree: pages a failed take lost
(counted as used, never written), pages of an earlier tree above a reload, and
pages a loaded image carries along.  A sweep that trusted the page bytes would
put their entries into a live bucket, and a trusted bucket answers a get
before any leaf is read.

The truth of every case is the oracle over the handle's dumped image
(test_gpu_arena_full.truth): it walks from the root.  The pages that must not
be read come from tests/image_builder.soil_pages (S1, S2) or from the library
itself (S3); their keys are among the probes of every reader:

  absent   valid entries of keys the tree never held: a get must not find them
  shadow   valid entries of stored keys with another value
  deleted  valid entries of keys the tree holds as deleted slots

S1  an image loaded with six such pages behind it.
S2  the exact arenas of test_gpu_arena_full: the soil is loaded into the
    arena's last pages, the image alone after it, and the hot chunk fails in
    each writer mode; the pages the failed take lost still hold the soil.
S3  no image builder: a tree that filled the arena, shrunk by compact() or a
    bulk load, grown again until SHM_ENOMEM; the lost pages hold leaves of
    the first tree.
S4  (inside S2 and S3; printed in S1) the directory of the rebuild: no prefix
    of a soil key is unusable that a build over the reached pages would make
    usable.

Every precondition is computed on the host and asserted: the table is trusted,
the directory exact, at least 16 soil keys of each kind lie in buckets of at
most 8 keys (the soil's counted: a bucket the soil itself overfilled would go
dead and hide the fault), and the model of the answering path
(get_paths.classify) gives soil keys of each kind to the table.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import arena_model as am  # noqa: E402
import dir_model  # noqa: E402
import get_paths  # noqa: E402
import image_builder as ib  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import assert_same, dev, gpu_search, host, lib_ok, U64  # noqa: E402
import test_gpu_arena_full as full  # noqa: E402
import test_gpu_bulk as bulk  # noqa: E402
import test_gpu_tall as tall  # noqa: E402
import valtab_model  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402

PAGE = ib.PAGE
KEY_MAX = (1 << 64) - 1
KINDS = (ib.ABSENT, ib.SHADOW, ib.DELETED)
SWEPT = KINDS + (ib.OUTSIDE,)  # the kinds a sweep would take: valid entries


# ---- the readers ------------------------------------------------------------------
def soil_probes(soil):
    """every soil key of every kind, and its neighbours"""
    k = np.concatenate([np.asarray(soil[kind], dtype=U64) for kind in ib.SOIL_KINDS])
    p = np.concatenate([k, k + U64(1), k - U64(1)])
    return np.unique(p[(p != U64(KEY_MAX)) & (p != U64(0))])


def swept_keys(soil, kinds=SWEPT):
    return np.unique(np.concatenate([np.asarray(soil[k], dtype=U64) for k in kinds]))


def preconditions(t, kv, soil, kinds=KINDS, least=16):
    """the table trusted, the directory exact, and per kind: `least` soil keys
    in buckets of at most 8 keys with the soil's counted, one of them a
    key the table answers"""
    assert t.vt_stats()["trusted"], t.vt_stats()
    assert t.dir_stats()["exact"], t.dir_stats()
    table, directory, flags = get_paths.dumps(t)
    buckets, vi = table
    n = buckets.shape[0]
    cnt = valtab_model.counts(np.unique(np.concatenate([kv[0], swept_keys(soil)])),
                              vi["lo"], vi["shift"], n)
    for kind in kinds:
        k = np.asarray(soil[kind], dtype=U64)
        b = valtab_model.bucket_of(k, vi["lo"], vi["shift"])
        inside = (b >= 0) & (b < n)
        ok = k[inside][cnt[b[inside]] <= valtab_model.SLOTS]
        assert ok.size >= least, (kind, ok.size, k.size, vi)
        cls = get_paths.classify(ok, table, directory, flags)
        assert (cls == get_paths.TABLE).any(), (kind, get_paths.tally(cls))
    return vi


def other_readers(t, kv, probe, focus, what):
    """the readers tall.check_reads leaves out, against the truth's sorted
    contents: descending scans and floors, scans with a buffer each, the
    sorted export whole and in three ranges"""
    keys, vals = kv
    froms = np.unique(np.concatenate([probe[::probe.size // 2000 + 1],
                                      np.array([0, KEY_MAX - 1, KEY_MAX], dtype=U64)]))
    for limit in (1, 54):
        bulk.check_scans(t, keys, vals, froms, limit)  # scan_batch and rscan_batch
    froms = froms[froms != U64(KEY_MAX)]
    found, k, v = t.floor_batch(dev(froms))
    at = np.searchsorted(keys, froms, side="right") - 1
    has = at >= 0
    assert np.array_equal(found.cpu().numpy(), has), what
    at = np.maximum(at, 0)
    assert np.array_equal(host(k)[has], keys[at][has]), what
    assert np.array_equal(host(v)[has], vals[at][has]), what
    # a window around every probe: from the key below it to the key above it
    at = np.unique(np.concatenate([focus, probe[::probe.size // 2000 + 1]]))
    at = at[at != U64(0)]
    assert at.size <= tall.MAX_BATCH
    lo, hi = at - U64(1), np.minimum(at, U64(KEY_MAX - 2)) + U64(1)
    counts, got = t.range_query_slots(dev(lo), dev(hi), 8).result()
    counts, got = counts.cpu().numpy(), host(got)
    a = np.searchsorted(keys, lo, side="left")
    b = np.searchsorted(keys, hi, side="right")
    bad = np.nonzero(counts != b - a)[0]
    assert bad.size == 0, (what, bad.size, hex(int(at[bad[0]])), counts[bad[0]], (b - a)[bad[0]])
    assert (b - a).max() <= 8
    for i in np.nonzero(b > a)[0]:
        assert np.array_equal(np.sort(got[i, :counts[i]]), np.sort(vals[a[i]:b[i]])), (what, i)
    q = [keys[keys.size // 4], keys[keys.size // 2], keys[3 * keys.size // 4]] if keys.size > 4 \
        else [U64(1), U64(2), U64(3)]
    for lo1, hi1 in ((0, KEY_MAX), (0, int(q[0]) + 1), (int(q[0]) + 1, int(q[2])),
                     (int(q[1]), KEY_MAX - 1)):
        ek, ev = t.export(lo1, hi1)
        x = np.searchsorted(keys, U64(lo1), side="left")
        y = np.searchsorted(keys, U64(hi1), side="right")
        assert np.array_equal(host(ek), keys[x:y]) and np.array_equal(host(ev), vals[x:y]), \
            (what, hex(lo1), hex(hi1), ek.numel(), y - x)
    assert t.last_error()["bits"] == 0, (what, t.last_error())


def tree_checks(t, kv, what):
    """the diagnostics over the directory and the table as they stand"""
    if t.dir_stats()["exact"]:
        dv = t.dir_verify()
        assert dv["bad_lists"] == dv["bad_pairs"] == dv["bad_fps"] == dv["bad_vals"] == 0, (what, dv)
    bad, vinfo = valtab_model.check_tree(t, *kv)
    assert bad == [], (what, bad[:8], vinfo)


def every_reader(t, info, soil, what, monkeypatch, node_id=0, trees=True, keep=None):
    """Every reader of the handle against the oracle over its dumped image:
    as it stands, in a read phase, and (trees) from the dump loaded into a
    tree without a table and into each kind of tall.READ_TREES.  `keep`: with
    the preconditions once the table is trusted.  Returns the dump."""
    T, kv, probe = full.truth(t, info, [soil_probes(soil)])  # check() and stats() inside
    want = T.search_batch(probe)
    # no soil key is stored unless the tree holds it, whatever the pages say
    held = dict(zip(kv[0].tolist(), kv[1].tolist()))
    for kind in SWEPT:
        k = np.asarray(soil[kind], dtype=U64)
        assert all(held.get(int(x), 0) != int(x) ^ ib.SOIL_XOR for x in k), kind
    assert_same(probe, *want, *gpu_search(t, probe), what)
    tree_checks(t, kv, what)
    tall.check_reads(t, T, info, what)
    other_readers(t, kv, probe, soil_probes(soil), what)
    tall.enter_read_phase(t, probe)
    if keep is not None:
        preconditions(t, kv, soil, **keep)
    tree_checks(t, kv, what + ", read phase")
    assert_same(probe, *want, *gpu_search(t, probe), what + ", read phase")
    tall.check_reads(t, T, info, what + ", read phase")
    other_readers(t, kv, probe, soil_probes(soil), what + ", read phase")
    # the side state after the read phase's builds: no unreached page is tagged
    img, root, _, _ = tall.assert_side(t, what + ", read phase")
    if trees:
        size = dict(arena_bytes=img.nbytes + 4 * PAGE, max_batch=tall.MAX_BATCH, node_id=node_id)
        monkeypatch.setenv("SHM_VALTAB", "0")
        others = [("no table", shm.Tree(**size))]
        monkeypatch.delenv("SHM_VALTAB")
        others += [(kind, shm.Tree(**size, **args)) for kind, args in tall.READ_TREES.items()]
        for name, other in others:
            other.load_image(img, root)
            tall.assert_side(other, f"{what}, {name}, as loaded")
            assert_same(probe, *want, *gpu_search(other, probe), f"{what}, {name}, as loaded")
            for _ in range(6):  # its read phase
                got = gpu_search(other, probe)
            assert_same(probe, *want, *got, f"{what}, {name}, read phase")
            if name == "no table":
                assert not other.vt_stats()["trusted"], name
            else:
                tree_checks(other, kv, f"{what}, {name}")
            other.close()
    T.close()
    return img, root


def unusable_prefixes(t, keys):
    """S4: the prefixes of `keys` whose entry is not usable in the pair-form
    directory as it stands although a build over the pages the tree reaches
    makes it usable (dir_model.Image walks from the root)"""
    ent, di = t.dir_dump()
    assert ent.shape[0] and di["form"] == "pairs", di
    d = dir_model.Directory(ent, di["lo"], di["shift"])
    im = dir_model.Image(*t.dump_image())
    p, cov = d.prefix_of(np.asarray(keys, dtype=U64))
    p = np.unique(p[cov])
    fresh = dir_model.fresh_usable(im, d, p)
    return p[fresh & ~d.pair_usable[p]], int(fresh.sum())


def rebuild(t, probe):
    """a read phase's build from nothing: the hint set again drops the
    directory and the table, the next searches build both"""
    st = t.dir_stats()
    builds = st["builds"]
    t.set_key_range(*t._hint)
    tall.enter_read_phase(t, probe)
    assert t.dir_stats()["builds"] > builds, (st, t.dir_stats())
    assert t.vt_stats()["trusted"] and t.dir_stats()["exact"], (t.vt_stats(), t.dir_stats())


# ---- S1: a loaded image with unreached leaves ----------------------------------------
def entry_states_info(info):
    """check_reads' description of the entry-states image (no path pages)"""
    out = dict(full.flat_info(info["keys"], info["keys"]))
    out["deleted"] = np.concatenate([info["deleted"], info["torn"], info["stale_copy"]])
    return out


@functools.lru_cache(maxsize=None)
def s1_image(which, node_id):
    if which == "tall":
        img, root, info = ib.build_tall(2, "middle", True, node_id=node_id)
        hint = (0, 64)
        reads = info
    else:
        img, root, info = ib.build_entry_states(node_id=node_id)
        # node 3: a hint of half the key space, so that soil keys lie outside it
        hint = (0, 64) if node_id == 0 else (1 << 62, 63)
        reads = entry_states_info(info)
    pages, soil = ib.soil_pages(6, ib.soil_keys(info, hint=hint), seed=1, node_id=node_id,
                                first_page=img.size // PAGE)
    both = ib.with_soil(img, pages)
    both.setflags(write=False)
    return img, both, root, reads, soil, hint


@pytest.mark.parametrize("node_id", [0, 3])
@pytest.mark.parametrize("which", ["tall", "entry_states"])
def test_loaded_image_with_unreached_leaves(lib_ok, monkeypatch, which, node_id):
    """S1: the image with six soil pages behind it, loaded once: every reader
    answers what the oracle reads from the root, the table and the directory
    hold no soil entry, and the dump gives back the image's bytes."""
    img, both, root, info, soil, hint = s1_image(which, node_id)
    for mod in (full, tall):  # their oracles over this node's pointers
        monkeypatch.setattr(mod, "OracleTree", functools.partial(OracleTree, node_id=node_id))
    t = shm.Tree(arena_bytes=both.nbytes + 8 * PAGE, max_batch=tall.MAX_BATCH, node_id=node_id,
                 key_lo=hint[0], key_bits=hint[1])
    t._hint = hint
    t.dir_config(maint="always")
    t.load_image(both, root)
    assert t.stats()["pages_used"] == both.size // PAGE - 1
    reach = ib.reached_pages(both, root)
    assert reach.sum() == img.size // PAGE - 1 and not reach[img.size // PAGE:].any()
    if hint[1] < 64:  # the outside keys belong to no bucket: held to the readers alone
        assert soil[ib.OUTSIDE].size >= 16
    dump, droot = every_reader(t, info, soil, f"S1 {which} node {node_id}", monkeypatch,
                               node_id=node_id, keep={})
    # soil and all: a load changes no byte behind the superblock's page
    assert droot == root and np.array_equal(dump[PAGE:], both[PAGE:])
    bad, fresh = unusable_prefixes(t, swept_keys(soil))
    print(f"S1 {which} node {node_id}: {bad.size} of {fresh} soil prefixes unusable: {bad[:8]}")
    t.close()


# ---- S2: pages lost to a failed take -----------------------------------------------
def soiled_arena(path, spare):
    """full.exact_arena's arena after a load that filled it with soil: the
    image with `spare` soil pages first, the image alone after it, so the
    arena's last `spare` pages keep the soil above next_page"""
    img, root, info = full.image(path)
    n_img = img.size // PAGE
    pages, soil = ib.soil_pages(spare, ib.soil_keys(info, *ib.soil_sizes(spare)), seed=spare,
                                first_page=n_img)
    t = shm.Tree(arena_bytes=img.nbytes + spare * PAGE, max_batch=tall.MAX_BATCH)
    t._hint = (0, 64)
    t.load_image(ib.with_soil(img, pages), root)
    st = t.stats()
    assert st["pages_used"] == st["pages_capacity"] == n_img + spare - 1, st
    t.load_image(img, root)
    st = t.stats()
    assert st["pages_capacity"] - st["pages_used"] == spare, st
    t.dir_config(maint="always")
    for _ in range(8):
        gpu_search(t, info["keys"][:512])
        if t.vt_stats()["trusted"] and t.dir_stats()["exact"]:
            break
    assert t.vt_stats()["trusted"] and t.dir_stats()["exact"], (t.vt_stats(), t.dir_stats())
    return t, info, pages, soil


def surviving_soil(t, n_img, pages, soil):
    """the soil pages below pages_used that the tree does not reach and that
    still hold their soil bytes; their entries as a soil info"""
    dump, root = t.dump_image()
    pg = dump.reshape(-1, PAGE)
    reach = ib.reached_pages(dump, root)
    left = [i for i in range(pages.shape[0])
            if n_img + i < pg.shape[0] and not reach[n_img + i] and
            np.array_equal(pg[n_img + i], pages[i])]
    s = soil["slots"]
    on = np.isin(s["page"], left)
    return left, {k: np.sort(s["key"][on & (s["kind"] == k)]) for k in ib.SOIL_KINDS}


@pytest.mark.parametrize("mode", list(tall.MODES))
def test_pages_lost_to_a_failed_take(lib_ok, monkeypatch, mode):
    """S2: the hot chunk fails for want of pages in an arena whose last pages
    hold soil.  Whatever of it the failed take left below pages_used is read
    by nobody: before and after a read phase's rebuild, and after one more
    chunk of overwrites and deletes (a shadow key's among them)."""
    path = "middle"
    need, before, after = full.control(mode, path)
    n_img = full.image(path)[0].size // PAGE
    left_by = {}
    for spare in range(1, need):
        t, info, pages, soil = soiled_arena(path, spare)
        what = f"S2 {mode} spare {spare}"
        keys, vals = am.hot_chunk(info)
        assert shm._hooks().shm__upper_force(t.h, tall.MODES[mode]) == 0
        full.failed(lambda: t.insert_batch(dev(keys), dev(vals)), shm.SHM_ENOMEM)
        full.error_state(t, shm.SHM_ENOMEM, full.NOMEM, full.NOMEM | full.HANDOFF)
        left, alive = surviving_soil(t, n_img, pages, soil)
        left_by[spare] = left
        st = t.stats()
        print(f"{what}: soil pages left below pages_used {left} of {spare}, "
              f"pages {st['pages_used']}/{st['pages_capacity']}, "
              f"{ {k: alive[k].size for k in KINDS} } keys on them")
        T, kv, probe = full.truth(t, info, [soil_probes(soil)])
        T.close()
        am.classify_outcome(before, after, kv, [])
        # the table as the failed chunk's upkeep left it, then a rebuild over
        # the arena as it is now
        preconditions(t, kv, soil)
        if left:
            preconditions(t, kv, alive, least=1)
        dump1, _ = every_reader(t, info, soil, what, monkeypatch)
        rebuild(t, probe)
        preconditions(t, kv, soil)
        bad, fresh = unusable_prefixes(t, swept_keys(soil))
        assert bad.size == 0, (what, bad[:8], fresh)
        dump2, _ = every_reader(t, info, soil, what + ", rebuilt", monkeypatch, trees=False)
        assert np.array_equal(dump1, dump2)  # (so the trees loaded from it are the same)
        # one more chunk that needs no page
        tk, tv = kv
        at = np.linspace(0, tk.size - 1, 24).astype(np.int64)
        shadow = (alive if left and np.isin(alive[ib.SHADOW], tk).any() else soil)[ib.SHADOW]
        shadow = shadow[np.isin(shadow, tk)]
        assert shadow.size >= 2, what
        dele = np.unique(np.concatenate([tk[at[1::3]], shadow[:2]]))
        over = tk[at[0::3]]
        over = over[~np.isin(over, dele)]
        ck = np.concatenate([over, dele])
        cv = np.concatenate([over ^ U64(0x7777), np.zeros(dele.size, dtype=U64)])
        used = t.stats()["pages_used"]
        t.insert_batch(dev(ck), dev(cv))
        assert t.last_error()["bits"] == 0, t.last_error()
        assert t.stats()["pages_used"] == used
        gv, gf = gpu_search(t, ck)
        assert np.array_equal(gf != 0, cv != 0) and np.array_equal(gv[cv != 0], cv[cv != 0]), what
        every_reader(t, info, soil, what + ", after one more chunk", monkeypatch)
        rebuild(t, probe)
        gv, gf = gpu_search(t, ck)
        assert np.array_equal(gf != 0, cv != 0) and np.array_equal(gv[cv != 0], cv[cv != 0]), what
        every_reader(t, info, soil, what + ", rebuilt again", monkeypatch, trees=False)
        t.close()
    assert any(left_by.values()), f"{mode}: no spare of {sorted(left_by)} left a soil page: {left_by}"


# ---- S3: the library's own leftovers -------------------------------------------------
# The arena of each case, page 0 counted.  Where the second key set's chunks
# split leaves two ways every take is one page, and a take of one page that
# fails leaves none behind: an arena of 256 pages ran out with no page lost
# (host analysis over 20 .. 256 pages, gpu run of s3_tree alone).  A page is
# lost where the tree is still small against a chunk of 512 keys, so that a
# leaf splits into three and more pages at once; and it holds a leaf of the
# first tree only if that tree wrote the arena's last page, so the first tree
# grows until no page is free.  These sizes left one such page each.
S3_PAGES = {"compact": 56, "bulk_load": 32}
S3_FULL = 0        # the first tree grows until at most this many pages are free
S3_CHUNK = 512


def grow_to(t, orc, first, free_at_most):
    """hashed keys from id `first` on, in chunks that shrink as the arena
    fills (a chunk of one key takes at most a page per level and the root's),
    until at most free_at_most pages are free; no chunk may fail"""
    held = []
    while True:
        st = t.stats()
        free = st["pages_capacity"] - st["pages_used"]
        if free <= free_at_most:
            return np.concatenate(held), first
        n = S3_CHUNK if free > 64 else 16 if free > 24 else 1
        k = full.gen_keys(t, first, n)
        first += n
        v = k ^ U64(0x1111)
        t.insert_batch(dev(k), dev(v))
        assert t.last_error()["bits"] == 0, t.last_error()
        orc.apply_batch(k, v)
        held.append(k)
        if n > 1:
            gpu_search(t, k)


def stale_leaves(t, first_set):
    """the unreached pages below pages_used that a sweep takes for leaves and
    that hold valid entries of the first key set: (pages, keys, values)"""
    dump, root = t.dump_image()
    reach = ib.reached_pages(dump, root)
    pg, _, k, v = ib.sweep_entries(dump.reshape(-1, PAGE))
    on = ~reach[pg] & (pg > 0) & np.isin(k, first_set)
    return np.unique(pg[on]), k[on], v[on]


def s3_tree(shrink, arena_pages=None, full_at=S3_FULL):
    """the tree of S3 up to the chunk that returned SHM_ENOMEM: (tree, first
    key set, its deleted keys, its kept keys, the failing chunk's keys, pages
    used by the first tree, pages used after the shrink)"""
    arena_pages = arena_pages or S3_PAGES[shrink]
    t = shm.Tree(arena_bytes=arena_pages * PAGE, max_batch=tall.MAX_BATCH)
    t._hint = (0, 64)
    t.dir_config(maint="always")
    orc = OracleTree(1 << 24)
    first_set, nxt = grow_to(t, orc, 1, full_at)
    used_first = t.stats()["pages_used"]
    o = np.random.default_rng(5).permutation(first_set.size)
    gone, kept = first_set[o[:4 * o.size // 5]], first_set[o[4 * o.size // 5:]]
    for k, v in ((gone, np.zeros(gone.size, dtype=U64)), (kept, kept ^ U64(0x2222))):
        for a in range(0, k.size, 4096):
            t.insert_batch(dev(k[a:a + 4096]), dev(v[a:a + 4096]))
            orc.apply_batch(k[a:a + 4096], v[a:a + 4096])
    assert t.last_error()["bits"] == 0 and t.stats()["pages_used"] == used_first
    if shrink == "compact":
        t.compact()
    else:
        run = np.sort(full.gen_keys(t, 1 << 30, 50))
        assert not np.isin(run, first_set).any()
        t.bulk_load(dev(run), dev(run ^ U64(0x3333)))
        orc.close()
        orc = OracleTree(1 << 24)
        orc.apply_batch(run, run ^ U64(0x3333))
    small = t.stats()["pages_used"]
    assert small <= used_first // 2, (small, used_first)
    tall.check_contents(t, orc, f"S3 after {shrink}")
    orc.close()
    # the second set, disjoint from the first, until the arena runs out
    nxt = 1 << 20
    for _ in range(64):
        k = full.gen_keys(t, nxt, S3_CHUNK)
        nxt += S3_CHUNK
        assert not np.isin(k, first_set).any()
        try:
            t.insert_batch(dev(k), dev(k ^ U64(0x4444)))
        except shm.ShermanError as e:
            assert e.rc == shm.SHM_ENOMEM, e
            return t, first_set, gone, kept, k, used_first, small
        for _ in range(6):
            gpu_search(t, k)
    raise AssertionError("the arena never ran out")


@pytest.mark.parametrize("shrink", ["compact", "bulk_load"])
def test_leftovers_of_an_earlier_tree(lib_ok, monkeypatch, shrink):
    """S3: a tree of hashed keys fills the arena; four fifths of it are
    deleted and the rest overwritten; compact() (or a bulk load of a 50-key
    run) shrinks it; a disjoint key set grows it until SHM_ENOMEM.  The pages
    the failed take lost hold leaves of the first tree.  After the bulk load
    every key of the first set is absent.  After compact() the fifth that was
    kept is stored, and the stale pages hold the same pairs; so half of the
    keys found there are then deleted and the other half overwritten, and no
    reader may see a stale pair after the next rebuild either."""
    t, first_set, gone, kept, k, used_first, small = s3_tree(shrink)
    full.error_state(t, shm.SHM_ENOMEM, full.NOMEM, full.NOMEM | full.HANDOFF)
    pages, sk, sv = stale_leaves(t, first_set)
    st = t.stats()
    print(f"S3 {shrink}: first tree {used_first} pages, {small} after the shrink, now "
          f"{st['pages_used']}/{st['pages_capacity']}; unreached pages with valid entries of the "
          f"first set: {pages.tolist()} ({sk.size} entries)")
    assert pages.size >= 1, "no page of the first tree was lost to the failed take"
    stale = {kind: np.zeros(0, dtype=U64) for kind in ib.SOIL_KINDS}
    stale[ib.ABSENT] = np.unique(sk)  # (their kind is decided by the truth below)
    info = dict(full.flat_info(first_set, sk), deleted=gone[:2000])
    what = f"S3 {shrink}"
    T, kv, probe = full.truth(t, info, [first_set, k])
    T.close()
    in_tree = np.isin(first_set, kv[0])
    if shrink == "bulk_load":
        assert not in_tree.any()
    else:
        assert np.array_equal(np.sort(first_set[in_tree]), np.sort(kept))
    gv, gf = gpu_search(t, first_set)
    assert np.array_equal(gf != 0, in_tree), (what, int((gf != 0).sum()), int(in_tree.sum()))

    def stage(what, trees):
        every_reader(t, info, stale, what, monkeypatch, trees=trees)
        rebuild(t, probe)
        T, kv, _ = full.truth(t, info, [first_set])
        T.close()
        cls = get_paths.classify(stale[ib.ABSENT], *get_paths.dumps(t))
        assert (cls == get_paths.TABLE).any(), (what, get_paths.tally(cls))
        bad, fresh = unusable_prefixes(t, stale[ib.ABSENT])
        assert bad.size == 0, (what, bad[:8], fresh)
        every_reader(t, info, stale, what + ", rebuilt", monkeypatch, trees=False)
        gv, gf = gpu_search(t, first_set)
        assert np.array_equal(gf != 0, np.isin(first_set, kv[0])), what

    stage(what, True)
    # the keys of the stale pages that the tree still holds: half deleted, half
    # overwritten, in place
    live = np.unique(sk[np.isin(sk, kv[0])])
    if shrink == "compact":
        assert live.size >= 2, live.size
    if live.size:
        ck = live
        cv = np.where(np.arange(live.size) % 2 == 0, U64(0), live ^ U64(0x5555))
        used = t.stats()["pages_used"]
        t.insert_batch(dev(ck), dev(cv))
        assert t.last_error()["bits"] == 0 and t.stats()["pages_used"] == used
        stage(what + ", stale keys changed", False)
        gv, gf = gpu_search(t, ck)
        assert np.array_equal(gf != 0, cv != 0) and np.array_equal(gv[cv != 0], cv[cv != 0]), what
    t.close()
