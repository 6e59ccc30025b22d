"""Sorted export and compaction on the GPU (Tree.export / count / compact ->
shm_export / shm_compact -> export.hip).

Expected results come from tests/export_model.py on the tree's own
dump_image() (a numpy walk sharing no code with the library), and from the
CPU oracle where the oracle holds the same tree.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bulk_model as bm  # noqa: E402
import export_model as em  # noqa: E402
import image_builder as ib  # noqa: E402
import sherman_amd as shm  # noqa: E402
from gpu_helpers import dev, gpu_search, host, lib_ok, SENT, U64  # noqa: E402
from oracle.pyoracle import OracleTree  # noqa: E402
from rscan_model import RScanModel  # noqa: E402
from scan_model import ScanModel  # noqa: E402

KEY_MAX = (1 << 64) - 1
PAGE = 1024
ARENA = 64 << 20
MAX_BATCH = 1 << 14


def tree(**kw):
    return shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH, **kw)


def sentinels(n):
    return torch.full((n,), SENT, dtype=torch.int64, device="cuda")


def raw_export(t, lo, hi, keys, vals, cap):
    """shm_export itself: (status, n_out)"""
    n = ctypes.c_uint64(1 << 60)
    rc = shm.lib().shm_export(t.h, lo, hi, shm._ptr(keys), shm._ptr(vals), cap, ctypes.byref(n),
                              None)
    return rc, int(n.value)


def assert_export(t, keys, vals, lo=0, hi=KEY_MAX, what=""):
    """the export of [lo, hi] equals keys / vals, the count too, and no word
    past the pairs is written"""
    n = keys.size
    assert t.count(lo, hi) == n, (what, t.count(lo, hi), n)
    ko, vo = sentinels(n + 1), sentinels(n + 1)
    rc, got = raw_export(t, lo, hi, ko, vo, n)
    assert rc == shm.SHM_OK and got == n, (what, rc, got, n)
    gk, gv = host(ko), host(vo)
    assert gk[n] == U64(SENT) and gv[n] == U64(SENT), what
    bad = np.nonzero((gk[:n] != keys) | (gv[:n] != vals))[0]
    assert bad.size == 0, (what, bad.size, int(bad[0]), hex(int(gk[bad[0]])), hex(int(keys[bad[0]])))
    assert t.last_error()["bits"] == 0, (what, t.last_error())


def assert_gets(t, keys, vals, absent, what):
    gv, gf = gpu_search(t, keys)
    bad = np.nonzero((gf != 1) | (gv != vals))[0]
    assert bad.size == 0, (what, bad.size, [hex(int(keys[i])) for i in bad[:4]])
    if absent.size:
        gv, gf = gpu_search(t, absent)
        bad = np.nonzero((gf != 0) | (gv != 0))[0]
        assert bad.size == 0, (what, "absent", bad.size, [hex(int(absent[i])) for i in bad[:4]])


def neighbours(keys, cap=2000):
    k = keys[::keys.size // cap + 1] if keys.size else keys
    p = np.concatenate([k + U64(1), k - U64(1), np.array([0, 1, KEY_MAX - 1], dtype=U64)])
    return np.unique(p[~np.isin(p, keys) & (p != U64(KEY_MAX))])


def model_of(t):
    img, root = t.dump_image()
    return em.export(img, root, node_id=t.node_id)


@functools.lru_cache(maxsize=None)
def shape(n, lf, inf):
    keys = bm.shape_keys(n, bm.shape_kind(n, lf, inf))
    vals = bm.shape_vals(keys)
    for a in (keys, vals):
        a.setflags(write=False)
    return keys, vals


@functools.lru_cache(maxsize=None)
def entry_states():
    img, root, info = ib.build_entry_states()
    img.setflags(write=False)
    return img, root, info


# ---- 1. loaded shapes -------------------------------------------------------------

@pytest.mark.parametrize("n,lf,inf", bm.SHAPES)
def test_export_of_loaded_shapes(lib_ok, n, lf, inf):
    """the empty tree, one key, exactly full pages, root levels 0..7"""
    keys, vals = shape(n, lf, inf)
    t = tree()
    t.bulk_load(dev(keys), dev(vals), lf, inf)
    assert_export(t, keys, vals, what=(n, lf, inf))
    k, v = t.export()
    assert k.numel() == v.numel() == n
    assert np.array_equal(host(k), keys) and np.array_equal(host(v), vals)
    mk, mv = model_of(t)
    assert np.array_equal(mk, keys) and np.array_equal(mv, vals)
    t.close()


def test_keys_only_and_values_only(lib_ok):
    keys, vals = shape(5000, 0, 0)
    n = keys.size
    t = tree()
    t.bulk_load(dev(keys), dev(vals))
    ko, vo = sentinels(n + 1), sentinels(n + 1)
    assert raw_export(t, 0, KEY_MAX, ko, None, n) == (shm.SHM_OK, n)
    assert np.array_equal(host(ko)[:n], keys) and host(ko)[n] == U64(SENT)
    assert (host(vo) == U64(SENT)).all()
    ko = sentinels(n + 1)
    assert raw_export(t, 0, KEY_MAX, None, vo, n) == (shm.SHM_OK, n)
    assert np.array_equal(host(vo)[:n], vals) and host(vo)[n] == U64(SENT)
    assert (host(ko) == U64(SENT)).all()
    k, v = t.export(keys=sentinels(n + 3))
    assert v is None and np.array_equal(host(k), keys)
    k, v = t.export(vals=sentinels(n))
    assert k is None and np.array_equal(host(v), vals)
    t.close()


# ---- 2. images --------------------------------------------------------------------

def image_cases():
    yield "tall4", lambda: ib.build_tall(4, "middle", True)
    yield "tall7", lambda: ib.build_tall(7, "right", False)
    yield "entry_states", lambda: entry_states()
    for name, r, l1 in (("dropped_both", True, True), ("dropped_root", True, False),
                        ("dropped_level1", False, True)):
        def make(r=r, l1=l1):
            img, root, info = entry_states()
            return em.drop_last_separators(img, root, in_root=r, in_level1=l1), root, info
        yield name, make


@pytest.mark.parametrize("name,make", list(image_cases()), ids=[c[0] for c in image_cases()])
def test_export_of_images(lib_ok, name, make):
    """Pages in shuffled order, the 53-entry hot leaf in shuffled slots, leaves
    whose entries are all deleted (build_tall); torn entries, stale copies,
    f = r = 15, a last leaf with no valid entry (build_entry_states); leaves
    and level-1 pages that only their left sibling reaches."""
    img, root, info = make()
    t = tree()
    t.load_image(img, root)
    mk, mv = em.export(img, root)
    assert np.array_equal(mk, info["keys"]) and np.array_equal(mv, info["vals"])
    assert_export(t, info["keys"], info["vals"], what=name)
    if "n_valid" in info:
        assert t.count() == info["n_valid"] == 478
        if name == "entry_states":
            assert t.check()["keys"] == 503  # the structural check counts torn entries
    # and one scan from 0 gives the same pairs
    n = info["keys"].size
    c, k, v = t.scan_batch(dev([0]), n + 1).result()
    assert int(c[0]) == n
    assert np.array_equal(host(k)[0, :n], info["keys"]) and np.array_equal(host(v)[0, :n], info["vals"])
    t.close()


# ---- 3. ranges --------------------------------------------------------------------

def range_ends(keys, fences):
    ks = [int(keys[0]), int(keys[-1]), int(keys[keys.size // 2]), int(keys[keys.size // 3])]
    ends = {0, 1, KEY_MAX - 1, KEY_MAX}
    for k in ks:
        ends |= {k, k + 1, max(k - 1, 0)}
    for f in fences:
        ends |= {int(f), max(int(f) - 1, 0)}
    return sorted(e for e in ends if 0 <= e <= KEY_MAX)


def check_ranges(t, keys, vals, fences, seed):
    model = ScanModel(keys, vals)
    ends = range_ends(keys, fences)
    los = [lo for lo in ends for _ in ends]
    his = [hi for _ in ends for hi in ends]
    absent = neighbours(keys, 10)
    los += [int(keys[5]), int(absent[3]), int(keys[9]), KEY_MAX, 0]
    his += [int(keys[5]), int(absent[3]), int(keys[4]), KEY_MAX, KEY_MAX]
    rng = np.random.default_rng(seed)
    rl = rng.integers(0, KEY_MAX, 300, dtype=np.uint64)
    rh = rl + (rng.integers(0, KEY_MAX, 300, dtype=np.uint64) >> rng.integers(0, 60, 300).astype(U64))
    rh[rh < rl] = U64(KEY_MAX)
    los += [int(x) for x in rl]
    his += [int(x) for x in rh]
    a, b = model.bounds(np.array(los, dtype=U64), np.array(his, dtype=U64))
    cap = keys.size + 1
    ko, vo = sentinels(cap), sentinels(cap)
    kd, vd = dev(keys), dev(vals)
    for lo, hi, x, y in zip(los, his, a, b):
        n = int(y - x) if lo <= hi else 0
        rc, got = raw_export(t, lo, hi, ko, vo, cap)
        assert rc == shm.SHM_OK and got == n, (hex(lo), hex(hi), rc, got, n)
        if n:
            assert torch.equal(ko[:n], kd[x:y]) and torch.equal(vo[:n], vd[x:y]), (hex(lo), hex(hi))
    assert t.count(7, 3) == 0 and t.count(KEY_MAX, KEY_MAX) == 0 and t.count(KEY_MAX) == 0
    assert t.count(0, KEY_MAX) == t.count() == keys.size
    assert t.last_error()["bits"] == 0


def test_ranges_on_the_entry_states(lib_ok):
    img, root, info = entry_states()
    t = tree()
    t.load_image(img, root)
    check_ranges(t, info["keys"], info["vals"], info["leaf_lo"][[1, 2, 8, 39]], 1)
    t.close()


def test_ranges_on_a_loaded_tree(lib_ok):
    keys, vals = shape(5000, 0, 0)
    t = tree()
    t.bulk_load(dev(keys), dev(vals))
    first = bm.deal(keys.size, bm.plan(keys.size)["level_pages"][0])
    check_ranges(t, keys, vals, keys[first[[1, 2, 41, 138]]], 2)
    t.close()


# ---- 4. capacity ------------------------------------------------------------------

def test_capacity(lib_ok):
    keys, vals = shape(5000, 0, 0)
    n = keys.size
    t = tree()
    t.bulk_load(dev(keys), dev(vals))
    ko, vo = sentinels(n), sentinels(n)
    assert raw_export(t, 0, KEY_MAX, ko, vo, n) == (shm.SHM_OK, n)
    assert np.array_equal(host(ko), keys) and np.array_equal(host(vo), vals)
    for which in ("both", "keys", "vals"):
        ko, vo = sentinels(n), sentinels(n)
        rc, got = raw_export(t, 0, KEY_MAX, ko if which != "vals" else None,
                             vo if which != "keys" else None, n - 1)
        assert (rc, got) == (shm.SHM_ENOSPC, n), which
        assert (host(ko) == U64(SENT)).all() and (host(vo) == U64(SENT)).all(), which
    with pytest.raises(shm.ShermanError) as e:
        t.export(keys=sentinels(n - 1), vals=sentinels(n))
    assert e.value.rc == shm.SHM_ENOSPC
    # count only: null outputs, cap ignored
    assert raw_export(t, 0, KEY_MAX, None, None, 0) == (shm.SHM_OK, n)
    assert raw_export(t, int(keys[10]), int(keys[19]), None, None, 3) == (shm.SHM_OK, 10)
    assert t.last_error()["bits"] == 0
    t.close()


# ---- 5. grown trees ---------------------------------------------------------------

def grow(seed, phases=4, check=None):
    """Random insert, overwrite and delete chunks from an empty tree: about
    40 K keys, so leaves split and slots hold holes.  check(t, orc, phase)
    runs after each phase."""
    rng = np.random.default_rng(seed)
    t = tree()
    orc = OracleTree(ARENA)
    for ph in range(phases):
        stored, _ = orc.dump()
        new = rng.integers(1, KEY_MAX - 1, 14000, dtype=np.uint64)
        # a clustered run as well: a leaf splits into many
        new = np.concatenate([new, new[:40, None].repeat(30, 1).ravel() +
                              np.tile(np.arange(1, 31, dtype=U64), 40)])
        k, v = new, new ^ U64(0x5151 + ph)
        if stored.size:
            over = stored[rng.integers(0, stored.size, 3000)]
            dele = stored[rng.integers(0, stored.size, 4000)]
            k = np.concatenate([new, over, dele])
            v = np.concatenate([v, over ^ U64(ph + 7), np.zeros(dele.size, dtype=U64)])
        o = rng.permutation(k.size)
        k, v = k[o], v[o]
        for at in range(0, k.size, MAX_BATCH):
            t.insert_batch(dev(k[at:at + MAX_BATCH]), dev(v[at:at + MAX_BATCH]))
            orc.apply_batch(k[at:at + MAX_BATCH], v[at:at + MAX_BATCH])
        if check:
            check(t, orc, ph)
    return t, orc


def sorted_dump(orc):
    k, v = orc.dump()
    o = np.argsort(k, kind="stable")
    return k[o], v[o]


def test_grown_tree_against_the_oracle(lib_ok):
    def check(t, orc, ph):
        ok, ov = sorted_dump(orc)
        assert_export(t, ok, ov, what=f"phase {ph}")
        a, b = ok.size // 4, 3 * ok.size // 4
        assert_export(t, ok[a:b], ov[a:b], int(ok[a]), int(ok[b - 1]), what=f"phase {ph}, a range")

    t, orc = grow(5, check=check)
    ok, ov = sorted_dump(orc)
    assert 35000 < ok.size < 60000 and t.stats()["root_level"] >= 2
    mk, mv = model_of(t)
    assert np.array_equal(mk, ok) and np.array_equal(mv, ov)
    # a queued batch, no synchronise in between: the export sees it
    rng = np.random.default_rng(8)
    new = rng.integers(1, KEY_MAX - 1, 6000, dtype=np.uint64)
    dele = ok[rng.integers(0, ok.size, 2000)]
    k = np.concatenate([new, dele])
    v = np.concatenate([new ^ U64(0xAA), np.zeros(dele.size, dtype=U64)])
    side = torch.cuda.Stream()
    kd, vd = dev(k), dev(v)
    torch.cuda.synchronize()
    t.insert_batch_async(kd, vd, stream=side)
    gk, gv = t.export()
    orc.apply_batch(k, v)
    ok, ov = sorted_dump(orc)
    assert np.array_equal(host(gk), ok) and np.array_equal(host(gv), ov)
    t.synchronize()
    assert t.last_error()["bits"] == 0
    orc.close()
    t.close()


# ---- 6. after SHM_ENOMEM ----------------------------------------------------------

def test_export_after_the_arena_ran_out(lib_ok):
    """A 64-page arena, chunks of 512 hashed keys until SHM_ENOMEM: pages of
    the failed chunk may hang on their left sibling alone."""
    t = shm.Tree(arena_bytes=64 * PAGE, max_batch=4096)
    first = 1
    while True:
        assert first < 64 * 64, "the arena never ran out"
        kd = torch.empty(512, dtype=torch.int64, device="cuda")
        t.gen_keys(first, 512, kd)
        first += 512
        try:
            t.insert_batch(kd, kd ^ 0x1111)
        except shm.ShermanError as e:
            assert e.rc == shm.SHM_ENOMEM, e
            break
    t.last_error(reset=True)
    mk, mv = model_of(t)
    assert mk.size > 512
    assert t.count() == mk.size
    k, v = t.export()
    assert np.array_equal(host(k), mk) and np.array_equal(host(v), mv)
    c, sk, sv = t.scan_batch(dev([0]), mk.size + 1).result()
    assert int(c[0]) == mk.size
    assert np.array_equal(host(sk)[0, :mk.size], mk) and np.array_equal(host(sv)[0, :mk.size], mv)
    t.close()


# ---- 7. read-only -----------------------------------------------------------------

def test_export_changes_nothing(lib_ok):
    t, orc = grow(6, phases=2)
    ok, ov = sorted_dump(orc)
    orc.close()
    for _ in range(6):  # a read phase: the directory and the table are built
        gpu_search(t, ok[:4096])
    assert t.dir_stats()["builds"] >= 1
    before = (t.dump_image(), t.stats(), t.dir_stats()["builds"], t.vt_stats())
    assert_export(t, ok, ov)
    a, b = 100, ok.size - 100
    assert_export(t, ok[a:b], ov[a:b], int(ok[a]), int(ok[b - 1]))
    assert raw_export(t, 0, KEY_MAX, sentinels(8), None, 8)[0] == shm.SHM_ENOSPC
    after = (t.dump_image(), t.stats(), t.dir_stats()["builds"], t.vt_stats())
    assert before[0][1] == after[0][1] and np.array_equal(before[0][0], after[0][0])
    assert before[1:] == after[1:], (before[1:], after[1:])
    assert_gets(t, ok, ov, neighbours(ok), "after the exports")
    t.close()


# ---- 8. compaction ----------------------------------------------------------------

def check_compacted(t, keys, vals, lf, inf, node_id=0):
    n = keys.size
    img, root, pl = bm.build(keys, vals, lf, inf, node_id)
    assert shm.bulk_plan(n, lf, inf) == pl
    got, groot = t.dump_image()
    assert groot == root == (1 << 26) | node_id
    assert got.size == img.size and np.array_equal(got[PAGE:], img[PAGE:])
    st = t.stats()
    assert st["pages_used"] == pl["pages"] and st["root_level"] == pl["root_level"], st
    assert t.check() == bm.counts(pl, n)
    assert_gets(t, keys, vals, neighbours(keys), "compacted")
    if n:
        froms = np.array([0, keys[n // 2]], dtype=U64)
        for model, call in ((ScanModel(keys, vals), t.scan_batch),
                            (RScanModel(keys, vals), t.rscan_batch)):
            c, k, v = call(dev(froms), 100).result()
            mc, mk, mv, w = model.scan(froms, 100)
            assert np.array_equal(c.cpu().numpy(), mc)
            assert np.array_equal(host(k)[w], mk[w]) and np.array_equal(host(v)[w], mv[w])
    assert_export(t, keys, vals, what="compacted")
    return got, groot


def later_chunk(t, img, root, keys, seed, node_id=0):
    """inserts and deletes after a compaction, against an oracle loaded with
    the compacted image"""
    orc = OracleTree(image=img, root_ptr=root, spare_bytes=8 << 20, node_id=node_id)
    rng = np.random.default_rng(seed)
    new = rng.integers(1, KEY_MAX - 1, 3000, dtype=np.uint64)
    dele = keys[rng.integers(0, keys.size, 1000)]
    k = np.concatenate([new, dele])
    v = np.concatenate([new ^ U64(0x33), np.zeros(dele.size, dtype=U64)])
    o = rng.permutation(k.size)
    t.insert_batch(dev(k[o]), dev(v[o]))
    orc.apply_batch(k[o], v[o])
    ok, ov = sorted_dump(orc)
    orc.close()
    assert_export(t, ok, ov, what="after a later chunk")
    assert_gets(t, ok, ov, dele[~np.isin(dele, ok)], "after a later chunk")
    assert t.check()["keys"] == ok.size


@pytest.mark.parametrize("lf,inf", [(0, 0), (53, 60)])
def test_compact_a_grown_tree(lib_ok, lf, inf):
    t, orc = grow(7, phases=3)
    ok, ov = sorted_dump(orc)
    orc.close()
    gpu_search(t, ok[:2048])  # a directory to drop
    used = t.stats()["pages_used"]
    t.compact(lf, inf)
    img, root = check_compacted(t, ok, ov, lf, inf)
    if lf == 53:  # splits leave leaves at 36 of 54 or fuller: only a denser fill must shrink it
        assert t.stats()["pages_used"] < used
    later_chunk(t, img, root, ok, 70 + lf)
    t.close()


@pytest.mark.parametrize("lf,inf,node_id", [(0, 0, 0), (53, 60, 3)])
def test_compact_a_tall_image(lib_ok, lf, inf, node_id):
    img, root, info = ib.build_tall(4, "middle", True, node_id=node_id)
    t = tree(node_id=node_id)
    t.load_image(img, root)
    t.compact(lf, inf)
    got, groot = check_compacted(t, info["keys"], info["vals"], lf, inf, node_id)
    later_chunk(t, got, groot, info["keys"], 80 + lf, node_id)
    t.close()


def test_compact_a_tree_emptied_by_deletes(lib_ok):
    keys, vals = shape(5000, 0, 0)
    t = tree()
    t.insert_batch(dev(keys), dev(vals))
    t.del_batch(dev(keys))
    assert t.count() == 0 and t.stats()["pages_used"] > 100
    k, v = t.export()
    assert k.numel() == 0 and v.numel() == 0
    t.compact()
    none = np.zeros(0, dtype=U64)
    check_compacted(t, none, none, 0, 0)
    assert t.stats()["pages_used"] == 1 and t.stats()["root_level"] == 0
    t.insert_batch(dev(keys[:100]), dev(vals[:100]))
    assert_export(t, keys[:100], vals[:100])
    t.close()


def test_rejected_compactions_leave_the_tree_alone(lib_ok):
    """Fills out of range; a plan too tall for the pairs (leaf_fill 1 under
    internal_fill 2 holds 3^7 = 2187 keys at most, so on 40 K keys
    shm_bulk_plan itself says SHM_EINVAL); a plan of more pages than the arena
    has (66 K keys at one per leaf in the arena's 65,535 pages: SHM_ENOMEM);
    an outstanding insert ticket."""
    n = 66000
    keys = bm.shape_keys(n, "spread", seed=3)
    vals = bm.shape_vals(keys)
    t = tree()
    t.bulk_load(dev(keys), dev(vals), 53, 60)
    drop = keys[::3]
    t.del_batch(dev(drop[:MAX_BATCH]))
    t.del_batch(dev(drop[MAX_BATCH:]))
    live = ~np.isin(keys, drop)
    keys, vals = keys[live], vals[live]
    gpu_search(t, keys[:2048])
    before, broot = t.dump_image()
    stats = t.stats()

    def unchanged(what):
        now, nroot = t.dump_image()
        assert nroot == broot and np.array_equal(now, before), what
        assert t.stats() == stats, what

    for lf, inf in ((54, 0), (0, 1), (0, 61)):
        with pytest.raises(shm.ShermanError) as e:
            t.compact(lf, inf)
        assert e.value.rc == shm.SHM_EINVAL
    unchanged("bad fills")
    with pytest.raises(shm.ShermanError) as e:
        shm.bulk_plan(keys.size, 1, 2)
    assert e.value.rc == shm.SHM_EINVAL
    with pytest.raises(shm.ShermanError) as e:
        t.compact(1, 2)
    assert e.value.rc == shm.SHM_EINVAL
    unchanged("too tall")
    # back to 66 K keys: one per leaf no longer fits the arena
    t.insert_batch(dev(drop[:MAX_BATCH]), dev(drop[:MAX_BATCH] | U64(1)))
    t.insert_batch(dev(drop[MAX_BATCH:]), dev(drop[MAX_BATCH:] | U64(1)))
    assert t.count() == n
    assert shm.bulk_plan(n, 1, 60)["pages"] + 1 > stats["pages_capacity"] + 1
    assert shm.bulk_plan(n, 1, 60)["root_level"] <= 7
    before, broot = t.dump_image()
    stats = t.stats()
    with pytest.raises(shm.ShermanError) as e:
        t.compact(1, 60)
    assert e.value.rc == shm.SHM_ENOMEM
    unchanged("too many pages")
    tk = t.insert_order(dev(keys[:10]), dev(vals[:10]))
    with pytest.raises(shm.ShermanError) as e:
        t.compact()
    assert e.value.rc == shm.SHM_EINVAL
    t.insert_apply(tk)
    t.synchronize()
    t.compact(53, 60)
    assert t.count() == n and t.stats()["pages_used"] == shm.bulk_plan(n, 53, 60)["pages"]
    t.close()


# ---- 9. size ----------------------------------------------------------------------

def test_a_million_keys(lib_ok):
    N = 1 << 20
    t = shm.Tree(arena_bytes=128 << 20, max_batch=N)
    kd = torch.empty(N, dtype=torch.int64, device="cuda")
    t.gen_keys(1, N, kd)
    keys = np.sort(host(kd))
    assert (keys[1:] > keys[:-1]).all()
    vals = bm.shape_vals(keys)
    t.bulk_load(dev(keys), dev(vals))
    t.del_batch(dev(keys[::3]))
    live = np.ones(N, dtype=bool)
    live[::3] = False
    keys, vals = keys[live], vals[live]
    assert t.count() == keys.size
    k, v = t.export()
    assert np.array_equal(host(k), keys) and np.array_equal(host(v), vals)
    used = t.stats()["pages_used"]
    t.compact()
    st = t.stats()
    assert st["pages_used"] == shm.bulk_plan(keys.size)["pages"] < used, (st, used)
    k, v = t.export()
    assert np.array_equal(host(k), keys) and np.array_equal(host(v), vals)
    assert t.last_error()["bits"] == 0
    t.close()
