"""Bulk load on the GPU (Tree.bulk_load -> shm_bulk_load -> bulk.hip): the
pages against the numpy model (tests/bulk_model.py) byte for byte, every
reader on the loaded tree, writes after a load against the CPU oracle, a load
over an existing tree, rejected inputs, and a 2^20-key load.

The models (bulk_model, scan_model, rscan_model) share no code with the
library.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bulk_model as bm  # noqa: E402
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


@functools.lru_cache(maxsize=None)
def shape(n, lf, inf, node_id=0):
    """keys, values, the model image, its root and plan (read only)"""
    keys = bm.shape_keys(n, bm.shape_kind(n, lf, inf))
    vals = bm.shape_vals(keys)
    img, root, pl = bm.build(keys, vals, lf, inf, node_id)
    for a in (keys, vals, img):
        a.setflags(write=False)
    return keys, vals, img, root, pl


def assert_gets(t, keys, vals, absent, what):
    """every key with its value, every absent probe a miss with value 0"""
    gv, gf = gpu_search(t, keys)
    bad = np.nonzero((gf != 1) | (gv != vals))[0]
    assert bad.size == 0, (what, bad.size, [hex(int(keys[i])) for i in bad[:4]])
    if absent.size:
        gv, gf = gpu_search(t, absent)
        bad = np.nonzero((gf != 0) | (gv != 0))[0]
        assert bad.size == 0, (what, "absent", bad.size, [hex(int(absent[i])) for i in bad[:4]])


def neighbours(keys, cap=4000):
    """key +- 1 of (a sample of) the keys, where no key is stored"""
    k = keys[::keys.size // cap + 1] if keys.size else keys
    p = np.concatenate([k + U64(1), k - U64(1), np.array([0, 1, KEY_MAX - 1], dtype=U64)])
    return np.unique(p[~np.isin(p, keys) & (p != U64(KEY_MAX))])


def assert_image(t, n, img, root, pl, what=""):
    got, groot = t.dump_image()
    assert groot == root, (what, hex(groot), hex(root))
    assert got.size == img.size == (pl["pages"] + 1) * PAGE, (what, got.size, img.size)
    diff = np.nonzero(got[PAGE:] != img[PAGE:])[0]
    if diff.size:
        at = int(diff[0]) + PAGE
        raise AssertionError(f"{what}: {diff.size} bytes differ, first at page {at // PAGE} "
                             f"offset {at % PAGE}: gpu {got[at]} model {img[at]}")
    st = t.stats()
    assert st["root_ptr"] == root and st["root_level"] == pl["root_level"], (what, st)
    assert st["height"] == pl["root_level"] + 1 and st["pages_used"] == pl["pages"], (what, st)
    assert t.check() == bm.counts(pl, n), what


# ---- 1. the bytes ---------------------------------------------------------------

@pytest.mark.parametrize("n,lf,inf,node_id", [s + (0,) for s in bm.SHAPES] + [(5000, 0, 0, 3),
                                                                             (54, 53, 60, 3)])
def test_pages_equal_the_model_byte_for_byte(lib_ok, n, lf, inf, node_id):
    keys, vals, img, root, pl = shape(n, lf, inf, node_id)
    assert shm.bulk_plan(n, lf, inf) == pl
    t = shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH, node_id=node_id)
    t.bulk_load(dev(keys), dev(vals), lf, inf)
    assert_image(t, n, img, root, pl)
    assert_gets(t, keys, vals, neighbours(keys), "after the load")
    assert t.last_error()["bits"] == 0
    t.close()


# ---- 2. every reader ------------------------------------------------------------

def check_scans(t, keys, vals, froms, limit):
    for model, call in ((ScanModel(keys, vals), t.scan_batch), (RScanModel(keys, vals), t.rscan_batch)):
        n = froms.size
        ko = torch.full((n, limit), SENT, dtype=torch.int64, device="cuda")
        vo = torch.full((n, limit), SENT, dtype=torch.int64, device="cuda")
        co = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        c, k, v = call(dev(froms), limit, keys=ko, vals=vo, counts=co).result()
        c, k, v = c.cpu().numpy(), host(k), host(v)
        mc, mk, mv, w = model.scan(froms, limit)
        bad = np.nonzero(c != mc)[0]
        assert bad.size == 0, (call.__name__, limit, bad.size, hex(int(froms[bad[0]])),
                               c[bad[0]], mc[bad[0]])
        assert np.array_equal(k[w], mk[w]) and np.array_equal(v[w], mv[w]), (call.__name__, limit)
        assert (k[~w] == U64(SENT)).all() and (v[~w] == U64(SENT)).all()


def check_readers(t, keys, vals, what):
    absent = neighbours(keys)
    assert_gets(t, keys, vals, absent, what)
    mix = np.random.default_rng(3).permutation(keys.size)
    assert_gets(t, keys[mix], vals[mix], absent[::-1], what + ", shuffled")
    # a batch large enough for the ordering pass of sort_gets (8192 gets)
    reps = -(-8192 // keys.size)
    assert_gets(t, np.tile(keys[mix], reps)[:MAX_BATCH], np.tile(vals[mix], reps)[:MAX_BATCH],
                absent[:0], what + ", a large batch")
    froms = np.unique(np.concatenate([keys[::keys.size // 1500 + 1], absent[::absent.size // 1500 + 1],
                                      np.array([0, keys[0], keys[-1], KEY_MAX - 1, KEY_MAX],
                                               dtype=U64)]))
    for limit in (1, 10, 60):
        check_scans(t, keys, vals, froms, limit)
    froms = froms[froms != U64(KEY_MAX)]
    found, k, v = t.lower_bound_batch(dev(froms))
    at = np.searchsorted(keys, froms, side="left")
    has = at < keys.size
    assert np.array_equal(found.cpu().numpy(), has), what
    at = np.minimum(at, keys.size - 1)
    assert np.array_equal(host(k)[has], keys[at][has]) and np.array_equal(host(v)[has], vals[at][has])
    found, k, v = t.floor_batch(dev(froms))
    at = np.searchsorted(keys, froms, side="right") - 1
    has = at >= 0
    assert np.array_equal(found.cpu().numpy(), has), what
    at = np.maximum(at, 0)
    assert np.array_equal(host(k)[has], keys[at][has]) and np.array_equal(host(v)[has], vals[at][has])
    # range scans: a loaded leaf holds its keys in slot order, so the values
    # come in key order
    lo = np.array([0, keys[0], keys[keys.size // 3], keys[keys.size // 2] + U64(1), keys[-1],
                   min(int(keys[-1]) + 1, KEY_MAX - 1), keys[5]], dtype=U64)
    hi = np.array([KEY_MAX - 1, keys[0], keys[2 * keys.size // 3], keys[keys.size // 2 + 70],
                   KEY_MAX - 1, KEY_MAX - 1, keys[4]], dtype=U64)
    counts, got = t.range_query_batch(dev(lo), dev(hi))
    counts, got = counts.cpu().numpy(), host(got)
    a = np.searchsorted(keys, lo, side="left")
    b = np.maximum(np.searchsorted(keys, hi, side="right"), a)
    assert np.array_equal(counts, b - a), (what, counts, b - a)
    assert np.array_equal(got, np.concatenate([vals[x:y] for x, y in zip(a, b)])), what
    assert t.last_error()["bits"] == 0, (what, t.last_error())


READ_TREES = {
    "default": {},
    "no_dir": {"leaf_dir": False},
    "sorted": {"sort_gets": True},
    "page_check": {"page_check": True},
}


@pytest.mark.parametrize("kind", list(READ_TREES))
@pytest.mark.parametrize("n,lf,inf", [(5000, 0, 0), (1000, 1, 2), (53 * 61, 53, 60)])
def test_every_reader_on_a_loaded_tree(lib_ok, n, lf, inf, kind):
    """Gets, ascending and descending scans, lower bounds, floors and range
    scans: as loaded (the first get builds the directory), then in a read
    phase, where the default tree answers from the pair-form directory and
    the bucket table."""
    keys, vals, img, root, pl = shape(n, lf, inf)
    t = shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH, **READ_TREES[kind])
    t.bulk_load(dev(keys), dev(vals), lf, inf)
    check_readers(t, keys, vals, "as loaded")
    for _ in range(6):
        gpu_search(t, keys[:512])
    ds = t.dir_stats()
    if kind == "no_dir":
        assert ds["form"] == "none", ds
    else:
        assert ds["form"] == "pairs" and ds["exact"], ds
        dv = t.dir_verify()
        assert dv["checked"] > 0, dv
        assert dv["bad_lists"] == dv["bad_pairs"] == dv["bad_fps"] == dv["bad_vals"] == 0, dv
    if kind == "default":
        assert t.vt_stats()["trusted"], t.vt_stats()
    check_readers(t, keys, vals, "read phase")
    assert_image(t, n, img, root, pl, "after the reads")
    t.close()


# ---- 3. writes after a load -----------------------------------------------------

def entry_bytes(image, page, slot):
    at = page * PAGE + bm.OFF_RECORDS + bm.LEAF_ENTRY * slot
    return bytes(image[at:at + bm.LEAF_ENTRY])


@pytest.mark.parametrize("n,lf,inf", [(53 * 61, 53, 60), (1000, 1, 2)])
def test_writes_after_a_load_agree_with_the_oracle(lib_ok, n, lf, inf):
    """The loaded image in the oracle, then the same chunks on both: 60 % new
    keys, 25 % overwrites, 15 % deletes, with gets between the chunks so that
    the chunks keep a directory.  At (53 * 61, 53, 60) the first new keys
    split a full leaf and the full root, which grows in place; at (1000, 1, 2)
    the tree stands at level 7 with one entry per leaf.

    Compared after each chunk: every get, the key count of both structural
    checks, and that both checks pass.  The leaf and internal page counts are
    not compared: the oracle splits one page in two at the 54th entry, the
    GPU cuts an overfull leaf into pages of 36 (layout.h kLeafSplitFill), so
    the two trees hold the same pairs in different numbers of pages."""
    keys, vals, img, root, pl = shape(n, lf, inf)
    t = shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH)
    t.bulk_load(dev(keys), dev(vals), lf, inf)
    got, groot = t.dump_image()
    orc = OracleTree(image=got, root_ptr=groot, spare_bytes=16 << 20)
    rc, osh = orc.check()
    assert rc == 0 and osh == dict(bm.counts(pl, n), height=pl["root_level"] + 1)
    gpu_search(t, keys[:256])  # a directory for the chunks to keep
    # one overwrite: the entry's 18 bytes as the reference writes them
    # (f and r go from 1 to 2 on both only if the load's f = r = 1 was right)
    i = n // 2
    first = bm.deal(n, pl["level_pages"][0])
    leaf = int(np.searchsorted(first, i, side="right")) - 1
    page, slot = (2 if pl["root_level"] else 1) + leaf, i - int(first[leaf])
    before = entry_bytes(got, page, slot)
    assert before[0] == 1 and before[17] == 1
    one_k, one_v = keys[i:i + 1], np.array([0xABCDEF0123], dtype=U64)
    t.insert_batch(dev(one_k), dev(one_v))
    orc.apply_batch(one_k, one_v)
    mine, theirs = entry_bytes(t.dump_image()[0], page, slot), entry_bytes(orc.image(), page, slot)
    assert mine == theirs and mine != before, (mine.hex(), theirs.hex(), before.hex())
    rng = np.random.default_rng([n, lf, inf])
    for b in range(6):
        ok, ov = orc.dump()
        new = rng.integers(1, KEY_MAX - 1, 2600, dtype=np.uint64)
        new = rng.permutation(np.unique(new[~np.isin(new, ok)]))[:2458]
        # overwrites and deletes are drawn with repeats (the 1,000-key tree
        # has fewer keys than its first chunk has such ops): the last writer
        # in chunk order wins on both trees
        over, dele = ok[rng.integers(0, ok.size, 1024)], ok[rng.integers(0, ok.size, 614)]
        k = np.concatenate([new, over, dele])
        v = np.concatenate([new ^ U64(0x6666),
                            over ^ (np.arange(1024, dtype=U64) << U64(8)) ^ U64(b + 1),
                            np.zeros(dele.size, dtype=U64)])
        assert k.size == 4096 and new.size == 2458 and (v[:3482] != 0).all()
        o = rng.permutation(k.size)
        t.insert_batch(dev(k[o]), dev(v[o]))
        orc.apply_batch(k[o], v[o])
        assert t.last_error()["bits"] == 0, (b, t.last_error())
        ok, ov = orc.dump()
        assert np.isin(new, ok).all() and n < ok.size < n + (b + 1) * 2458
        gone = dele[~np.isin(dele, ok)]
        assert gone.size > 50
        assert_gets(t, ok, ov, np.concatenate([gone, neighbours(ok, 500)]), f"chunk {b}")
        rc, osh = orc.check()
        st = t.check()
        assert rc == 0 and st["keys"] == osh["keys"] == ok.size, (b, rc, st, osh)
    assert t.stats()["root_level"] >= pl["root_level"]
    if (n, lf, inf) == (53 * 61, 53, 60):
        assert t.stats()["root_level"] == 2 and t.stats()["root_ptr"] == root  # grew in place
    orc.close()
    t.close()


# ---- 4. a load replaces the tree ------------------------------------------------

@pytest.mark.parametrize("leaf_dir", [True, False])
def test_a_load_replaces_the_tree(lib_ok, leaf_dir):
    rng = np.random.default_rng(44)
    old = np.unique(rng.integers(1, KEY_MAX - 1, 20400, dtype=np.uint64))[:20000]
    old = old[rng.permutation(old.size)]
    t = shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH, leaf_dir=leaf_dir)
    for at in range(0, old.size, MAX_BATCH):
        t.insert_batch(dev(old[at:at + MAX_BATCH]), dev(old[at:at + MAX_BATCH] ^ U64(0x33)))
    # a read phase: the bucket table is live
    for _ in range(6):
        gv, gf = gpu_search(t, old[:4096])
        assert gf.all()
    if leaf_dir:
        assert t.vt_stats()["trusted"], t.vt_stats()
    old_pages = t.stats()["pages_used"]
    keys = bm.shape_keys(3000, "spread", seed=9)
    keys = keys[~np.isin(keys, old)]
    vals = bm.shape_vals(keys)
    img, root, pl = bm.build(keys, vals)
    assert pl["pages"] < old_pages
    t.bulk_load(dev(keys), dev(vals))
    assert not t.vt_stats()["trusted"]
    for again in range(2):  # the first search builds the directory, the second reads it
        assert_gets(t, keys, vals, old, f"search {again} after the load")
    # the old leaves past the new tree are not leaves any more: in a read
    # phase again (directory entries, summary lines, the table), still absent
    for _ in range(6):
        gpu_search(t, old[:4096])
    assert_gets(t, keys, vals, old, "read phase after the load")
    assert_image(t, keys.size, img, root, pl, "replace")
    # an image whose root is not page 1, then a load: the root is page 1
    timg, troot, info = ib.build_tall(3, "middle", True)
    assert troot != root
    t.load_image(timg, troot)
    assert t.stats()["root_ptr"] == troot
    assert_gets(t, info["keys"], info["vals"], keys[:100], "the tall image")
    t.bulk_load(dev(keys), dev(vals))
    assert_image(t, keys.size, img, root, pl, "after a loaded image")
    assert_gets(t, keys, vals, np.concatenate([old[:2000], info["keys"]]), "after a loaded image")
    # and writes go on: the allocator continues after the loaded pages
    t.insert_batch(dev(old[:8000]), dev(old[:8000] ^ U64(0x44)))
    assert_gets(t, np.concatenate([keys, old[:8000]]),
                np.concatenate([vals, old[:8000] ^ U64(0x44)]), old[8000:10000], "inserts after")
    assert t.check()["keys"] == keys.size + 8000
    t.close()


# ---- 5. rejections leave the tree alone -----------------------------------------

def test_rejected_loads_leave_the_tree_alone(lib_ok):
    old = bm.shape_keys(700, "spread", seed=5)
    old_v = bm.shape_vals(old)
    t = shm.Tree(arena_bytes=ARENA, max_batch=MAX_BATCH)
    t.bulk_load(dev(old), dev(old_v), 5, 4)
    gpu_search(t, old)
    before, broot = t.dump_image()
    n = 1000
    keys = bm.shape_keys(n, "spread", seed=6)
    keys = keys[~np.isin(keys, old)]
    n = keys.size
    vals = bm.shape_vals(keys)
    cases = []
    for i in (0, n - 2, 63, 255):
        k = keys.copy()
        k[i], k[i + 1] = keys[i + 1], keys[i]
        cases.append((f"swapped at {i}", k, vals))
        k = keys.copy()
        k[i + 1] = k[i]
        cases.append((f"equal at {i}", k, vals))
    k = keys.copy()
    k[-1] = KEY_MAX
    cases.append(("KEY_MAX last", k, vals))
    v = vals.copy()
    v[n // 2] = 0
    cases.append(("zero value", keys, v))

    def unchanged(what):
        now, nroot = t.dump_image()
        assert nroot == broot and np.array_equal(now, before), what
        assert_gets(t, old, old_v, keys[:500], what)

    for what, k, v in cases:
        with pytest.raises(shm.ShermanError) as e:
            t.bulk_load(dev(k), dev(v))
        assert e.value.rc == shm.SHM_EINVAL, what
        unchanged(what)
    with pytest.raises(shm.ShermanError) as e:
        t.bulk_load(dev(keys), dev(vals), 54, 0)
    assert e.value.rc == shm.SHM_EINVAL
    with pytest.raises(shm.ShermanError) as e:
        dense = np.arange(1, 2189, dtype=U64)  # 3^7 + 1 leaves of one: level 8
        t.bulk_load(dev(dense), dev(dense), 1, 2)
    assert e.value.rc == shm.SHM_EINVAL
    unchanged("bad fills, too tall")
    # an outstanding insert ticket
    tk = t.insert_order(dev(keys[:10]), dev(vals[:10]))
    with pytest.raises(shm.ShermanError) as e:
        t.bulk_load(dev(keys), dev(vals))
    assert e.value.rc == shm.SHM_EINVAL
    unchanged("with a ticket outstanding")
    t.insert_apply(tk)
    t.synchronize()
    assert_gets(t, keys[:10], vals[:10], keys[10:100], "the ticket's chunk")
    # the accepted input loads
    t.bulk_load(dev(keys), dev(vals))
    assert_gets(t, keys, vals, old, "accepted")
    t.close()
    # the arena: plan.pages + the superblock must fit
    pl = bm.plan(n)
    small = shm.Tree(arena_bytes=(pl["pages"] + 1 - 2) * PAGE, max_batch=1 << 10)
    few = keys[:20]
    small.bulk_load(dev(few), dev(vals[:20]))
    before, broot = small.dump_image()
    with pytest.raises(shm.ShermanError) as e:
        small.bulk_load(dev(keys), dev(vals))
    assert e.value.rc == shm.SHM_ENOMEM
    now, nroot = small.dump_image()
    assert nroot == broot and np.array_equal(now, before)
    assert_gets(small, few, vals[:20], keys[20:200], "after SHM_ENOMEM")
    small.close()
    fits = shm.Tree(arena_bytes=(pl["pages"] + 1) * PAGE, max_batch=1 << 10)
    fits.bulk_load(dev(keys), dev(vals))
    assert fits.stats()["pages_used"] == pl["pages"] == fits.stats()["pages_capacity"]
    assert_gets(fits, keys, vals, old[:200], "an arena that just fits")
    fits.close()


# ---- 6. size --------------------------------------------------------------------

def test_a_million_hashed_keys(lib_ok):
    N = 1 << 20
    t = shm.Tree(arena_bytes=128 << 20, max_batch=N)
    kd = torch.empty(N, dtype=torch.int64, device="cuda")
    t.gen_keys(1, N, kd)
    hk = host(kd)
    order = np.argsort(hk, kind="stable")
    keys = hk[order]
    vals = (U64(2) * (order.astype(U64) + U64(1)))
    assert (keys[1:] > keys[:-1]).all()
    t.bulk_load(dev(keys), dev(vals))
    pl = shm.bulk_plan(N)
    assert pl == bm.plan(N)
    assert t.check() == bm.counts(pl, N)
    st = t.stats()
    assert st["pages_used"] == pl["pages"] and st["root_level"] == pl["root_level"], st
    gv, gf = gpu_search(t, hk)  # generation order: unsorted gets
    assert gf.all() and np.array_equal(gv, U64(2) * np.arange(1, N + 1, dtype=U64))
    t.gen_keys(N + 1, N // 10, kd[:N // 10])
    miss = host(kd[:N // 10])
    miss = miss[~np.isin(miss, keys)]
    gv, gf = gpu_search(t, miss)
    assert not gf.any() and not gv.any()
    rng = np.random.default_rng(6)
    froms = rng.integers(0, KEY_MAX, 1000, dtype=np.uint64)
    check_scans(t, keys, vals, froms, 10)
    assert t.last_error()["bits"] == 0
    t.close()
